"""The published contract of csrc/wv_fx.hip through the C ABI, per sample against float64 (oracle/wv_oracle_fx.py): wv_fx_fir_bank beyond
what the product calls (strides, up to 8 filters, the interleaved layout, unequal zero / replicate pads, taps over several 1024-tap LDS
pieces), wv_fx_resample and its adjoint against the dense operator of the same kernel table at clip lengths around and below the filter's,
wv_fx_fold_replicate, and the band-pass / resample gradients of effects.apply_effect_backward against float64 autograd.  Every comparison
is max |got - ref| / max |ref| <= 2e-5, the project's filter bar, which tests/test_oracle_fx_dense.py shows to be fair for these inputs;
`exact` ones say so.  PARITY of the taps with julius / torchaudio stays unpinned (see waveverify_amd/effects.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fx_contract_cases as FC
from guard import Guards
from oracle import wv_oracle_fx as OF
from waveverify_amd import _lib
from waveverify_amd import effects as E

pytestmark = pytest.mark.gpu
BAR = FC.BAR
ROWS = FC.ROWS


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(got, ref) -> float:
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert np.isfinite(g).all()
    return float(np.abs(g - ref).max() / max(1e-300, np.abs(ref).max()))


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def untouched(out) -> None:
    torch.cuda.synchronize()
    out.check(expect_unwritten=torch.ones(out.t.shape, dtype=torch.bool))


# ================================================================== wv_fx_fir_bank
def fir_call(xg, tg, yg, rows, T, nf, L, stride, pl, pr, rep, il) -> int:
    return _lib.load().wv_fx_fir_bank(xg.t.data_ptr(), tg.t.data_ptr(), yg.t.data_ptr(), rows, T, nf, L, stride, pl, pr, rep, il, stream())


@pytest.mark.parametrize("case", FC.fir_cases(), ids=FC.fir_id)
def test_fir_bank_contract(case):
    L, nf, stride, rep, pads, il, T = case
    pl, pr = FC.fir_pads(pads, L)
    x, taps = FC.fir_inputs(case)
    ref = OF.fir_bank(x, taps, stride, pl, pr, rep, il)
    assert np.abs(ref).max() > 0
    g = Guards(offset=1)
    xg, tg = g.input(x, "x"), g.input(taps, "taps")
    yg = g.output(ref.shape, name="y")
    assert fir_call(xg, tg, yg, ROWS, T, nf, L, stride, pl, pr, rep, il) == 0
    g.check()                                                           # guards intact, inputs unchanged, every output written
    e = rel(yg.t, ref)
    print(f"RECORD fir_bank {FC.fir_id(case)} Tout={FC.fir_tout(case)}: {e:.3e}")
    assert e <= BAR
    first = bits(yg.t)
    yg.refill_pattern()
    assert fir_call(xg, tg, yg, ROWS, T, nf, L, stride, pl, pr, rep, il) == 0
    g.check()
    assert np.array_equal(bits(yg.t), first)


@functools.lru_cache(maxsize=None)
def _kernels(of, nf):
    k, width, orig, new = E.resample_kernels(of, nf)
    return k, width, orig, new, cu(k)


@pytest.mark.parametrize("T", FC.POLYPHASE_T)
@pytest.mark.parametrize("of,nf", FC.POLYPHASE_RATES)
def test_fir_bank_as_the_polyphase_resampler(of, nf, T):
    """The resampler is the FIR bank's interleaved, strided, zero-padded configuration: one filter per output phase, stride = orig,
    width zeros in front and width + orig behind.  Its first t_out outputs are wv_fx_resample's, and both are the dense operator's."""
    k, width, orig, new, kd = _kernels(of, nf)
    L = k.shape[1]
    x, _ = FC.resample_inputs(of, nf, T, 1)
    t_out = E.resampled_length(T, of, nf)
    n_out = (T + 2 * width + orig - L) // orig + 1
    assert n_out * new >= t_out
    g = Guards(offset=1)
    xg, yg = g.input(x, "x"), g.output((ROWS, n_out * new), name="y")
    assert _lib.load().wv_fx_fir_bank(xg.t.data_ptr(), kd.data_ptr(), yg.t.data_ptr(), ROWS, T, new, L, orig, width, width + orig, 0, 1, stream()) == 0
    g.check()
    res = E.resample_waveform(cu(x), of, nf)
    ref = x.astype(np.float64) @ OF.resample_matrix(k, T, orig, new, width, t_out).T
    e_res, e_ref = rel(yg.t[:, :t_out], res.cpu().numpy().astype(np.float64)), rel(yg.t[:, :t_out], ref)
    print(f"RECORD polyphase {of}->{nf} T={T}: vs wv_fx_resample {e_res:.3e}, vs the dense operator {e_ref:.3e}")
    assert e_res <= BAR and e_ref <= BAR and rel(res, ref) <= BAR


def test_fir_bank_refusals_leave_the_output_alone():
    rng = np.random.default_rng(3)
    T, L = 64, 5
    g = Guards(offset=1)
    xg = g.input(rng.standard_normal((ROWS, T)).astype(np.float32), "x")
    tg = g.input(rng.standard_normal((9, L)).astype(np.float32), "taps")
    yg = g.output((ROWS, 9, T), name="y")
    for what, (rows, t, nf, l, stride, pl, pr) in [("n_filters = 9", (ROWS, T, 9, L, 1, 0, 0)),
                                                   ("T + pad_l + pad_r < L", (ROWS, 2, 1, L, 1, 1, 1)),
                                                   ("LDS past 64 KB", (ROWS, T, 1, L, 64, 0, 0)),
                                                   ("n_filters = 0", (ROWS, T, 0, L, 1, 0, 0)), ("stride = 0", (ROWS, T, 1, L, 0, 0, 0))]:
        for rep in (0, 1):
            assert fir_call(xg, tg, yg, rows, t, nf, l, stride, pl, pr, rep, 0) != 0, what
            untouched(yg)
    # rows = 65536 on buffers that do hold 65536 rows
    xb = g.input(np.zeros((65536, 4), np.float32), "x 65536 rows")
    yb = g.output((65536, 1, 4), name="y 65536 rows")
    assert fir_call(xb, tg, yb, 65536, 4, 1, 1, 1, 0, 0, 0, 0) != 0
    untouched(yb)
    assert fir_call(xg, tg, yg, ROWS, T, 8, L, 1, 2, 2, 1, 0) == 0          # the same buffers, inside the contract: served
    torch.cuda.synchronize()
    xg.check(); tg.check(); xb.check()
    left = yg.unwritten().flatten()                                         # y [ROWS][8][64] at the front of the 9-filter buffer
    assert not left[:ROWS * 8 * T].any() and left[ROWS * 8 * T:].all() and not yg.guard_report()


# ================================================================== wv_fx_resample / wv_fx_resample_adjoint
@pytest.mark.parametrize("of,nf,T", FC.resample_cases())
def test_resample_and_adjoint_vs_the_dense_operator(of, nf, T):
    k, width, orig, new, kd = _kernels(of, nf)
    L = k.shape[1]
    lib = _lib.load()
    t_product = E.resampled_length(T, of, nf)
    t_outs = FC.resample_t_outs(T, orig, new)
    assert t_outs[0] == t_product and t_outs[-1] == FC.resample_t_max(T, orig, new) >= t_product
    A_max = OF.resample_matrix(k, T, orig, new, width, t_outs[-1])
    for t_out in t_outs:
        A = A_max[:t_out]
        x, d = FC.resample_inputs(of, nf, T, t_out)
        g = Guards(offset=1)
        xg, dg = g.input(x, "x"), g.input(d, "dy")
        yg, dxg = g.output((ROWS, t_out), name="y"), g.output((ROWS, T), name="dx")
        assert lib.wv_fx_resample(xg.t.data_ptr(), kd.data_ptr(), yg.t.data_ptr(), ROWS, T, orig, new, L, width, t_out, stream()) == 0
        assert lib.wv_fx_resample_adjoint(dg.t.data_ptr(), kd.data_ptr(), dxg.t.data_ptr(), ROWS, T, orig, new, L, width, t_out, stream()) == 0
        g.check()
        e_fwd, e_adj = rel(yg.t, x.astype(np.float64) @ A.T), rel(dxg.t, d.astype(np.float64) @ A)
        print(f"RECORD resample {of}->{nf} T={T} t_out={t_out}: forward {e_fwd:.3e}, adjoint {e_adj:.3e}")
        assert e_fwd <= BAR and e_adj <= BAR
        if t_out == t_product:                                          # the product's wrappers make exactly these calls
            assert np.array_equal(bits(E.resample_waveform_adjoint(cu(d), of, nf, T)), bits(dxg.t))
            assert np.array_equal(bits(E.resample_waveform(cu(x), of, nf)), bits(yg.t))
    # one past the stated maximum: the forward is refused and writes nothing
    g = Guards(offset=1)
    xg, yg = g.input(x, "x"), g.output((ROWS, t_outs[-1] + 1), name="y")
    assert lib.wv_fx_resample(xg.t.data_ptr(), kd.data_ptr(), yg.t.data_ptr(), ROWS, T, orig, new, L, width, t_outs[-1] + 1, stream()) != 0
    untouched(yg)
    xg.check()


# ================================================================== wv_fx_fold_replicate
@pytest.mark.parametrize("T", FC.FOLD_T)
def test_fold_replicate_vs_float64(T):
    lib = _lib.load()
    for pl, pr in FC.FOLD_PADS:
        dxp = np.random.default_rng([T, pl, pr]).standard_normal((ROWS, T + pl + pr)).astype(np.float32)
        ref = OF.fold_replicate(dxp, T, pl, pr)
        g = Guards(offset=1)
        sg, og = g.input(dxp, "dxp"), g.output((ROWS, T), name="dx")
        assert lib.wv_fx_fold_replicate(sg.t.data_ptr(), og.t.data_ptr(), ROWS, T, pl, pr, stream()) == 0
        g.check()
        e = rel(og.t, ref)
        print(f"RECORD fold_replicate T={T} pads=({pl},{pr}): {e:.3e}")
        assert e <= BAR
        if T > 2:                                                       # the samples between the two ends are plain copies: exact
            assert np.array_equal(og.t.cpu().numpy()[:, 1:-1], dxp[:, pl + 1:pl + T - 1])
        first = bits(og.t)
        og.refill_pattern()
        assert lib.wv_fx_fold_replicate(sg.t.data_ptr(), og.t.data_ptr(), ROWS, T, pl, pr, stream()) == 0
        g.check()
        assert np.array_equal(bits(og.t), first)


# ================================================================== the adjoints as the trainer calls them
@pytest.mark.parametrize("T", FC.EFFECT_T)
@pytest.mark.parametrize("name,params", FC.EFFECT_SETTINGS, ids=[f"{n}-{'-'.join(str(v) for v in p.values())}" for n, p in FC.EFFECT_SETTINGS])
def test_bandpass_and_resample_gradients_per_sample(name, params, T):
    """effects.apply_effect_backward against float64 autograd through the oracle's restatement of the effect (band-pass: two low-passes
    over one replicate padding; resample: there, back, cropped or zero-padded to T) -- every sample, the clip's edges included."""
    d = np.random.default_rng([T, len(name), *params.values()]).standard_normal((2, 1, T)).astype(np.float32)
    ref = OF.effect_gradient(name, params, d)
    got = E.apply_effect_backward(name, params, cu(d))
    e = rel(got, ref)
    print(f"RECORD {name} {params} T={T} gradient: {e:.3e}")
    assert e <= BAR
