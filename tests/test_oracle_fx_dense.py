"""The float64 oracles behind tests/test_gpu_fx_contract.py and tests/test_gpu_aug_backward.py, held on the CPU to what they restate: the
dense resample operator to oracle.wv_oracle_fx.resample, the FIR-bank formula to the julius-style lowpass, the fold to torch's autograd
through replicate padding, the augmentation backward to torch's autograd through the forward -- and the GPU tests' FIR inputs to the
condition that makes the project's 2e-5 filter bar fair for a float32 fma chain."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_backward_cases as AC
import fx_contract_cases as FC
from oracle import wv_oracle_aug as OA
from oracle import wv_oracle_fx as OF
from waveverify_amd import effects as E

TAPS_ROUNDING_CAP = FC.BAR / 10     # 2e-6: what the taps' float32 rounding may cost at the most, a tenth of the filter bar


def test_resample_matrix_is_the_oracle_resample_up_to_the_taps_rounding():
    """resample_matrix(float32 kernels) @ x against OF.resample(x) (float64 taps) for every (orig, new, T) of the GPU test: the two differ
    only by the float32 rounding of effects.resample_kernels' taps.  MEASURED over the 49 cases: the largest difference relative to the
    output's peak is 5.0e-8 (16000 -> 32000 at T = 255); asserted at ten times that, 5e-7, which is under the cap of 2e-6 (BAR / 10)."""
    bound = min(10 * 5.0e-8, TAPS_ROUNDING_CAP)
    worst = (0.0, None)
    for of, nf, T in FC.resample_cases():
        k, width, orig, new = E.resample_kernels(of, nf)
        assert (orig, new, width) == FC.resample_geometry(of, nf) and k.dtype == np.float32 and k.shape == (new, 2 * width + orig)
        x, _ = FC.resample_inputs(of, nf, T, 1)
        ref = OF.resample(x, of, nf)
        A = OF.resample_matrix(k, T, orig, new, width, ref.shape[-1])
        rel = float(np.abs(x.astype(np.float64) @ A.T - ref).max() / np.abs(ref).max())
        worst = max(worst, (rel, (of, nf, T)))
        assert rel <= bound, (of, nf, T, rel)
    print(f"MEASURED taps rounding: {worst[0]:.3e} at {worst[1]} over {len(FC.resample_cases())} cases")


def test_resample_matrix_rows_past_the_clip_and_the_stated_maximum():
    """Rows of a longer t_out than the product's are the same formula continued (the first rows do not change), and the rows past the
    last input sample that any tap reaches are zero."""
    k, width, orig, new = E.resample_kernels(16000, 12000)
    T = 37
    t = FC.resample_t_outs(T, orig, new)
    A, Amax = OF.resample_matrix(k, T, orig, new, width, t[0]), OF.resample_matrix(k, T, orig, new, width, t[-1])
    assert t[-1] == FC.resample_t_max(T, orig, new) > t[0] and np.array_equal(Amax[:t[0]], A)
    m_dead = -(-(T + width) // orig) * new                    # (m // new) * orig - width >= T: no tap inside the clip
    assert not OF.resample_matrix(k, T, orig, new, width, m_dead + new)[m_dead:].any()


@pytest.mark.parametrize("cutoff,T", [(0.375, 1001), (0.0625, 37), (0.5, 5)])
def test_fir_bank_is_the_lowpass_in_the_julius_configuration(cutoff, T):
    x = np.random.default_rng(T).standard_normal((3, T))
    half = int(8 / cutoff / 2)
    taps = OF.lowpass_filter_taps(cutoff, half)[None]
    got = OF.fir_bank(x, taps, 1, half, half, 1, 0)
    assert got.shape == (3, 1, T) and np.abs(got[:, 0] - OF.lowpass(x, cutoff)).max() <= 1e-12


def test_fir_bank_layouts_strides_and_paddings():
    """The formula against a second, scalar evaluation (one output at a time), interleaved and planar, ragged strides, unequal pads."""
    rng = np.random.default_rng(5)
    x, taps = rng.standard_normal((2, 11)), rng.standard_normal((3, 4))
    for stride, pl, pr, rep in [(1, 0, 0, 0), (2, 7, 0, 1), (3, 0, 13, 0), (4, 3, 3, 1), (3, 20, 0, 1)]:
        xp = np.stack([np.concatenate([np.full(pl, r[0] if rep else 0.0), r, np.full(pr, r[-1] if rep else 0.0)]) for r in x])
        n_out = (11 + pl + pr - 4) // stride + 1
        ref = np.array([[[sum(taps[f, j] * xp[r, n * stride + j] for j in range(4)) for n in range(n_out)] for f in range(3)] for r in range(2)])
        assert np.abs(OF.fir_bank(x, taps, stride, pl, pr, rep, 0) - ref).max() <= 1e-14
        assert np.array_equal(OF.fir_bank(x, taps, stride, pl, pr, rep, 1), OF.fir_bank(x, taps, stride, pl, pr, rep, 0).transpose(0, 2, 1).reshape(2, -1))
    with pytest.raises(ValueError):
        OF.fir_bank(x, rng.standard_normal((1, 12)), 1, 0, 0, 0, 0)


@pytest.mark.parametrize("T", FC.FOLD_T)
def test_fold_replicate_is_autograd_through_replicate_padding(T):
    rng = np.random.default_rng(T)
    for pl, pr in FC.FOLD_PADS:
        dxp = rng.standard_normal((3, T + pl + pr))
        x = torch.zeros(3, 1, T, dtype=torch.float64, requires_grad=True)
        (F.pad(x, (pl, pr), mode="replicate") * torch.from_numpy(dxp)[:, None]).sum().backward()
        assert np.abs(OF.fold_replicate(dxp, T, pl, pr) - x.grad.numpy()[:, 0]).max() <= 1e-12, (T, pl, pr)


@pytest.mark.parametrize("case", [c for c in AC.cases() if c[0] == AC.SHAPES[1]] + [c for c in AC.cases() if c[0] == AC.SHAPES[2]], ids=AC.case_id)
def test_aug_backward_oracle_is_autograd_through_the_forward(case):
    """The forward as an index gather times the keep mask (what apply_plan then apply_seqmap do to the watermarked input), differentiated
    by torch in float64: exactly the oracle's backward, for every map kind, with a plan and without."""
    (B, C, T, seg), (_, mode, a, b, c, perm, t_out) = case
    rng = np.random.default_rng(B + T)
    wm, orig = rng.standard_normal((B, C, T)), rng.standard_normal((B, C, T))
    d_out = rng.standard_normal((B, C, t_out))
    src = OA.apply_seqmap(np.arange(T), mode, a, b, c, perm)
    for plan in (AC.plan(B, T, seg, 7), None):
        keep = np.ones((B, 1, T)) if plan is None else (np.repeat(plan, seg, axis=1)[:, None, :T] == 0).astype(np.float64)
        w = torch.from_numpy(wm).requires_grad_(True)
        out = (w * torch.from_numpy(keep))[..., torch.from_numpy(src)]
        if plan is not None:                                   # the gather form IS the oracle's forward on the kept samples
            fw = OA.apply_seqmap(OA.apply_plan(orig, wm, plan, seg)[0], mode, a, b, c, perm)
            kept = keep[..., src].repeat(C, axis=1) == 1
            assert np.array_equal(out.detach().numpy()[kept], fw[kept])
        (out * torch.from_numpy(d_out)).sum().backward()
        got = OA.backward_to_watermarked(d_out, plan, seg, mode, a, b, c, perm, T)
        assert got.shape == (B, C, T) and np.array_equal(got, w.grad.numpy())
        if mode == AC.PERMUTE and t_out < T:
            assert not got[..., t_out:].any()


def test_aug_plans_hold_every_code_and_enough_kept_segments():
    for B, C, T, seg in AC.SHAPES:
        p = AC.plan(B, T, seg, B * 1000 + T)
        assert p.shape == (B, -(-T // seg)) and p.min() >= 0 and p.max() < 3 + B
        assert set(AC.forced_codes(B, p.shape[1])) <= set(p[0].tolist())
        assert 3 * int((p == 0).sum()) >= p.size


def test_fir_cases_cover_the_published_contract():
    cases = FC.fir_cases()
    assert 60 <= len(cases) <= 70 and len(set(cases)) == len(cases)
    for i, values in enumerate([FC.FIR_L, FC.FIR_NF, FC.FIR_STRIDE, [0, 1], FC.FIR_PADS, [0, 1]]):
        assert {c[i] for c in cases} == set(values), i
    assert {FC.fir_tout(c) for c in cases} == set(FC.FIR_TOUT)
    assert any(c[6] < FC.fir_pads(c[4], c[0])[0] for c in cases)                                   # a clip shorter than its front pad
    assert any(c[0] > 2048 and c[5] == 1 and c[2] == 4 for c in cases) and any(c[1] == 8 and c[0] == 2049 for c in cases)
    assert any(c[0] == 1 and c[2] == 3 for c in cases)
    for c in cases:                                          # what the entry point needs: the 64 KB of LDS
        assert (255 * c[2] + 1024 + c[1] * 1024) * 4 <= 64 * 1024


def test_fir_inputs_leave_the_bar_to_the_kernel():
    """For every input of the GPU FIR tests the formula in float32 numpy, taps in plain order (one rounded multiply and one rounded add per
    tap: no fma, so at least the error of the kernel's fma chain), stays within BAR / 4 = 5e-6 of the float64 oracle, relative to the
    output's peak.  MEASURED over the 65 cases: at most 3.1e-6 (L = 2500, one filter, stride 1, replicate 'half' pads, T = 599; the
    cases of at most 1025 taps stay at or below 1.3e-6), inside BAR / 4 with unit-L1 taps -- so a GPU result past BAR is the kernel's doing, not the
    arithmetic's."""
    worst = (0.0, None)
    for c in FC.fir_cases():
        L, nf, stride, rep, pads, il, T = c
        x, taps = FC.fir_inputs(c)
        assert np.allclose(np.abs(taps.astype(np.float64)).sum(1), 1.0, atol=1e-5)
        pl, pr = FC.fir_pads(pads, L)
        ref = OF.fir_bank(x, taps, stride, pl, pr, rep, il)
        f32 = OF.fir_bank(x, taps, stride, pl, pr, rep, il, dtype=np.float32)
        assert f32.dtype == np.float32 and ref.shape == f32.shape == ((FC.ROWS, FC.fir_tout(c) * nf) if il else (FC.ROWS, nf, FC.fir_tout(c)))
        rel = float(np.abs(f32 - ref).max() / np.abs(ref).max())
        worst = max(worst, (rel, FC.fir_id(c)))
        assert rel <= FC.BAR / 4, (FC.fir_id(c), rel)
    print(f"MEASURED float32 chain: {worst[0]:.3e} at {worst[1]}; BAR / 4 = {FC.BAR / 4:.1e}")


@pytest.mark.parametrize("name,params", FC.EFFECT_SETTINGS[:1] + FC.EFFECT_SETTINGS[3:4])
def test_effect_gradient_is_the_transposed_restatement(name, params):
    """effect_gradient against the oracle's own forward: <effect(x), d> == <x, gradient> in float64 (both are linear)."""
    T = 37
    rng = np.random.default_rng(T)
    x, d = rng.standard_normal((2, 1, T)), rng.standard_normal((2, 1, T))
    if name == "bandpass_filter":
        y = OF.bandpass(x, params["cutoff_freq_low"] / 8000.0, params["cutoff_freq_high"] / 8000.0)
    else:
        y = OF.resample(OF.resample(x, 16000, params["new_sample_rate"]), params["new_sample_rate"], 16000)
        y = y[..., :T] if y.shape[-1] >= T else np.pad(y, ((0, 0), (0, 0), (0, T - y.shape[-1])))
    g = OF.effect_gradient(name, params, d)
    assert abs((y * d).sum() - (x * g).sum()) <= 1e-12 * np.abs(y).max() * np.abs(d).sum()
