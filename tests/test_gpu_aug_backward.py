"""The temporal augmentation's backward (csrc/wv_aug.hip aug_bwd_kernel, augment.inverse_map / backward_to_watermarked /
TemporalAugmenter.backward) on its own: bit-equal to an oracle that is derived from the forward (oracle/wv_oracle_aug.py, held to torch's
autograd by tests/test_oracle_fx_dense.py), for every sequence map with a known answer -- a roll's inverse shift, a permutation's inverse
with its dropped tail, both orders of a chunk swap -- and tied to the forward launch itself by the pairing <out, d_out> = <wm, d_wm> + the
share of the samples the plan replaced."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import aug_backward_cases as AC
from guard import Guards
from oracle import wv_oracle_aug as OA
from waveverify_amd import _lib
from waveverify_amd import augment as A

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def seqmap(m) -> A.SeqMap:
    _, mode, a, b, c, perm, t_out = m
    return A.SeqMap(mode, a, b, c, perm, t_out)


def oracle(d_out, plan, seg, m, T):
    _, mode, a, b, c, perm, _ = m
    return OA.backward_to_watermarked(d_out, plan, seg, mode, a, b, c, perm, T)


def test_mode_numbers_are_the_package_s():
    assert (AC.IDENTITY, AC.REVERSE, AC.ROLL, AC.PERMUTE, AC.CHUNK_SWAP) == (A.SEQ_IDENTITY, A.SEQ_REVERSE, A.SEQ_ROLL, A.SEQ_PERMUTE, A.SEQ_CHUNK_SWAP)


@pytest.mark.parametrize("case", AC.cases(), ids=AC.case_id)
def test_backward_is_the_oracle_s_and_pairs_with_the_forward(case):
    (B, Cc, T, seg), m = case
    sm = seqmap(m)
    rng = np.random.default_rng(B * 1000 + T + sm.mode)
    plan = AC.plan(B, T, seg, B * 1000 + T)
    forced = AC.forced_codes(B, plan.shape[1])
    assert set(forced) <= set(plan[0].tolist()) and 3 * int((plan == 0).sum()) >= plan.size
    orig = rng.standard_normal((B, Cc, T)).astype(np.float32)
    wm = rng.standard_normal((B, Cc, T)).astype(np.float32)
    d_out = rng.standard_normal((B, Cc, sm.t_out)).astype(np.float32)
    d_dev = cu(d_out)
    for p in (plan, None):
        ref = oracle(d_out, p, seg, m, T)
        assert ref.dtype == np.float32 and ref.shape == (B, Cc, T)
        got = A.backward_to_watermarked(d_dev, p, seg, sm, T)
        again = A.backward_to_watermarked(d_dev, p, seg, sm, T)
        g = got.cpu().numpy()
        assert g.shape == ref.shape and np.array_equal(g, ref), (m[0], p is None, int((g != ref).sum()), np.argwhere(g != ref)[:4].tolist())
        assert np.array_equal(bits(got), bits(again))
        assert np.array_equal(bits(d_dev), d_out.view(np.int32))                        # the incoming gradient is not written
        if sm.mode == A.SEQ_PERMUTE and sm.t_out < T:
            assert not g[..., sm.t_out:].any()                                           # the dropped tail: exact zeros
        # the pairing with the forward LAUNCH: out[t] is wm[src(t)] where the mask says so, something else where it does not
        wm_out, _, mask = (t.cpu().numpy().astype(np.float64) for t in A._launch(cu(orig), cu(wm), p, seg, sm))
        prod = wm_out * d_out.astype(np.float64)                                         # float32 x float32: exact in float64
        lhs = math.fsum(prod.ravel())
        rhs = math.fsum(np.concatenate([(wm.astype(np.float64) * g.astype(np.float64)).ravel(), prod[mask == 0]]))
        assert lhs == rhs, (m[0], lhs, rhs)                                              # exactly rounded sums of the same terms
        if p is None:
            assert bool((mask == 1).all())


@pytest.mark.parametrize("kind", ["identity", "reverse", "roll_Tdiv3", "permute_Tdiv7", "swap_b_lt_a_to_the_end"])
def test_backward_guarded_through_the_c_abi(kind):
    """One run per map kind on guarded, one-element-misaligned buffers at T = 999: nothing outside d_wm is written, every element of d_wm is
    (the zeros included), the inputs are untouched, and the result is the wrapper's bit for bit."""
    B, Cc, T, seg = AC.SHAPES[1]
    m = next(m for m in AC.maps(T) if m[0] == kind)
    sm = seqmap(m)
    inv = A.inverse_map(sm, T)
    rng = np.random.default_rng(T + sm.mode)
    plan = AC.plan(B, T, seg, 11)
    d_out = rng.standard_normal((B, Cc, sm.t_out)).astype(np.float32)
    g = Guards(offset=1)
    dg, pg = g.input(d_out, "d_out"), g.input(plan, "plan")
    permg = g.input(np.ascontiguousarray(inv.perm, dtype=np.int32), "inverse perm") if inv.perm is not None else None
    out = g.output((B, Cc, T), name="d_wm")
    rc = _lib.load().wv_aug_backward(dg.t.data_ptr(), pg.t.data_ptr(), plan.shape[1], seg, inv.mode, inv.a, inv.b, inv.c,
                                     permg.t.data_ptr() if permg is not None else None, out.t.data_ptr(), B, Cc, T, sm.t_out,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    g.check()
    want = A.backward_to_watermarked(cu(d_out), plan, seg, sm, T)
    assert np.array_equal(bits(out.t), bits(want)) and np.array_equal(want.cpu().numpy(), oracle(d_out, plan, seg, m, T))


# one numpy / torch seed per method SequenceAugmentation.draw returns, found on the CPU (B = 3, T = 999, draw_plan first, as forward() draws).
# 'unchanged' is drawn only where the clip is too short for two shuffle segments (the method's own branch needs u >= 0.3 + 0.4 + 0.3 = 1.0,
# which numpy's rand() never returns), so that one case uses sample_rate = 1000: a 500-sample segment against T = 999.
SEEDED = [("shuffle", 100, 0), ("circular_shift", 100, 1), ("reverse", 100, 6), ("unchanged", 1000, 0)]


@pytest.mark.parametrize("method,sample_rate,seed", SEEDED)
def test_temporal_augmenter_backward_after_a_seeded_forward(method, sample_rate, seed):
    B, T = 3, 999
    rng = np.random.default_rng(seed + 40)
    orig, wm = (rng.standard_normal((B, 1, T)).astype(np.float32) for _ in range(2))
    np.random.seed(seed); torch.manual_seed(seed)
    probe = A.TemporalAugmenter(sample_rate, 0.1)
    probe.localization_augmenter.draw_plan(B, T)
    assert probe.seq_augmenter.draw(B, T)[0] == method                                   # the hard-coded seed still draws this method
    np.random.seed(seed); torch.manual_seed(seed)
    aug = A.TemporalAugmenter(sample_rate, 0.1)
    sig, mask, _, _ = aug(cu(orig), cu(wm))
    plan, seg, sm, t_in = aug.last
    assert (seg, t_in) == (sample_rate // 10, T) and plan.shape == (B, -(-T // seg)) and (plan != 0).any()
    assert sm.mode == {"shuffle": A.SEQ_PERMUTE, "circular_shift": A.SEQ_ROLL, "reverse": A.SEQ_REVERSE, "unchanged": A.SEQ_IDENTITY}[method]
    if method == "shuffle":
        assert sm.a == sample_rate // 2 and sm.t_out == (T // sm.a) * sm.a < T
    d_out = rng.standard_normal((B, 1, sm.t_out)).astype(np.float32)
    assert sig.audio_data.shape == d_out.shape
    got = aug.backward(cu(d_out)).cpu().numpy()
    ref = OA.backward_to_watermarked(d_out, plan, seg, sm.mode, sm.a, sm.b, sm.c, sm.perm, T)
    assert got.shape == (B, 1, T) and np.array_equal(got, ref)
    # where the mask is 1 the augmented sample IS the watermarked one the gradient went to
    src = OA.apply_seqmap(np.arange(T), sm.mode, sm.a, sm.b, sm.c, sm.perm)
    kept = mask.cpu().numpy()[:, 0] == 1
    for b in range(B):
        assert np.array_equal(got[b, 0, src[kept[b]]], d_out[b, 0, kept[b]])


def test_backward_refuses_bad_maps_before_any_launch():
    B, Cc, T, seg = 2, 1, 100, 10
    lib = _lib.load()
    g = Guards(offset=1)
    dg = g.input(np.ones((B, Cc, T), np.float32), "d_out")
    pg = g.input(np.zeros((B, 10), np.int32), "plan")
    out = g.output((B, Cc, T), name="d_wm")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nseg, mode, a, b, c):
        return lib.wv_aug_backward(dg.t.data_ptr(), pg.t.data_ptr(), nseg, seg, mode, a, b, c, None, out.t.data_ptr(), B, Cc, T, T, stream)
    for what, args in [("roll by 0", (10, A.SEQ_ROLL, 0, 0, 0)), ("roll by T", (10, A.SEQ_ROLL, T, 0, 0)),
                       ("nseg != ceil(T / seg_len)", (9, A.SEQ_IDENTITY, 0, 0, 0)), ("nseg != ceil(T / seg_len)", (11, A.SEQ_IDENTITY, 0, 0, 0)),
                       ("overlapping chunks", (10, A.SEQ_CHUNK_SWAP, 0, 10, 25)), ("overlapping chunks", (10, A.SEQ_CHUNK_SWAP, 30, 10, 25))]:
        assert call(*args) != 0, what
        torch.cuda.synchronize()
        dg.check(); pg.check()
        out.check(expect_unwritten=torch.ones(out.t.shape, dtype=torch.bool))            # refused before any launch: nothing written
    assert call(10, A.SEQ_ROLL, 1, 0, 0) == 0                                            # the same buffers, a valid map: served
    g.check()
