"""head16_kernel (csrc/wv_h16.hip) on its own, through wv_h16_head, against oracle/wv_oracle_h16.py's float64 restatement of its arithmetic
(head16_probs): L2Norm in the kernel's f32 operations, z and the composed head weight as f16, logits / sigmoid / time sums in float64.

What separates the two is f32 accumulation order, __expf / rcpf and the rare f16 boundary flip of z: the GPU's L2Norm scale can sit
an f32 ulp away from the restated one, and a z within that of an f16 rounding midpoint then rounds the other way, which moves that
frame's probabilities by up to ~1e-4 (measured once: 8.9e-5, exactly the reference's value with that frame's scale one ulp up).  So the
reference is taken over the scale moved by -2 .. +2 ulps, per frame (head16_bounds; a single value except for such frames), and the
bar is 1e-6 on a probability (sums add the f32 summation bound) -- the per-sample check (one kept sample per row) then sees a wrong time mapping, a wrong keep
mask or a wrong bit-to-wave assignment that a time mean would average away."""
import numpy as np
import pytest
import torch

from oracle import wv_oracle_h16 as O16

pytestmark = pytest.mark.gpu

# Bars, set from the MI355X (max over every case below, outside frames with a flipped z): per-sample probabilities 1.5e-7 measured, window
# sums 1.3e-7 per kept sample, means 2.6e-7 -- except where a clip's samples are all equal (the all-zero frame: sigmoid(bias) at every t),
# whose f32 sums round the same way at every step: 1.2e-6 measured (Fr = 2, hop = 320).  So sums and means are held to SAMPLE_BAR plus the
# f32 bound of a naive sum over the samples one lane adds (sum_slack); window sums per kept sample.
SAMPLE_BAR = 1e-6


def sum_slack(Fr, hop):
    """(n - 1) * 2^-24 relative for a naive f32 sum of n terms: a lane adds hop / 2 samples of each of its frames (two per 64-frame tile),
    then six butterfly steps across the wave."""
    return (hop // 2 * 2 * -(-Fr // 64) + 6) * 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def _weights(rng, D, nb, hop):
    wc = (1.5 / np.sqrt(D) * rng.standard_normal((D, nb * hop))).astype(np.float32)     # logits of order 1: the whole sigmoid is used
    bc = (0.5 * rng.standard_normal(nb)).astype(np.float32)
    return wc, bc


def _latent(rng, B, D, Fr):
    """Random frames with the edges of the L2Norm: an all-zero frame (the 1e-12 clamp), one of very large values (its f32 sum of squares
    still finite), one of tiny values whose norm is below the clamp, one small but above it."""
    lat = rng.standard_normal((B, D, Fr)).astype(np.float32)
    lat[-1, :, Fr - 1] *= np.float32(3e12)
    if Fr > 2:
        lat[B // 2, :, Fr // 2] *= np.float32(1e-15)
        lat[0, :, 1] *= np.float32(1e-9)
    lat[0, :, 0] = 0.0
    return lat


def _cases():
    Ds, nbs, hops, Frs = [16, 48, 64, 128], [4, 8, 16, 20, 32], [32, 64, 320, 640], [1, 2, 63, 64, 65, 127, 128, 129, 200]
    out = []
    for i in range(20):
        D, nb, hop, Fr = Ds[i % 4], nbs[i % 5], hops[(i // 5 + i) % 4], Frs[i % 9]
        B = 1 + (i * 3) % 5
        while B > 1 and B * Fr * nb * hop > 6_000_000:
            B -= 1
        T = (Fr * hop, (Fr - 1) * hop + 1, (Fr - 1) * hop + 1 + (7 * i + 3) % hop)[i % 3]
        out.append((B, D, Fr, nb, hop, T))
    return out + [(1, 128, 200, 32, 640, 200 * 640 - 1)]


@pytest.mark.parametrize("B,D,Fr,nb,hop,T", _cases())
def test_head16_mean_and_whole_range_sum(ops, B, D, Fr, nb, hop, T):
    """The mean output against the reference, and the windowed output over [0, T): T times the mean, to f32 summation order."""
    rng = np.random.default_rng(B * 1000 + D + Fr + nb + hop)
    lat, (wc, bc) = _latent(rng, B, D, Fr), _weights(rng, D, nb, hop)
    lo, hi = O16.head16_bounds(lat, wc, bc, T)
    got = ops.h16_head(torch.from_numpy(lat).cuda(), wc, bc, T).cpu().numpy()
    err = float(np.maximum(lo - got, got - hi).max())
    print(f"MEASURE head16 mean B={B} D={D} Fr={Fr} nb={nb} hop={hop} T={T}: {err:.2e} (reference interval {float((hi - lo).max()):.1e})")
    assert np.isfinite(got).all() and err <= SAMPLE_BAR + sum_slack(Fr, hop), err
    ps = ops.h16_head(torch.from_numpy(lat).cuda(), wc, bc, T, keep_lo=[0] * B, keep_hi=[T] * B).cpu().numpy()
    np.testing.assert_allclose(ps / np.float32(T), got, rtol=2.0 ** -21, atol=0)


def _per_sample_case(ops, D, nb, hop, Fr, T, ts, seed):
    rng = np.random.default_rng(seed)
    lat1, (wc, bc) = _latent(rng, 1, D, Fr), _weights(rng, D, nb, hop)
    p = np.stack([O16.head16_probs(lat1, wc, bc, inv_ulps=u)[0] for u in range(-2, 3)])    # [5, nb, Fr * hop]
    ts = np.asarray(sorted(ts), np.int32)
    lat = torch.from_numpy(lat1).cuda().expand(len(ts), D, Fr).contiguous()
    got = ops.h16_head(lat, wc, bc, T, keep_lo=ts, keep_hi=ts + 1).cpu().numpy()    # row r = sigmoid(logit(t_r)) of every bit
    return got, p, ts


@pytest.mark.parametrize("D,nb,hop,Fr", [(64, 16, 32, 130), (48, 20, 64, 66), (128, 32, 320, 3), (16, 4, 640, 2), (128, 8, 32, 200)])
def test_head16_per_sample(ops, D, nb, hop, Fr):
    """B copies of one latent, row r keeping only [t_r, t_r + 1): each psum entry is one sigmoid(logit), compared element by element --
    every sample of the first frame and of the frames at the 32- and 64-frame tile edges, a stride through the rest."""
    T = Fr * hop - 3
    ts = set(range(0, min(T, 2 * hop))) | set(range(0, T, 5))
    for f in (31, 32, 33, 63, 64, 65, 127, 128, 129, Fr - 1):
        ts |= {t for t in range(f * hop - 1, (f + 1) * hop + 1) if 0 <= t < T}
    got, p, ts = _per_sample_case(ops, D, nb, hop, Fr, T, ts, seed=D + nb + hop + Fr)
    err = float(np.abs(got[None] - p[:, :, ts].transpose(0, 2, 1)).min(axis=0).max())
    print(f"MEASURE head16 per-sample D={D} nb={nb} hop={hop} Fr={Fr}: {err:.2e} over {len(ts)} samples")
    assert err <= SAMPLE_BAR, err


def test_head16_keep_ranges(ops):
    """Window sums over keep ranges that straddle a frame boundary and a 64-frame tile boundary, start exactly on a tile edge (the kernel
    skips whole tiles before keep_lo), run past T, or are empty (exactly 0); one distinct latent per row."""
    for D, nb, hop, Fr in ((64, 8, 32, 200), (128, 16, 320, 140)):
        T = Fr * hop - 17
        E = 64 * hop
        ranges = [(5 * hop - 3, 5 * hop + 4), (E - 10, E + 10), (E, E + 50), (E - 1, E), (E, E + 1), (2 * E, T), (2 * E - 1, 2 * E + hop + 1),
                  (E + hop - 1, E + hop + 1), (7, 7), (E, E), (T, T), (0, T), (0, 1), (T - 1, T), (100, 100 + 70 * hop), (2 * E + 5, T + 1000)]
        lo, hi = [a for a, _ in ranges], [b for _, b in ranges]
        rng = np.random.default_rng(Fr + hop)
        lat, (wc, bc) = _latent(rng, len(ranges), D, Fr), _weights(rng, D, nb, hop)
        got = ops.h16_head(torch.from_numpy(lat).cuda(), wc, bc, T, keep_lo=lo, keep_hi=hi).cpu().numpy()
        rlo, rhi = O16.head16_bounds(lat, wc, bc, T, keep_lo=lo, keep_hi=hi)
        n = np.array([max(0, min(b, T) - a) for a, b in ranges], np.float64)[:, None]
        err = np.maximum(np.maximum(rlo - got, got - rhi), 0)
        print(f"MEASURE head16 keep ranges D={D} hop={hop}: {float((err / np.maximum(n, 1)).max()):.2e} per kept sample")
        assert (err <= (SAMPLE_BAR + sum_slack(Fr, hop)) * np.maximum(n, 1)).all(), (err / np.maximum(n, 1)).max(axis=1)
        assert (got[n[:, 0] == 0] == 0).all()                                          # lo == hi: nothing enters the sum
        mean = ops.h16_head(torch.from_numpy(lat[11:12]).cuda(), wc, bc, T).cpu().numpy()
        np.testing.assert_allclose(got[11] / np.float32(T), mean[0], rtol=2.0 ** -21, atol=0)


@pytest.mark.parametrize("D,nb,hop", [(64, 36, 32), (64, 64, 32), (128, 36, 320), (144, 16, 320), (40, 16, 320), (64, 6, 32), (64, 16, 48)])
def test_head16_refuses_shapes_outside_its_gate(ops, D, nb, hop):
    """More than 32 bits, D > 128 or not a multiple of 16, nb % 4, hop % 32: WV_EINVAL, nothing launched."""
    lat = torch.ones(1, D, 2, device="cuda")
    wc, bc = np.ones((D, nb * hop), np.float32), np.zeros(nb, np.float32)
    with pytest.raises(RuntimeError, match="wv_h16_head"):
        ops.h16_head(lat, wc, bc, 2 * hop)
    with pytest.raises(RuntimeError, match="wv_h16_head"):
        ops.h16_head(lat, wc, bc, 2 * hop, keep_lo=[0], keep_hi=[1])


def test_head16_refuses_a_length_its_latent_does_not_have(ops):
    lat = torch.ones(1, 64, 3, device="cuda")
    wc, bc = np.ones((64, 4 * 32), np.float32), np.zeros(4, np.float32)
    for T in (64, 97):                                                                  # Fr = ceil(T / hop) must be 3
        with pytest.raises(RuntimeError, match="wv_h16_head"):
            ops.h16_head(lat, wc, bc, T)
    assert ops.h16_head(lat, wc, bc, 65).shape == (1, 4)
