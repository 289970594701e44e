"""The localized heads on their own: head_frames_kernel (wv_op_head_frames) and head16_frames_kernel (wv_h16_head_frames) against the
float64 restatement of tests/localized_cases.py, wv_frames_reduce against a float64 sum, and all four forward entry points on guard
bands, poisoned workspaces and at offset 1.

Bars.  Exact kernel: every frame's sum within 2e-6 x (gated samples of the frame) of float64 -- the project's per-probability bar for
the head (test_gpu_ops.test_head) -- so a frame without gated samples is exactly 0; the count row exact.  f16 kernel: the reference is
the interval head16_bounds forms (O16.head16_probs over inv_ulps -2 .. +2, per frame), and the error outside it at most
(SAMPLE_BAR + sum_slack(1, hop)) x gated samples, the bars of test_gpu_h16_head.  No frame is excluded.
Measured on the MI355X (max over every case and gate below, per gated sample): exact 1.4e-7; f16 1.4e-6 outside the interval (hop 320,
a frame whose samples are all equal, as test_gpu_h16_head records for head16_kernel), 2.8e-7 elsewhere; wv_frames_reduce 0.50 ulp."""
import numpy as np
import pytest
import torch

from guard import Guards, PoisonedWorkspace
from localized_cases import frame_sums_from_probs, frame_sums_ref, reduce_ref
from oracle import wv_oracle as O
from oracle import wv_oracle_h16 as O16
from test_gpu_h16_head import SAMPLE_BAR, _latent, _weights, sum_slack
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict

pytestmark = pytest.mark.gpu

EXACT_BAR = 2e-6
THR = 0.25                                                        # exactly representable: a gate value can EQUAL it

# (B, D, Fr, nb, hop, T kind): Fr on both sides of head16's 64-frame tile and of the exact head's 64-row tile (launch_head: Tile<64, 64>),
# hop below / at / above the exact head's 64-column tile, D and nb at both ends of head16's gate
CASES = [(1, 16, 1, 4, 32, "full"), (3, 128, 2, 16, 320, "ragged"), (1, 128, 63, 4, 64, "one"), (3, 16, 64, 32, 32, "full"),
         (1, 16, 65, 16, 320, "ragged"), (1, 128, 129, 4, 32, "one"), (3, 16, 129, 4, 64, "ragged"), (1, 128, 64, 32, 320, "full"),
         (3, 16, 1, 4, 320, "ragged")]


def _T(Fr, hop, kind):
    return {"full": Fr * hop, "one": (Fr - 1) * hop + 1, "ragged": (Fr - 1) * hop + 1 + (3 * hop) // 7}[kind]


def _gates(rng, B, T, hop):
    """name -> gate [B, T] f32 or None; gated iff gate > THR."""
    off, on = np.float32(THR - 1), np.float32(THR + 1)
    t = np.arange(T)
    one = np.full((B, T), off)
    one[B - 1, (2 * T) // 3] = on
    mid = min(T - 1, (T // 2 // hop) * hop + hop // 2)
    edge = max(1, T // 2 // hop) * hop
    equal = np.full((B, T), np.float32(THR))                      # == gate_thr: off
    equal[:, ::3] = np.nextafter(np.float32(THR), np.float32(1))  # one ulp above: on
    equal[:, 1::3] = np.nextafter(np.float32(THR), np.float32(0))
    return {"null": None, "all off": np.full((B, T), off), "all on": np.full((B, T), on), "one sample": one,
            "edge in mid-frame": np.where(t >= mid, on, off)[None].repeat(B, 0).astype(np.float32),
            "edge on a frame boundary": np.where(t < edge, on, off)[None].repeat(B, 0).astype(np.float32),
            "a value equal to gate_thr": equal, "random": rng.uniform(THR - 0.5, THR + 0.5, (B, T)).astype(np.float32)}


@pytest.fixture(scope="module")
def ops():
    from waveverify_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _head_sd(rng, D, O_, nb, hop):
    r = lambda *s, scale=1.0: (scale * rng.standard_normal(s)).astype(np.float32)
    return {"reverse_convolution.weight": r(D, O_, hop, scale=D ** -0.5), "reverse_convolution.bias": r(O_, scale=0.1),
            "last_layer.weight": r(nb, O_, 1, scale=O_ ** -0.5), "last_layer.bias": r(nb)}


def _sd_args(sd):
    return (sd["reverse_convolution.weight"], sd["reverse_convolution.bias"], sd["last_layer.weight"], sd["last_layer.bias"])


@pytest.mark.parametrize("B,D,Fr,nb,hop,kind", CASES)
def test_exact_frames_vs_float64(ops, B, D, Fr, nb, hop, kind):
    T = _T(Fr, hop, kind)
    rng = np.random.default_rng(B + D + Fr + nb + hop)
    Z, sd = _latent(rng, B, D, Fr), _head_sd(rng, D, 8, nb, hop)
    p64 = 1.0 / (1.0 + np.exp(-np.clip(O.head_forward(O._Net(None, sd, np.float64), Z, T), -700, 700)))
    Zc, worst = _cu(Z), 0.0
    for name, g in _gates(rng, B, T, hop).items():
        ref = frame_sums_from_probs(p64, g, THR, hop, T)
        got_t = ops.head_frames(Zc, *_sd_args(sd), T, _cu(g), THR)
        got = got_t.cpu().numpy().astype(np.float64)
        n = ref[:, nb]
        assert np.array_equal(got[:, nb], n), name                                      # the count row, exactly
        err = np.abs(got[:, :nb] - ref[:, :nb])
        worst = max(worst, float((err / np.maximum(n, 1)[:, None]).max()))
        assert (err <= EXACT_BAR * n[:, None]).all(), (name, float((err / np.maximum(n, 1)[:, None]).max()))
        assert torch.equal(got_t, ops.head_frames(Zc, *_sd_args(sd), T, _cu(g), THR)), name          # two runs, bit for bit
        if name == "null":
            _, mean = ops.head(Zc, *_sd_args(sd), T, want_logits=False)
            assert np.abs(got[:, :nb].sum(-1) / T - mean.cpu().numpy()).max() <= 2e-6
        if name == "random" and Fr > 2:             # sensitivity: the gate one sample late breaks the bar (Fr <= 2: the roll wraps inside the all-zero frame)
            bad = frame_sums_from_probs(p64, np.roll(g, 1, axis=1), THR, hop, T)
            assert not (np.abs(got[:, :nb] - bad[:, :nb]) <= EXACT_BAR * bad[:, nb][:, None]).all()
    print(f"MEASURE head_frames B={B} D={D} Fr={Fr} nb={nb} hop={hop} T={T}: {worst:.2e} per gated sample")


@pytest.mark.parametrize("B,D,Fr,nb,hop,kind", CASES)
def test_f16_frames_vs_its_own_arithmetic(ops, B, D, Fr, nb, hop, kind):
    T = _T(Fr, hop, kind)
    rng = np.random.default_rng(7 * B + D + Fr + nb + hop)
    lat, (wc, bc) = _latent(rng, B, D, Fr), _weights(rng, D, nb, hop)
    ps = [O16.head16_probs(lat, wc, bc, inv_ulps=u) for u in range(-2, 3)]
    latc, worst = _cu(lat), 0.0
    bar = SAMPLE_BAR + sum_slack(1, hop)
    for name, g in _gates(rng, B, T, hop).items():
        refs = np.stack([frame_sums_from_probs(p, g, THR, hop, T) for p in ps])
        lo, hi, n = refs.min(0)[:, :nb], refs.max(0)[:, :nb], refs[0][:, nb]
        got_t = ops.h16_head_frames(latc, wc, bc, T, _cu(g), THR)
        got = got_t.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.array_equal(got[:, nb], n), name
        err = np.maximum(np.maximum(lo - got[:, :nb], got[:, :nb] - hi), 0)
        worst = max(worst, float((err / np.maximum(n, 1)[:, None]).max()))
        assert (err <= bar * n[:, None]).all(), (name, float((err / np.maximum(n, 1)[:, None]).max()))
        assert torch.equal(got_t, ops.h16_head_frames(latc, wc, bc, T, _cu(g), THR)), name
        if name == "random" and Fr > 2:
            bad = np.stack([frame_sums_from_probs(p, np.roll(g, 1, axis=1), THR, hop, T) for p in ps])
            blo, bhi, bn = bad.min(0)[:, :nb], bad.max(0)[:, :nb], bad[0][:, nb]
            assert not (np.maximum(np.maximum(blo - got[:, :nb], got[:, :nb] - bhi), 0) <= bar * bn[:, None]).all()
    print(f"MEASURE head16_frames B={B} D={D} Fr={Fr} nb={nb} hop={hop} T={T}: {worst:.2e} per gated sample outside the interval")


@pytest.mark.parametrize("D,nb,hop", [(64, 36, 32), (144, 16, 320), (40, 16, 320), (64, 6, 32), (64, 16, 48), (64, 4, 2048)])
def test_f16_frames_refuses_shapes_outside_its_gate(ops, D, nb, hop):
    """head16's gate (and the frames kernel's own hop <= 2016): refused with a reason, nothing launched, and the next good call runs."""
    lat = torch.ones(1, D, 2, device="cuda")
    with pytest.raises(RuntimeError, match="wv_h16_head_frames.*head limits"):
        ops.h16_head_frames(lat, np.ones((D, nb * hop), np.float32), np.zeros(nb, np.float32), 2 * hop)
    with pytest.raises(RuntimeError, match="Fr is not ceil"):
        ops.h16_head_frames(torch.ones(1, 64, 3, device="cuda"), np.ones((64, 4 * 32), np.float32), np.zeros(4, np.float32), 64)
    with pytest.raises(RuntimeError, match="Fr is not ceil"):
        ops.head_frames(torch.ones(1, 8, 3, device="cuda"), np.ones((8, 4, 32), np.float32), np.zeros(4, np.float32), np.ones((2, 4, 1), np.float32),
                        np.zeros(2, np.float32), 97)
    ok = ops.h16_head_frames(torch.ones(1, 64, 3, device="cuda"), np.ones((64, 4 * 32), np.float32), np.zeros(4, np.float32), 65)
    torch.cuda.synchronize()
    assert ok.shape == (1, 5, 3) and ok[0, 4].tolist() == [32.0, 32.0, 1.0]


def test_frames_reduce_vs_float64(ops):
    """Whole-clip, empty, single-frame and overlapping segments, one of ungated frames only: prob within 1 f32 ulp of the float64
    quotient, count exact, prob = 0 where nothing is gated."""
    rng = np.random.default_rng(5)
    B, nb, Fr, hop = 3, 16, 257, 320
    n = rng.integers(0, hop + 1, (B, Fr)).astype(np.float64)
    n[1] = 0                                                       # a clip without a gated sample
    n[2, 100:140] = 0
    fsum = np.zeros((B, nb + 1, Fr), np.float32)
    fsum[:, :nb] = (rng.uniform(0, 1, (B, nb, Fr)) * n[:, None, :]).astype(np.float32)
    fsum[:, nb] = n
    segs = [(b, 0, Fr) for b in range(B)] + [(0, 7, 7), (0, 9, 10), (2, 0, 1), (2, Fr - 1, Fr), (0, 10, 200), (0, 150, 257), (2, 100, 140), (2, 99, 141)]
    prob, count = ops.frames_reduce(_cu(fsum), segs)
    rp, rc, exact = reduce_ref(fsum, segs)
    prob, count = prob.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(count, rc)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    err = np.abs(prob.astype(np.float64) - exact)
    print(f"MEASURE frames_reduce: {float((err / ulp).max()):.2f} ulp")
    assert (err <= ulp).all() and np.array_equal(prob, rp)
    assert (prob[rc == 0] == 0).all() and (rc == 0).sum() == 3


# ---- guard bands, poisoned workspaces, offset 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_unit_entry_points_on_guarded_arenas(ops, offset):
    """wv_op_head_frames and wv_h16_head_frames with the latent, the gate and fsum between guard bands (offset 1: one float past a
    256-byte boundary): no store outside fsum, every element of fsum written, inputs unchanged, the result that of plain buffers."""
    B, D, Fr, nb, hop = 2, 16, 66, 4, 64
    T = (Fr - 1) * hop + 9
    rng = np.random.default_rng(offset)
    lat, (wc, bc), sd = _latent(rng, B, D, Fr), _weights(rng, D, nb, hop), _head_sd(rng, D, 8, nb, hop)
    gate = rng.uniform(THR - 0.5, THR + 0.5, (B, T)).astype(np.float32)
    for use_gate in (True, False):
        g = Guards(offset=offset)
        x, ga, out = g.input(lat, "latent"), g.input(gate, "gate"), g.output((B, nb + 1, Fr), name="fsum")
        gt = ga.t if use_gate else None
        ops.head_frames(x.t, *_sd_args(sd), T, gt, THR, out=out.t)
        g.check()
        assert torch.equal(out.t, ops.head_frames(_cu(lat), *_sd_args(sd), T, _cu(gate) if use_gate else None, THR))
        out.refill_pattern()
        ops.h16_head_frames(x.t, wc, bc, T, gt, THR, out=out.t)
        g.check()
        assert torch.equal(out.t, ops.h16_head_frames(_cu(lat), wc, bc, T, _cu(gate) if use_gate else None, THR))


@pytest.fixture(scope="module")
def detector():
    from waveverify_amd.nets import HipNet
    cfg = default_config("detector")
    return HipNet(cfg, random_state_dict(cfg, 0))


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("offset", [0, 1])
def test_net_entry_points_on_guarded_arenas_and_poisoned_workspaces(detector, monkeypatch, precision, offset):
    """wv_detector_forward_frames[_f16]: x, gate and fsum between guard bands, the workspace an exact-size 0xFF arena between guards;
    a second run on the re-poisoned workspace is bit-identical and equals the run on plain buffers."""
    from waveverify_amd import _lib
    made = []

    def scratch(nbytes, device):
        made.append(PoisonedWorkspace(int(nbytes), device, name=f"workspace ({int(nbytes)} bytes)"))
        return made[-1].t

    B, hop, nb = 2, detector.hop_length, detector.cfg.head_bits
    T = 2 * hop + 5
    rng = np.random.default_rng(11 + offset)
    xs = (0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)
    gate = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    plain = detector.detector_frame_sums(_cu(xs), _cu(gate), 0.0, precision)
    monkeypatch.setattr(_lib, "scratch", scratch)
    monkeypatch.setattr(detector, "_ws", {})
    g = Guards(offset=offset)
    x, ga, out = g.input(xs, "x"), g.input(gate, "gate"), g.output((B, nb + 1, 3), name="fsum")
    detector.detector_frame_sums(x.t, ga.t, 0.0, precision, out=out.t)
    g.check()
    assert made, "no workspace went through waveverify_amd._lib.scratch"
    first = out.t.clone()
    for a in made:
        a.check()
        a.repoison()
    out.refill_pattern()
    detector.detector_frame_sums(x.t, ga.t, 0.0, precision, out=out.t)
    g.check()
    for a in made:
        a.check()
    assert torch.equal(out.t, first) and torch.equal(first, plain)
    assert np.array_equal(first[:, nb].cpu().numpy(), frame_sums_ref(np.zeros((B, 1, T)), gate, 0.0, hop, T)[:, 1])
