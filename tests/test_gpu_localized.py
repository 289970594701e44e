"""Localized detection at the net and API level on the MI355X: WaveVerify.detect_localized_batch / detect_segments_batch / the file API,
HipNet.detector_frame_sums and its windowed form, against the float64 oracle (oracle.wv_oracle.detector_forward in float64 ->
tests/localized_cases.py's restatement of the frames kernels and the segment reduce).

Bars: 1e-5 on a masked mean probability against float64, the project's mean-probability bar (test_gpu_longform); 1e-3 between the f16
mode and the exact path with equal bits (the same file's f16 bar); windowed against whole-clip frame sums 1e-5 per gated sample.
Measured on the MI355X: exact path vs float64 6.4e-8 (gate = mask) and 3.6e-8 (gate = locator logits); f16 vs exact 1.3e-5; windowed vs
whole clip 1.6e-7 per gated sample (f32; the f16 mode's windows reproduce its whole-clip sums exactly), 6.0e-8 on a clip's probabilities."""
import numpy as np
import pytest
import torch

from localized_cases import decide, frame_sums_ref, reduce_ref
from oracle import wv_oracle as O
from waveverify_amd import metrics, ops, window
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict, synthetic_clips

pytestmark = pytest.mark.gpu

SEED = 0                                                          # chosen on the CPU: see test_gate_mask_vs_float64's margin assertion
LENGTHS = (4800, 16001)
BAR = 1e-5


@pytest.fixture(scope="module")
def wv():
    from waveverify_amd import WaveVerify
    return WaveVerify.random_init(seed=SEED)


@pytest.fixture(scope="module")
def oracle():
    """T -> (clips [3,1,T] f32, float64 detector logits [3,16,T]), computed once and shared."""
    cfg = default_config("detector")
    sd = random_state_dict(cfg, SEED)
    out = {}
    for T in LENGTHS:
        x, _ = synthetic_clips(3, T, seed=50 + SEED)
        out[T] = (x, O.detector_forward(cfg, sd, x, dtype=np.float64))
    return out


def _masks(T):
    """Clip 0: the second half on; clip 1: two islands; clip 2: nothing."""
    m = np.zeros((3, T), np.float32)
    m[0, T // 2:] = 1
    m[1, T // 8: T // 8 + T // 5] = 1
    m[1, T // 2 + 500: T // 2 + 500 + T // 5] = 1
    return m


def _whole(fsum64):
    B, _, Fr = fsum64.shape
    return reduce_ref(fsum64, [(b, 0, Fr) for b in range(B)])


@pytest.mark.parametrize("T", LENGTHS)
def test_gate_mask_vs_float64(wv, oracle, T):
    x, lg = oracle[T]
    hop, m = wv.model.detector.hop_length, _masks(T)
    rp, rc, exact = _whole(frame_sums_ref(lg, m, 0.5, hop, T))
    live = rc > 0
    assert np.abs(exact[live] - 0.5).min() > BAR                  # no oracle probability within the bar of the threshold
    bits, prob, cov = wv.detect_localized_batch(torch.from_numpy(x).cuda(), gate=torch.from_numpy(m).cuda())
    bits, prob, cov = bits.cpu().numpy(), prob.cpu().numpy(), cov.cpu().numpy()
    err = float(np.abs(prob.astype(np.float64) - exact).max())
    print(f"MEASURE localized gate=mask T={T}: {err:.2e}")
    assert err <= BAR and np.array_equal(bits, decide(rp))
    assert np.array_equal(cov, rc / T)
    assert cov[2] == 0 and (prob[2] == 0).all() and (bits[2] == 0).all()            # no watermark found


def test_locator_driven_vs_float64(wv, oracle):
    """The GPU's own locator logits are the restatement's gate, so a gate flip at the threshold cannot confound the detector's check."""
    T = LENGTHS[1]
    x, lg = oracle[T]
    xt = torch.from_numpy(x).cuda()
    loc = wv.model.locator.locator(xt)[:, 0]
    p = float(torch.sigmoid(loc.double().median()))               # a threshold that splits the samples (random weights: any p would do)
    from waveverify_amd.localize import gate_threshold
    thr = np.float32(gate_threshold(p))                           # the kernel compares in float32
    rp, rc, exact = _whole(frame_sums_ref(lg, loc.cpu().numpy(), thr, wv.model.detector.hop_length, T))
    bits, prob, cov = wv.detect_localized_batch(xt, threshold=p)
    err = float(np.abs(prob.cpu().numpy().astype(np.float64) - exact).max())
    print(f"MEASURE localized gate=locator T={T}: {err:.2e}, coverage {cov.tolist()}")
    assert 0 < rc.sum() < 3 * T
    assert err <= BAR and np.array_equal(cov.cpu().numpy(), rc / T)
    far = np.abs(exact - 0.5) > BAR
    assert np.array_equal(bits.cpu().numpy()[far], decide(rp)[far])


def test_f16_mode_vs_the_exact_path(wv, oracle):
    T = LENGTHS[1]
    xt = torch.from_numpy(oracle[T][0]).cuda()
    mask = (wv.model.locator.locator(xt)[:, 0] > 0).float()       # the exact path's locator decides in both runs
    if mask.sum() == 0 or mask.sum() == mask.numel():
        mask = torch.from_numpy(_masks(T)).cuda()
    bits, prob, cov = wv.detect_localized_batch(xt, gate=mask)
    wv.detector_precision = "f16"
    try:
        bits16, prob16, cov16 = wv.detect_localized_batch(xt, gate=mask)
    finally:
        wv.detector_precision = "f32"
    err = float((prob - prob16).abs().max())
    print(f"MEASURE localized f16 vs exact: {err:.2e}")
    assert err <= 1e-3 and torch.equal(bits, bits16) and torch.equal(cov, cov16)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_windowed_frame_sums_vs_whole_clip(wv, precision):
    D = wv.model.detector
    hop, nb = D.hop_length, D.cfg.head_bits
    L = window.halo(D.cfg) + hop                                  # the smallest legal window
    lengths = [L + 3 * hop + 7, 2 * L, 900]
    rng = np.random.default_rng(3)
    clips = [torch.from_numpy((0.1 * rng.standard_normal(T)).astype(np.float32)).cuda() for T in lengths]
    gates = [torch.from_numpy((rng.uniform(0, 1, T) > 0.4).astype(np.float32)).cuda() for T in lengths]
    got = window.windowed_detector_frame_sums(D, clips, gates, 0.5, L, precision, max_windows=3)
    bar = 1e-5
    for b, T in enumerate(lengths):
        ref = D.detector_frame_sums(clips[b].view(1, 1, T), gates[b].view(1, T), 0.5, precision)[0]
        assert got[b].shape == ref.shape == (nb + 1, -(-T // hop))
        assert torch.equal(got[b][nb], ref[nb])                   # counts: exact
        n = ref[nb].clamp_min(1.0)
        e = float(((got[b][:nb] - ref[:nb]).abs() / n).max())
        p, c = ops.frames_reduce(got[b].unsqueeze(0), [(0, 0, ref.shape[1])])
        pr, cr = ops.frames_reduce(ref.unsqueeze(0), [(0, 0, ref.shape[1])])
        ep = float((p - pr).abs().max())
        print(f"MEASURE windowed frames {precision} T={T}: {e:.2e} per gated sample, clip {ep:.2e}")
        assert e <= bar and ep <= bar and torch.equal(c, cr)
    none = window.windowed_detector_frame_sums(D, clips, None, 0.0, L, precision, max_windows=3)
    for b, T in enumerate(lengths):
        assert none[b][nb].sum().item() == T


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_fused_bits_equal_the_materialising_route(precision):
    """Small config (strides [2, 2], hop 4: outside head16's gate, so the f16 mode runs the exact frames kernel on its f32 tail): the bits
    of the fused route equal metrics.ber_per_clip on the materialised logits with the same mask."""
    from waveverify_amd.nets import HipNet
    cfg = default_config("detector", output_dim=8, channels_enc=32, dimension=16, strides=[2, 2], n_fft_base=16)
    net = HipNet(cfg, random_state_dict(cfg, 3))
    rng = np.random.default_rng(9)
    B, T = 4, 67
    x = torch.from_numpy((0.3 * rng.standard_normal((B, 1, T))).astype(np.float32)).cuda()
    mask = torch.from_numpy((rng.uniform(0, 1, (B, 1, T)) > 0.5).astype(np.float32)).cuda()
    mask[3] = 0
    logits = net.detector(x, precision=precision)
    errors, valid, avg = metrics.ber_per_clip(logits, torch.zeros(B, cfg.head_bits, device="cuda"), mask)
    fsum = net.detector_frame_sums(x, mask, 0.5, precision)
    prob, count = ops.frames_reduce(fsum, [(b, 0, fsum.shape[2]) for b in range(B)])
    assert torch.equal(count, mask[:, 0].sum(-1).double())
    live = count > 0
    assert live.tolist() == [True, True, True, False] and (prob[3] == 0).all()
    assert float((prob[live] - avg[live]).abs().max()) <= 1e-6
    assert torch.equal(prob[live] >= 0.5, avg[live] >= 0.5)
    assert torch.equal((prob[live] >= 0.5).sum(1).int(), errors[live])               # ber_per_clip's errors against all-zero bits


def test_segments_two_islands(wv, oracle):
    """Two islands 0.5 s apart: two segments with frame-exact edges, each decoded over its own island."""
    T = LENGTHS[1]
    x, lg = oracle[T]
    hop, sr = wv.model.detector.hop_length, wv.sample_rate
    gate = np.zeros((3, T), np.float32)
    islands = [(5, 15), (40, 48)]                                 # frames; 25 frames = 0.5 s apart
    for lo, hi in islands:
        gate[0, lo * hop: hi * hop] = 1
    gate[1] = 1
    segs = wv.detect_segments_batch(torch.from_numpy(x).cuda(), gate=torch.from_numpy(gate).cuda())
    assert [len(s) for s in segs] == [2, 1, 0]
    fs = frame_sums_ref(lg, gate, 0.5, hop, T)
    for s, (lo, hi) in zip(segs[0], islands):
        assert s.frames == (lo, hi) and s.start_s == lo * hop / sr and s.end_s == hi * hop / sr and s.coverage == 1.0
        rp, _, exact = reduce_ref(fs, [(0, lo, hi)])
        assert float(np.abs(s.prob.astype(np.float64) - exact[0]).max()) <= BAR
        far = np.abs(exact[0] - 0.5) > BAR
        assert np.array_equal(np.array([int(c) for c in s.watermark.to_bits()])[far], decide(rp[0])[far])
        assert s.confidence == pytest.approx(float(s.prob.mean()))
    whole = segs[1][0]
    assert whole.frames == (0, -(-T // hop)) and whole.start_s == 0 and whole.end_s == T / sr and whole.coverage == 1.0


def test_file_api(wv, tmp_path):
    from waveverify_amd.utils import load_audio, save_audio
    x, _ = synthetic_clips(1, 16000, seed=8)
    path = tmp_path / "clip.wav"
    save_audio(torch.from_numpy(x[0]), path, wv.sample_rate)
    audio, _ = load_audio(path, wv.sample_rate)
    _, mp = wv.detect_batch(audio.unsqueeze(0))
    wid, conf = wv.detect(path)                                   # unchanged: the whole-clip mean
    assert conf == mp.mean().item() and wid.to_bits() == "".join(str(int(v)) for v in (mp[0] >= 0.5).tolist())
    lwid, lconf = wv.detect(path, localized=True)
    _, lp, cov = wv.detect_localized_batch(audio.unsqueeze(0))
    assert lconf == lp.mean().item() and 0.0 <= float(cov[0]) <= 1.0
    assert wv.detect(path, localized=True, window_seconds=0.5)[0] is not None
    assert isinstance(wv.verify(path, lwid, localized=True), bool) and wv.verify(path, lwid, localized=True)
    for segs in (wv.segments(path), wv.segments(path, window_seconds=0.5)):
        assert isinstance(segs, list)
        for s in segs:
            assert 0.0 <= s.start_s < s.end_s <= 1.0 and 0.0 < s.coverage <= 1.0
    with pytest.raises(RuntimeError, match="Failed to detect watermark segments"):
        wv.segments(tmp_path / "missing.wav")
