"""Windowed long-form, mixed-length and live-session execution on the MI355X (waveverify_amd/window.py, session.py,
csrc/wv_window.hip) against the whole-clip forwards of the same nets."""

import numpy as np
import pytest
import torch

from oracle import wv_oracle as O
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict, synthetic_clips

pytestmark = pytest.mark.gpu

KINDS = ("generator", "detector", "locator")


def _net(kind):
    from waveverify_amd.nets import HipNet
    return HipNet(default_config(kind), random_state_dict(default_config(kind), 0))


@pytest.fixture(scope="module")
def nets():
    return {k: _net(k) for k in KINDS}


def _loc_ok(got, ref):
    """Locator logits: whole-clip forwards of different lengths already differ by up to 1e-4 (the log-magnitude STFT amplifies
    f32 summation-order differences on quiet frames; test_gpu_longform's prefix property uses that bar), so 1e-4, scaled by
    the logits' magnitude, and the decisions' MIoU."""
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    err = float(np.abs(got - ref).max())
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), err
    assert O.miou((got > 0.5).astype(int), (ref > 0.5).astype(int)) >= 0.9999


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


def test_mixed_lengths_windowed_vs_whole_clip(nets):
    from waveverify_amd import window
    lengths = [16000 * 7 + 123, 48000, 1000]
    clips, msgs = [], []
    for i, T in enumerate(lengths):
        x, m = synthetic_clips(1, T, seed=40 + i)
        clips.append(torch.from_numpy(x[0, 0]).cuda())
        msgs.append(torch.from_numpy(m).cuda())
    msg = torch.cat(msgs)
    G, D, L = nets["generator"], nets["detector"], nets["locator"]
    wm = window.windowed_generator(G, clips, msg, window=32000)
    mp = window.windowed_detector_mean_prob(D, wm, window=32000)
    lo = window.windowed_locator(L, wm, window=32000)
    wm16 = window.windowed_generator(G, clips, msg, window=32000, precision="f16")
    for b, (x, T) in enumerate(zip(clips, lengths)):
        ref = G.generator(x.view(1, 1, T), msg[b: b + 1], add_input=True)[0, 0]
        assert wm[b].shape == (T,)
        assert _err(wm[b], ref) <= 1e-6
        assert _err(wm16[b], ref) <= 1e-4
        mref = D.detector_mean_prob(ref.view(1, 1, T))[0]
        assert _err(mp[b], mref) <= 1e-6
        assert torch.equal(mp[b] >= 0.5, mref >= 0.5)
        assert torch.equal(window.windowed_detector_mean_prob(D, [wm16[b]], window=32000)[0] >= 0.5, mref >= 0.5)
        _loc_ok(lo[b], L.locator(ref.view(1, 1, T))[0, 0])


def test_beyond_the_k1_gate(nets):
    """One 200 s clip (past the ~175 s where the whole-clip generator leaves its fast path) with 30 s windows."""
    from waveverify_amd import window
    T = 3200000
    G = nets["generator"]
    need = G._lib.wv_workspace_bytes(G._h, 1, T)
    assert need < 16 * 2 ** 30, need
    x, m = synthetic_clips(1, T, seed=77)
    x, m = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    ref = G.generator(x, m, add_input=True)
    Gw, Dw, Lw = _net("generator"), _net("detector"), _net("locator")
    wm = window.windowed_generator(Gw, x, m, window=480000, max_windows=4)
    assert wm.shape == (1, 1, T)
    assert _err(wm, ref) <= 1e-6
    mp = window.windowed_detector_mean_prob(Dw, ref, window=480000, max_windows=4)[0]
    logits = nets["detector"].detector(ref)[0]
    mref = torch.sigmoid(logits.double()).mean(dim=1)
    del logits
    assert _err(mp, mref) <= 1e-6
    assert torch.equal(mp >= 0.5, mref >= 0.5)
    assert torch.equal(mp >= 0.5, nets["detector"].detector_mean_prob(ref)[0] >= 0.5)
    _loc_ok(window.windowed_locator(Lw, ref, window=480000, max_windows=4), nets["locator"].locator(ref))
    for net in (Gw, Dw, Lw):
        cap = net._lib.wv_workspace_bytes(net._h, 4, 480000)
        assert all(w.numel() <= cap for w in net._ws.values()) and not net._retired


def test_windowed_detect_is_deterministic(nets):
    from waveverify_amd import window
    x, _ = synthetic_clips(2, 16000 * 9 + 5, seed=8)
    x = torch.from_numpy(x).cuda()
    a = window.windowed_detector_mean_prob(nets["detector"], x, window=48000)
    b = window.windowed_detector_mean_prob(nets["detector"], x, window=48000)
    assert torch.equal(a, b)


SIZES = [1, 319, 320, 641, 5, 7000, 0, 3333]


def _pushes(sess, x):
    outs, seen = [], 0
    for n in SIZES:
        outs.append((seen + n, sess.push(x[:, seen: seen + n])))
        seen += n
    return outs, sess.flush()


@pytest.mark.parametrize("kind", ["generator", "locator"])
def test_embed_and_locate_sessions(nets, kind):
    from waveverify_amd.session import EmbedSession, LocateSession
    S, T = 3, sum(SIZES)
    x, m = synthetic_clips(S, T, seed=12)
    x, m = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    net = nets[kind]
    if kind == "generator":
        sess, ref = EmbedSession(net, m), net.generator(x, m, add_input=True)
    else:
        sess, ref = LocateSession(net, S), net.locator(x)
    hop = net.cfg.hop_length
    outs, last = _pushes(sess, x[:, 0])
    emitted = 0
    for seen, y in outs:
        assert y.shape == (S, 1, seen // hop * hop - emitted)
        emitted += y.shape[-1]
    got = torch.cat([y for _, y in outs] + [last], dim=-1)
    assert got.shape == ref.shape
    if kind == "generator":
        assert _err(got, ref) <= 1e-6
    else:
        _loc_ok(got, ref)


def test_detect_session(nets):
    from waveverify_amd.session import DetectSession
    S, T = 3, sum(SIZES)
    x, _ = synthetic_clips(S, T, seed=13)
    x = torch.from_numpy(x).cuda()
    D = nets["detector"]
    sess = DetectSession(D, S)
    hop = D.cfg.hop_length
    seen = 0
    for n in SIZES:
        st = sess.push(x[:, 0, seen: seen + n])
        seen += n
        mlen = seen // hop * hop
        assert st.samples_seen == mlen
        if mlen:
            assert _err(st.mean_prob, D.detector_mean_prob(x[:, :, :mlen])) <= 1e-6
    st = sess.flush()
    ref = D.detector_mean_prob(x)
    assert st.samples_seen == T
    assert _err(st.mean_prob, ref) <= 1e-6
    assert torch.equal(st.bits, (ref >= 0.5).to(torch.int32))
    sess.reset()
    assert sess.push(x[:, 0, :hop]).samples_seen == hop


def test_api_clips_and_sessions_agree_with_batches(tmp_path):
    from waveverify_amd.core import WaveVerify
    from waveverify_amd.utils import save_audio
    wv = WaveVerify.random_init(seed=0)
    lengths = [16000 * 3 + 7, 20000]
    clips = [torch.from_numpy(synthetic_clips(1, T, seed=60 + i)[0][0, 0]).cuda() for i, T in enumerate(lengths)]
    ids = [1234, 4321]
    wm = wv.embed_clips(clips, ids, window_seconds=1.0)
    for b, x in enumerate(clips):
        msg = wv._messages(ids[b])
        ref = wv.embed_batch(x.view(1, 1, -1), msg)[0, 0]
        assert _err(wm[b], ref) <= 1e-6
    bits, mp = wv.detect_clips(wm, window_seconds=1.0)
    loc = wv.locate_clips(wm, window_seconds=1.0)
    for b, y in enumerate(wm):
        rb, rmp = wv.detect_batch(y.view(1, 1, -1))
        assert torch.equal(bits[b], rb[0]) and _err(mp[b], rmp[0]) <= 1e-6
        assert _err(loc[b], wv.locate_batch(y.view(1, 1, -1))[0]) <= 1e-4
    es = wv.open_embed_session(ids)
    assert es.S == 2 and isinstance(wv.open_detect_session(2).push(torch.zeros(2, 640, device="cuda")).samples_seen, int)
    assert wv.open_locate_session(1).push(torch.zeros(1, 100, device="cuda")).shape == (1, 1, 96)      # locator hop 32
    x, _ = synthetic_clips(1, 12 * 16000, seed=61)
    path = tmp_path / "clip.wav"
    save_audio(torch.from_numpy(x[0]), path, 16000)
    a, _, _ = wv.embed(path, 777)
    b, _, _ = wv.embed(path, 777, window_seconds=5)
    assert np.abs(a - b).max() <= 1e-6
    assert wv.detect(path, window_seconds=5)[0] == wv.detect(path)[0]


def test_windowed_f16_detect_vs_the_oracle(nets):
    """The windowed f16 detect (head16_kernel's windowed mode behind every window, then one f64 reduction per clip) on mixed lengths, two
    of them windowed, against the oracle of the mode's arithmetic on the whole clip (oracle/wv_oracle_h16.detect_mean_prob), not only by
    its decisions.  Measured on the MI355X: 3.1e-6 at most; the bar is the whole-clip test's det_mean_bar(T) (tests/test_gpu_h16.py)."""
    from oracle import wv_oracle_h16 as O16
    from oracle import wv_oracle_torch as OT
    from waveverify_amd import window
    lengths = [16000, 9001, 1000]
    clips = [synthetic_clips(1, T, seed=90 + i)[0][0, 0] for i, T in enumerate(lengths)]
    mp = window.windowed_detector_mean_prob(nets["detector"], [torch.from_numpy(c).cuda() for c in clips], window=6400, precision="f16")
    cfg = default_config("detector")
    net = OT.Net(cfg, random_state_dict(cfg, 0))
    for b, c in enumerate(clips):
        ref = O16.detect_mean_prob(net, c.reshape(1, 1, -1))[0]
        err = _err(mp[b].cpu(), ref)
        print(f"MEASURE windowed f16 detect T={lengths[b]}: {err:.2e}")
        assert err <= 2e-5 + 2e-4 / lengths[b] ** 0.5, err


def test_exact_window_psum_per_sample(nets):
    """The exact path's windowed head (head_kernel's WIN mode): rows that are copies of one clip, each keeping a narrow range -- single
    samples at frame and 64-frame tile edges, ranges across them, an empty one -- sum exactly what sigmoid(detector(x)) sums over the
    same columns, to f32 order (measured 1e-7 per kept sample)."""
    D = nets["detector"]
    hop = D.cfg.hop_length
    L = 70 * hop - 11
    x = torch.from_numpy(synthetic_clips(1, L, seed=5)[0]).cuda()
    E = 64 * hop
    ranges = [(0, 1), (1, 2), (hop - 1, hop), (hop, hop + 1), (hop + 1, hop + 2), (E - 1, E), (E, E + 1), (E + 1, E + 2), (L - 1, L),
              (E - 3, E + 4), (hop - 2, hop + 3), (E, L), (0, L), (7, 7), (E, E), (32 * hop - 1, 32 * hop + 1), (63 * hop + 5, 65 * hop + 9)]
    lo, hi = [a for a, _ in ranges], [b for _, b in ranges]
    ps = D.detector_window_psum(x.expand(len(ranges), 1, L).contiguous(), lo, hi).double().cpu()
    p = torch.sigmoid(D.detector(x)[0].double()).cpu()                                # [nb, L]
    worst = 0.0
    for r, (a, b) in enumerate(ranges):
        ref = p[:, a:b].sum(dim=1)
        err = float((ps[r] - ref).abs().max())
        worst = max(worst, err / max(1, b - a))
        assert err <= 1e-6 * max(1, b - a), (a, b, err)
        if a == b:
            assert (ps[r] == 0).all()
    print(f"MEASURE exact window psum: {worst:.2e} per kept sample")
