"""CPU-only tests of the host side: WatermarkID (against the reference's own answers), bit <-> tensor
helpers, WAV I/O, metrics, checkpoint formats, parameter grammar, C-ABI exports, sharding."""
import ctypes as C
import json
import os
import re
import struct
import wave
from datetime import datetime

import numpy as np
import pytest
import torch

from oracle import wv_oracle as O
from waveverify_amd import WatermarkID
from waveverify_amd import _lib, checkpoint, metrics, parallel, params, utils
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- WatermarkID
@pytest.fixture(scope="module")
def wid_golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "watermark_ids.json")))


def test_watermark_id_known_answers(wid_golden):
    g = wid_golden
    for s, bits in g["creator"].items():
        assert WatermarkID.for_creator(s).bits == bits
    for s, (bits, kind) in g["tracking"].items():
        w = WatermarkID.for_tracking(s)
        assert (w.bits, w.metadata["id_type"]) == (bits, kind)
    for s, (bits, code, custom) in g["license"].items():
        w = WatermarkID.for_license(s)
        assert (w.bits, w.metadata["code"], w.metadata["is_custom"]) == (bits, code, custom)
    for iso, bits in g["timestamp"].items():
        assert WatermarkID.for_timestamp(datetime.fromisoformat(iso)).bits == bits
    for rep, (bits, hx, iv, by, st) in g["custom"].items():
        w = WatermarkID.custom(eval(rep))
        assert (w.bits, w.to_hex(), w.to_int(), list(w.to_bytes()), str(w)) == (bits, hx, iv, by, st)
    assert str(WatermarkID.for_creator("abc")) == g["str"]["creator"]
    assert str(WatermarkID.for_license("MIT")) == g["str"]["license"]
    assert str(WatermarkID.for_tracking("77")) == g["str"]["tracking"]
    assert WatermarkID.custom(42).bits == "0000000000101010"


def test_watermark_id_errors_and_identity():
    for bad in ["101", "10101010101010102", "", 65536, -1, b"\x01", b"\x01\x02\x03"]:
        with pytest.raises(ValueError):
            WatermarkID.custom(bad)
    for bad in [1.5, None, [1, 0]]:
        with pytest.raises(TypeError):
            WatermarkID.custom(bad)
    with pytest.raises(TypeError):
        WatermarkID(123)
    with pytest.raises(ValueError):
        WatermarkID.for_creator("")
    with pytest.raises(ValueError):
        WatermarkID.for_tracking("")
    with pytest.raises(ValueError):
        WatermarkID.for_timestamp(datetime(2023, 1, 1))
    a, b = WatermarkID.custom(7), WatermarkID.custom("0000000000000111")
    assert a == b and hash(a) == hash(b) and a != WatermarkID.custom(8) and a != "0000000000000111"
    assert len({a, b}) == 1


# ----------------------------------------------------------------------------- bits <-> tensors
def test_message_tensor_roundtrip():
    t = utils.message_to_tensor("1010101010101010")
    assert t.shape == (1, 16) and t.dtype == torch.float32
    assert utils.message_to_tensor([1, 0] * 8).tolist() == t.tolist()
    for bad in ["101", "2" * 16]:
        with pytest.raises(ValueError):
            utils.message_to_tensor(bad)
    with pytest.raises(TypeError):
        utils.message_to_tensor(42)
    probs = torch.zeros(2, 16, 50)
    probs[0, ::2] = 0.9
    probs[0, 1, :25] = 1.0                  # mean exactly 0.5 -> '1' (>= threshold)
    assert utils.tensor_to_message(probs) == "1110" + "10" * 6
    assert utils.tensor_to_message(probs.mean(2)) == utils.tensor_to_message(probs)
    with pytest.raises(ValueError):
        utils.tensor_to_message(probs, threshold=1.5)
    with pytest.raises(TypeError):
        utils.tensor_to_message(np.zeros(16))


# ----------------------------------------------------------------------------- audio files
def test_wav_io(tmp_path):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(np.clip(rng.standard_normal((1, 4000)).astype(np.float32) * 0.5, -2, 2))
    p = tmp_path / "a" / "f.wav"
    utils.save_audio(x, p, 16000)                      # float32 WAV, clamped to [-1, 1]
    y, sr = utils.load_audio(p)
    assert sr == 16000 and y.shape == (1, 4000)
    assert torch.equal(y, x.clamp(-1, 1))
    # PCM16 stereo written by the stdlib -> mono mix-down
    p16 = tmp_path / "s.wav"
    pcm = (rng.standard_normal((1000, 2)) * 3000).astype("<i2")
    with wave.open(str(p16), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    y, sr = utils.load_audio(p16)
    assert y.shape == (1, 1000)
    assert np.allclose(y.numpy()[0], pcm.astype(np.float32).mean(1) / 32768.0, atol=1e-7)
    with pytest.raises(FileNotFoundError):
        utils.load_audio(tmp_path / "missing.wav")
    with pytest.raises(ValueError):
        utils.load_audio(tmp_path)
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")
    with pytest.raises(RuntimeError, match="Cannot load audio file"):
        utils.load_audio(bad)
    with pytest.raises(ValueError):
        utils.save_audio(np.zeros(10), tmp_path / "x.wav")


# ----------------------------------------------------------------------------- metrics
def test_metrics_match_oracle():
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((4, 16, 200)).astype(np.float32) * 2
    bits = rng.integers(0, 2, (4, 16))
    mask = (rng.random((4, 1, 200)) > 0.5).astype(np.float32)
    mask[3] = 0
    ber = metrics.BER()
    assert abs(float(ber(torch.from_numpy(logits), torch.from_numpy(bits))) - O.ber(logits, bits)) < 1e-7
    assert abs(float(ber(torch.from_numpy(logits), torch.from_numpy(bits), torch.from_numpy(mask)))
               - O.ber(logits, bits, mask)) < 1e-7
    assert float(ber(torch.from_numpy(logits), torch.from_numpy(bits), torch.zeros(4, 1, 200))) == 0.0
    with pytest.raises(RuntimeError):
        ber(torch.zeros(2, 16, 5), torch.zeros(2, 8))
    p = rng.integers(0, 2, 500); g = rng.integers(0, 2, 500)
    assert abs(metrics.MIOU()(p, g) - O.miou(p, g)) < 1e-12
    assert metrics.MIOU()(np.zeros(5, int), np.zeros(5, int)) == 1.0
    with pytest.raises(RuntimeError):
        metrics.MIOU()(np.array([0, 2]), np.array([0, 1]))


# ----------------------------------------------------------------------------- checkpoints
def _torch_sd(cfg, seed, parametrized=False):
    return {k: torch.from_numpy(v) for k, v in random_state_dict(cfg, seed, parametrized).items()}


def test_checkpoint_formats(tmp_path):
    cfgs = {k: default_config(k) for k in ("generator", "detector", "locator")}
    models = {k: _torch_sd(c, 0) for k, c in cfgs.items()}
    d = tmp_path / "run"
    d.mkdir()
    torch.save({"step": 1000, "models": models, "config": {"Generator.res_scale_enc": 0.5}}, d / "latest.pth")
    torch.save({"step": 2000, "models": {"detector": models["detector"]}}, d / "best.pth")
    assert checkpoint.is_atomic_checkpoint(d)
    assert checkpoint.find_atomic_checkpoint_file(d).name == "best.pth"        # core.py:161-165
    sds, got = checkpoint.load_checkpoint(d)
    assert set(sds) == {"detector"} and got["detector"] == cfgs["detector"]
    sds, got = checkpoint.load_checkpoint(d / "latest.pth")
    assert set(sds) == set(cfgs)
    assert got["detector"] == cfgs["detector"] and got["locator"] == cfgs["locator"]
    assert got["generator"].res_scale_enc == 0.5 and got["generator"].channels_dec == 96
    assert got["generator"].n_residual_dec == 3 and got["generator"].strides == [8, 5, 4, 2]
    # legacy layout + parametrized tensors + a shrunk architecture
    small = default_config("locator", channels_enc=4, dimension=8, strides=[2, 2], n_fft_base=16, output_dim=8)
    leg = tmp_path / "legacy" / "locator"
    leg.mkdir(parents=True)
    torch.save(_torch_sd(small, 3, parametrized=True), leg / "model.pth")
    assert not checkpoint.is_atomic_checkpoint(tmp_path / "legacy")
    sds, got = checkpoint.load_checkpoint(tmp_path / "legacy")
    assert got["locator"] == small
    with pytest.raises(FileNotFoundError):
        checkpoint.load_checkpoint(tmp_path / "nope")
    with pytest.raises(NotImplementedError):
        checkpoint.apply_argbind_config("generator", cfgs["generator"], {"Generator.causal": False})


def test_checkpoint_with_full_train_py_key_set(tmp_path):
    """An atomic checkpoint carrying every key scripts/train.py:1632-1656 writes (optimizers with real
    Adam state, scheduler dicts, tracker, message_threshold, an argbind-style config dict with entries of
    other classes and None values) loads under weights_only=True; discovery follows core.py:343-356
    (first file that loads AND has a 'models' dict), and a file the safe loader refuses is reported as
    such instead of falling through to the legacy layout."""
    cfgs = {k: default_config(k) for k in ("generator", "detector", "locator")}
    models = {k: _torch_sd(c, 0) for k, c in cfgs.items()}
    models["discriminator"] = {"convs.0.weight": torch.zeros(4, 1, 3)}
    lin = torch.nn.Linear(3, 2)
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-4)
    lin(torch.ones(1, 3)).sum().backward(); opt.step()
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    full = {"step": 123, "models": models,
            "optimizers": {"generator": opt.state_dict(), "discriminator": opt.state_dict()},
            "schedulers": {"generator": sched.state_dict(), "discriminator": sched.state_dict()},
            "tracker": {"step": 123, "history": {"loss": [1.0, 0.5]}}, "message_threshold": 0.5,
            "config": {"Generator.res_scale_enc": 0.4, "Generator.sample_rate": 16000, "Generator.causal": True,
                       "Discriminator.rates": [], "AdamW.lr": 1e-4, "train.seed": None, "Detector.nbits": 16}}
    d = tmp_path / "run"; d.mkdir()
    torch.save({"not_models": 1}, d / "best.pth")              # loads, but is not an atomic checkpoint
    torch.save(full, d / "zz_step123.pth")
    assert checkpoint.is_atomic_checkpoint(d)
    assert checkpoint.find_atomic_checkpoint_file(d).name == "zz_step123.pth"
    sds, got = checkpoint.load_checkpoint(d)
    assert set(sds) == {"generator", "detector", "locator"}
    assert got["generator"].res_scale_enc == pytest.approx(0.4) and got["detector"] == cfgs["detector"]
    # a checkpoint the safe loader refuses: clear error, no legacy fallback
    import argparse
    bad = tmp_path / "bad"; bad.mkdir()
    torch.save({"models": {}, "tracker": argparse.Namespace(step=1)}, bad / "latest.pth")   # an arbitrary pickled object
    with pytest.raises(checkpoint.UnsafeCheckpointError, match="weights_only"):
        checkpoint.load_checkpoint(bad)
    with pytest.raises(NotImplementedError, match="res_scale_dec"):
        checkpoint.apply_argbind_config("generator", cfgs["generator"], {"Generator.res_scale_dec": None})


def test_infer_config_small_generator():
    cfg = default_config("generator", channels_enc=8, channels_dec=8, n_residual_dec=2, dimension=16,
                         strides=[2, 2], n_fft_base=16, zero_init=False)
    assert checkpoint.infer_config("generator", random_state_dict(cfg, 1)) == cfg


# ----------------------------------------------------------------------------- parameter grammar / C ABI
def test_param_counts_match_reference_probe():
    """9,588,507 / 4,312,541 / 132,470 parameters (zero_init=True)."""
    # detector / locator also carry the unused message MLP + FiLM tensors (seanet.py:831-846)
    assert params.param_count(default_config("generator")) == 9588507
    assert params.param_count(default_config("detector")) == 4312541
    assert params.param_count(default_config("locator")) == 132470


def test_c_abi_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert "wv_train_last_error" not in declared and not [n for n in declared if n.startswith("wv_train_half_")]   # one channel, no half exports
    for name in declared:
        assert getattr(lib, name) is not None
    assert b"gfx950" in lib.wv_version()


@pytest.mark.parametrize("kind", ["generator", "detector", "locator"])
def test_c_param_table_matches_python_grammar(kind):
    """The library's parameter table (no GPU call involved) == params.param_specs == reference keys."""
    from waveverify_amd.nets import _fill_config
    lib = _lib.load()
    for kw in ({}, {"zero_init": False}, {"strides": [2, 2], "channels_enc": 8, "n_fft_base": 16}):
        cfg = default_config(kind, **kw)
        h = C.c_void_p()
        c = _fill_config(cfg)
        _lib.check(lib.wv_model_create(C.byref(c), C.byref(h)))
        try:
            n = lib.wv_model_num_params(h)
            name, shape = C.create_string_buffer(256), (C.c_int64 * 4)()
            nd, wn = C.c_int(), C.c_int()
            table = {}
            for i in range(n):
                _lib.check(lib.wv_model_param_info(h, i, name, 256, shape, C.byref(nd), C.byref(wn)))
                table[name.value.decode()] = (tuple(shape[: nd.value]), bool(wn.value))
            want = {k: (tuple(s), role == "wn") for k, s, role in params.param_specs(cfg)}
            assert table == want
            # errors are loud and typed
            buf = (C.c_float * 4)()
            assert lib.wv_model_set_param(h, b"no.such.key", buf, 4) == -2
            assert b"unknown parameter" in lib.wv_last_error()
            assert lib.wv_model_set_param(h, b"encoder.conv_pre.1.conv.conv.bias", buf, 3) == -1
            assert lib.wv_model_finalize(h) == -2 and b"missing parameter" in lib.wv_last_error()
            assert lib.wv_workspace_bytes(h, 4, 16000) > 0
        finally:
            lib.wv_model_destroy(h)


# entry points whose all-null / all-zero call is refused before the library's first HIP call; the four training calls with the reason
# their own (former) error channel gave
_REFUSED_NULL_CALLS = ["wv_op_pw_dw", "wv_op_head", "wv_h16_head", "wv_stft_plan_create", "wv_stft_plan_logmag", "wv_specloss", "wv_metrics_iou",
                       "wv_metrics_decode", "wv_fx_median", "wv_fx_pointwise", "wv_fx_resample", "wv_aug_sequence", "wv_aug_backward",
                       "wv_window_gather", "wv_session_advance"]
_REFUSED_TRAIN_CALLS = {"wv_train_unit_create": "bad kernel size / stride", "wv_train_bce_logits": "null / bad argument",
                        "wv_train_adamw": "null / bad argument", "wv_train_film_forward": "null / bad argument (E <= 256, layers <= 4)"}


def test_c_every_refusal_states_its_own_reason():
    """One error channel: a call refused with a non-zero status leaves ITS reason in wv_last_error(), whichever source file exports it --
    never the message of an earlier, unrelated failure."""
    from waveverify_amd.nets import _fill_config
    lib = _lib.load()
    h = C.c_void_p()
    c = _fill_config(default_config("detector"))
    _lib.check(lib.wv_model_create(C.byref(c), C.byref(h)))
    try:
        for name in _REFUSED_NULL_CALLS + list(_REFUSED_TRAIN_CALLS):
            buf = (C.c_float * 4)()
            assert lib.wv_model_set_param(h, b"no.such.key", buf, 4) == -2
            assert b"unknown parameter: no.such.key" in lib.wv_last_error()
            if name == "wv_train_unit_create":
                out = C.c_void_p()
                rc = lib.wv_train_unit_create(64, 64, 17, 1, C.byref(out))
                assert not out.value
            else:
                zero = {C.c_int: 0, C.c_int64: 0, C.c_size_t: 0, C.c_float: 0.0, C.c_double: 0.0}
                rc = getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]])
            msg = lib.wv_last_error().decode()
            assert rc == -1, (name, rc)
            assert msg and "unknown parameter" not in msg, (name, msg)
            assert _REFUSED_TRAIN_CALLS.get(name, "") in msg, (name, msg)
    finally:
        lib.wv_model_destroy(h)


def test_c_config_default_matches_python():
    lib = _lib.load()
    from waveverify_amd.nets import _fill_config
    for kind, code in _lib.WV_KIND.items():
        c = _lib.WvConfig()
        _lib.check(lib.wv_config_default(code, C.byref(c)))
        p = _fill_config(default_config(kind))
        for f, _ in _lib.WvConfig._fields_:
            a, b = getattr(c, f), getattr(p, f)
            if hasattr(a, "__len__"):
                assert [round(float(v), 6) for v in a][: p.n_strides] == [round(float(v), 6) for v in b][: p.n_strides], f
            else:
                assert a == pytest.approx(b), f


def test_no_cpu_fallback():
    from waveverify_amd import WaveVerify
    from waveverify_amd.nets import HipNet
    cfg = default_config("locator")
    with pytest.raises(RuntimeError):
        HipNet(cfg, random_state_dict(cfg, 0), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="WaveVerify initialization failed"):
            WaveVerify({"locator": random_state_dict(cfg, 0)})
    with pytest.raises(RuntimeError, match="WaveVerify initialization failed"):
        WaveVerify("base")                      # empty download URL upstream: cannot succeed there either


# ----------------------------------------------------------------------------- sharding
def test_shard_bounds_cover_and_balance():
    for n in (0, 1, 7, 256, 1000):
        for world in (1, 2, 3, 8):
            spans = [parallel.shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        parallel.shard_bounds(4, 2, 2)


def test_gradient_destination_views_are_checked():
    """train._dst: kernels write parameter gradients straight into the caller's arena views -- a view of the wrong size, dtype or
    layout must be refused on the host (the kernel would otherwise write past it), a missing one falls back to a fresh tensor."""
    from waveverify_amd.train import _dst
    arena = torch.zeros(64)
    good = arena[8:8 + 12].view(3, 4, 1)
    assert _dst(dict(dv=good), "dv", (3, 4), "cpu") is good                       # same element count, any shape
    fresh = _dst(None, "dv", (3, 4), "cpu")
    assert fresh.shape == (3, 4) and fresh.dtype == torch.float32
    assert _dst(dict(other=good), "dv", (3, 4), "cpu").shape == (3, 4)            # key absent -> fresh tensor
    for bad in (arena[:11], arena[:24:2], arena[:12].double()):
        with pytest.raises(ValueError):
            _dst(dict(dv=bad), "dv", (3, 4), "cpu")


def test_stft_basis_is_the_reference_buffer(golden_dir):
    """checkpoint.stft_basis forms the `...spec.weight` buffers written into state dicts with the reference's own torch calls
    (modules/conv.py:1003-1020): bit-equal to the buffers of the reference's modules (tests/golden/dft_basis.npz)."""
    import os
    import numpy as np
    from waveverify_amd.checkpoint import stft_basis
    g = np.load(os.path.join(golden_dir, "dft_basis.npz"))
    b64 = stft_basis(64)
    assert tuple(b64.shape) == (66, 1, 64) and np.array_equal(b64[:, 0].numpy(), g["n64"])
    assert np.array_equal(stft_basis(1024)[::19, 0].numpy(), g["n1024_rows_every19"])


def test_to_parametrized_is_weight_norm_of_the_same_weights():
    """checkpoint.to_parametrized: original0 = ||w|| over all dimensions but the first, original1 = w (torch's weight_norm applied to an
    existing weight), so g v / ||v|| gives the weights back; plain tensors and already-parametrized pairs pass through."""
    import numpy as np
    import torch
    from waveverify_amd.checkpoint import to_parametrized
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    cfg = default_config("locator")
    plain = random_state_dict(cfg, 4)
    live = to_parametrized({k: torch.from_numpy(v) for k, v in plain.items()}, cfg)
    assert set(live) == set(random_state_dict(cfg, 4, parametrized=True))
    for k, w in plain.items():
        if k in live:
            assert np.array_equal(live[k].numpy(), w)
            continue
        base = k[: -len("weight")] + "parametrizations.weight.original"
        g, v = live[base + "0"], live[base + "1"]
        assert tuple(g.shape) == (w.shape[0], 1, 1) and np.array_equal(v.numpy(), w)
        back = v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1))
        assert float((back - torch.from_numpy(w)).abs().max()) <= 1e-6 * float(np.abs(w).max())
    again = to_parametrized(live, cfg)
    assert all(torch.equal(again[k], live[k]) for k in live)


def test_f16_rounding_of_the_weight_packers():
    """The f16 mode packs its weights on the host: f32 -> f16 round-to-nearest-even, bit for bit numpy's (normals, ties, subnormals,
    overflow to inf, signed zeros, inf / nan)."""
    import ctypes as C
    from waveverify_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    vals = [rng.standard_normal(20000).astype(np.float32), (rng.standard_normal(5000) * 1e-5).astype(np.float32),
            (rng.standard_normal(5000) * 3e4).astype(np.float32), (rng.standard_normal(2000) * 1e-7).astype(np.float32)]
    halves = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)          # every finite f16 ...
    ties = (halves[:-1] + halves[1:]) * np.float32(0.5)                                        # ... and every midpoint between neighbours
    special = np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, 65519.99, 65520.0, 1e9, -1e9, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 6.1e-5], np.float32)
    x = np.concatenate(vals + [halves, -halves, ties, -ties, special])
    out = np.empty(x.size, np.uint16)
    assert lib.wv_h16_round_host(x.ctypes.data, out.ctypes.data, C.c_int64(x.size)) == 0
    with np.errstate(over="ignore"):
        ref = x.astype(np.float16).view(np.uint16)
    assert np.array_equal(out, ref), np.flatnonzero(out != ref)[:10]
    nan = np.array([np.nan], np.float32)
    o = np.empty(1, np.uint16)
    assert lib.wv_h16_round_host(nan.ctypes.data, o.ctypes.data, C.c_int64(1)) == 0 and np.isnan(o.view(np.float16)[0])


def test_checkpoint_config_rebuilds_our_architecture_in_the_reference(golden_dir):
    """the reference's loader builds Generator / Detector / Locator under argbind.scope(checkpoint['config'])
    (waveverify/core.py:226-236,272-276), so the `config` a checkpoint of ours carries must spell the WHOLE architecture -- a key left out
    takes the class default (zero_init=True, channels_enc=64, ...).  tests/golden/state_dict_keys.json holds, for several configurations
    incl. zero_init=False (what conf/base.yml ships) and non-default widths, the dict this library emits and the state-dict key -> shape
    table of the reference's modules constructed from exactly that dict (make_golden_keys.py).  Here: we still emit that dict, and the
    reference's key set and shapes are ours (live weight-norm layout + the DFT buffers; a detector / locator encoder also carries the
    message MLP + FiLM tensors it never uses)."""
    import json
    import os
    from waveverify_amd.checkpoint import argbind_config, stft_basis
    from waveverify_amd.config import default_config
    from waveverify_amd.params import param_specs
    fx = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    assert len(fx) == 12
    tag = "parametrizations.weight.original"
    for name, case in fx.items():
        kind = name.split("/")[1]
        cfg = default_config(kind, **case["overrides"])
        assert argbind_config({kind: cfg}) == case["config"], name
        ours = {}
        for key, shape, role in param_specs(cfg):
            if role == "wn":
                base = key[: -len("weight")] + tag
                ours[base + "0"] = [shape[0]] + [1] * (len(shape) - 1)
                ours[base + "1"] = list(shape)
            else:
                ours[key] = list(shape)
        ref = case["keys"]
        missing = {k: v for k, v in ours.items() if ref.get(k) != v}
        assert not missing, (name, list(missing.items())[:5])
        extra = set(ref) - set(ours)
        for k in extra:
            if k.endswith(".spec.weight"):
                n_fft = ref[k][2]
                assert ref[k] == list(stft_basis(n_fft).shape), (name, k)
            else:
                assert kind != "generator" and (k.startswith("encoder.msg_embedding.") or k.startswith("encoder.film_layers.")), (name, k)
        if not cfg.zero_init:
            assert not any(k.endswith("scale_param") for k in ref), name
