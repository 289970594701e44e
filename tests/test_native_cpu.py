"""Host side of the native-rate embed route (waveverify_amd/native.py, utils.load_audio_native, the new parameters of WaveVerify.embed and
window.windowed_generator): everything that can be held without a GPU.  The kernels are held in tests/test_gpu_native.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import native_cases as NC
from waveverify_amd import _lib, effects, native, window
from waveverify_amd.core import WaveVerify
from waveverify_amd.utils import load_audio_native, save_audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wv_native_downmix_resample", "wv_native_upsample_add")


def test_exports_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "waveverify_hip.h")).read()
    declared = set(re.findall(r"\b(wv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in EXPORTS:
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES[name][0] and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES[EXPORTS[0]][1]) == 12 and len(_lib.SIGNATURES[EXPORTS[1]][1]) == 14


def test_null_calls_are_refused_with_their_own_reason():
    """All-null, all-zero calls never reach a launch: WV_EINVAL and a message naming the call."""
    lib = _lib.load()
    import ctypes as C
    zero = {C.c_int: 0, C.c_float: 0.0}
    for name in EXPORTS:
        assert getattr(lib, name)(*[zero.get(t) for t in _lib.SIGNATURES[name][1]]) == -1
        assert name in lib.wv_last_error().decode()


@pytest.mark.parametrize("sr", NC.RATES)
def test_transposed_tables(sr):
    for of, nf in ((sr, NC.MODEL_RATE), (NC.MODEL_RATE, sr)):
        kt, orig, nw, L, width = native.transposed_table(of, nf)
        assert kt.dtype == np.float32 and kt.flags["C_CONTIGUOUS"] and kt.shape == (L, nw)
        assert (orig, nw, L, width) == native.table_geometry(of, nf) == NC.geometry(of, nf)
        if sr == NC.MODEL_RATE:
            assert (orig, nw, L, width) == (1, 1, 1, 0) and kt.tolist() == [[1.0]]         # the identity table, not a sinc
        else:
            k, w, o, n = effects.resample_kernels(of, nf)
            assert (o, n, k.shape[1], w) == (orig, nw, L, width) and L == 2 * width + orig
            assert np.array_equal(kt.view(np.int32), np.ascontiguousarray(k.T).view(np.int32))


@pytest.mark.parametrize("sr,Tn", NC.cases())
def test_upsampled_length_covers_the_clip_within_the_kernels_maximum(sr, Tn):
    T16 = NC.t16(Tn, sr)
    assert T16 >= 1
    orig, nw, _, _ = NC.geometry(sr, NC.MODEL_RATE)
    assert T16 <= NC.resample_t_max(Tn, orig, nw)                       # the front end's output length is inside its stated maximum
    up = native.upsampled_length(T16, sr)
    orig, nw, _, _ = NC.geometry(NC.MODEL_RATE, sr)
    assert up >= Tn                                                     # the up-sampled residual reaches the clip's end ...
    assert Tn <= up <= NC.resample_t_max(T16, orig, nw)                 # ... and Tn is inside the back end's stated maximum


def test_every_case_fits_the_lds_window():
    """((nw + 254) / nw) * orig + L floats of a 256-output tile against the 64 KB a workgroup may ask for."""
    for sr in NC.RATES + [96000, 192000, 11025, 24000]:
        for of, nf in ((sr, NC.MODEL_RATE), (NC.MODEL_RATE, sr)):
            orig, nw, L, _ = native.table_geometry(of, nf)
            assert ((nw + 254) // nw * orig + L) * 4 <= 64 * 1024, (of, nf)


def test_table_size_refusal_names_the_rate():
    """44101 Hz shares no factor with 16000: 16000 x 44135 taps one way (2.8 GB).  Sizes only: no such table is built."""
    orig, nw, L, _ = native.table_geometry(44101, 16000)
    assert (orig, nw) == (44101, 16000) and nw * L > native.MAX_TABLE_FLOATS == 4 * 1024 * 1024
    with pytest.raises(ValueError, match="44101"):
        native.check_rate(44101)
    for sr in NC.RATES + [96000, 192000, 11025]:
        native.check_rate(sr)                                           # 44100 among them: 160 x 475 and 441 x 174 taps


def test_cpu_tensors_are_refused_not_served_by_a_fallback():
    x = torch.zeros(1, 2, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.downmix_resample(x, 48000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.upsample_add(x, torch.zeros(1, 1, 34), 48000)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_load_audio_native_reads_back_what_save_audio_wrote(C, tmp_path):
    x = torch.from_numpy(np.random.default_rng(C).uniform(-0.5, 0.5, (C, 1234)).astype(np.float32))
    path = tmp_path / f"c{C}.wav"
    save_audio(x, path, 44100)
    got, sr = load_audio_native(path)
    assert sr == 44100 and got.dtype == torch.float32 and tuple(got.shape) == (C, 1234)
    assert torch.equal(got, x)
    with pytest.raises(FileNotFoundError):
        load_audio_native(tmp_path / "missing.wav")
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFF\0\0\0\0WAVE")
    with pytest.raises(RuntimeError, match="Cannot load audio file"):
        load_audio_native(bad)


def test_embed_signature():
    p = inspect.signature(WaveVerify.embed).parameters
    assert p["native"].default is False and p["native"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["strength"].default == 1.0 and p["strength"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["window_seconds"].default is None
    assert list(p)[:4] == ["self", "audio_path", "watermark_id", "output_path"]            # the reference's positional arguments
    q = inspect.signature(WaveVerify.embed_native_batch).parameters
    assert list(q) == ["self", "audio", "sample_rate", "message", "strength", "window_seconds"]
    assert q["strength"].default == 1.0 and q["window_seconds"].default is None
    assert list(inspect.signature(WaveVerify.to_model_rate).parameters) == ["self", "audio", "sample_rate"]


def test_strength_without_native_is_a_value_error():
    wv = WaveVerify.__new__(WaveVerify)                                 # no nets needed: refused before anything is loaded
    with pytest.raises(ValueError, match="native"):
        wv.embed("nowhere.wav", 1, strength=0.5)


def test_windowed_generator_add_input_defaults_to_true():
    p = inspect.signature(window.windowed_generator).parameters
    assert p["add_input"].default is True
