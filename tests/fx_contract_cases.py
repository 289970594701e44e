"""The cases of tests/test_gpu_fx_contract.py (a plain module, like specloss_cases.py), shared with tests/test_oracle_fx_dense.py, which
checks on the CPU that the float64 oracle and the project's filter bar are fair for exactly these inputs."""
from __future__ import annotations

import math

import numpy as np

BAR = 2e-5                      # the project's filter bar (tests/test_gpu_effects.py)
ROWS = 3

# ---- wv_fx_fir_bank: the whole published contract ------------------------------------------------------------------------------------
FIR_L = [1, 5, 321, 1024, 1025, 2049, 2500]          # one, two and three 1024-tap LDS pieces, and a ragged last piece
FIR_NF = [1, 2, 3, 8]
FIR_STRIDE = [1, 2, 3, 4]
FIR_PADS = ["none", "half", "full", "left7", "right13"]
FIR_TOUT = [1, 255, 256, 257, 600]                   # the 256-output tile's edge and the last partial workgroup


def fir_pads(kind: str, L: int):
    return {"none": (0, 0), "half": (L // 2, L // 2), "full": (L - 1, L - 1), "left7": (7, 0), "right13": (0, 13)}[kind]


def _fir_case(L, nf, stride, replicate, pads, interleave, tout, extra=0):
    """-> (L, nf, stride, replicate, pads, interleave, T) with T such that Tout = (T + pad_l + pad_r - L) // stride + 1 == tout
    (`extra` < stride more samples leave Tout alone), or None when no T >= 1 gives it."""
    pl, pr = fir_pads(pads, L)
    T = (tout - 1) * stride + L - pl - pr + extra % stride
    return None if T < 1 else (L, nf, stride, replicate, pads, interleave, T)


FIR_CORNERS = [
    _fir_case(2500, 3, 4, 0, "half", 1, 257),        # three pieces, interleaved, stride 4
    _fir_case(2049, 8, 1, 1, "half", 0, 256),        # eight filters over three pieces
    _fir_case(1, 2, 3, 0, "left7", 0, 600),          # L = 1 with stride 3
    _fir_case(321, 2, 1, 1, "full", 0, 600),         # T = 280 < pad_l = 320: the first windows are copies of x[0] but for one sample
    _fir_case(321, 1, 2, 0, "full", 1, 255),         # T = 189 < pad_l = 320, zero padding: every window is mostly pad
]


def fir_cases(n: int = 60, seed: int = 2025):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = _fir_case(int(rng.choice(FIR_L)), int(rng.choice(FIR_NF)), int(rng.choice(FIR_STRIDE)), int(rng.integers(0, 2)),
                      str(rng.choice(FIR_PADS)), int(rng.integers(0, 2)), int(rng.choice(FIR_TOUT)), int(rng.integers(0, 4)))
        if c is not None and c not in out:
            out.append(c)
    return out + [c for c in FIR_CORNERS if c not in out]


def fir_tout(case) -> int:
    L, nf, stride, replicate, pads, interleave, T = case
    pl, pr = fir_pads(pads, L)
    return (T + pl + pr - L) // stride + 1


def fir_inputs(case):
    """-> (x [ROWS, T] float32 Gaussian, taps [nf, L] float32 with unit L1 norm per filter), seeded by the case."""
    L, nf, stride, replicate, pads, interleave, T = case
    rng = np.random.default_rng([L, nf, stride, replicate, FIR_PADS.index(pads), interleave, T])
    x = rng.standard_normal((ROWS, T)).astype(np.float32)
    taps = rng.standard_normal((nf, L))
    return x, (taps / np.abs(taps).sum(1, keepdims=True)).astype(np.float32)


def fir_id(case) -> str:
    L, nf, stride, replicate, pads, interleave, T = case
    return f"L{L}-f{nf}-s{stride}-{'rep' if replicate else 'zero'}-{pads}-{'il' if interleave else 'pl'}-T{T}"


# ---- wv_fx_resample / wv_fx_resample_adjoint --------------------------------------------------------------------------------------------
RESAMPLE_RATES = [(16000, 8000), (8000, 16000), (16000, 12000), (44100, 16000), (16000, 22050), (16000, 32000)]
POLYPHASE_RATES = [(16000, 12000), (8000, 16000), (16000, 8000)]          # at most 8 phases: what the FIR bank can hold as filters
POLYPHASE_T = [1001, 37]


def resample_geometry(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(orig, new, width) of effects.resample_kernels, from the published formula."""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    return orig, new, math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))


def resample_lengths(orig: int, width: int):
    """T shorter than the filter, T = 1, orig > T, the two sides of one phase group of inputs, and the 256-thread block's edge."""
    return sorted({T for T in (1, 2, width, orig - 1, orig + 1, 255, 256, 257, 1001) if T >= 1})


def resample_cases():
    out = []
    for of, nf in RESAMPLE_RATES:
        orig, new, width = resample_geometry(of, nf)
        out += [(of, nf, T) for T in resample_lengths(orig, width)]
    return out


def resample_t_outs(T: int, orig: int, new: int):
    """The product's ceil(new T / orig); one less (stops inside a phase group, where it exists); wv_fx_resample's stated maximum."""
    t = int(math.ceil(new * T / orig))
    return [t] + ([t - 1] if t > 1 else []) + [resample_t_max(T, orig, new)]


def resample_t_max(T: int, orig: int, new: int) -> int:
    return (-(-T // orig) + 1) * new


def resample_inputs(of: int, nf: int, T: int, t_out: int):
    rng = np.random.default_rng([of, nf, T, t_out])
    return rng.standard_normal((ROWS, T)).astype(np.float32), rng.standard_normal((ROWS, t_out)).astype(np.float32)


# ---- wv_fx_fold_replicate -------------------------------------------------------------------------------------------------------------
FOLD_T = [1, 2, 3, 1001]
FOLD_PADS = [(0, 0), (1, 0), (0, 1), (160, 160), (300, 7), (1000, 1000)]

# ---- band-pass and resample adjoints through effects.apply_effect_backward ----------------------------------------------------------------
EFFECT_SETTINGS = [("bandpass_filter", {"cutoff_freq_low": 300, "cutoff_freq_high": 3500}),
                   ("bandpass_filter", {"cutoff_freq_low": 300, "cutoff_freq_high": 4000}),
                   ("resample", {"new_sample_rate": 8000}), ("resample", {"new_sample_rate": 12000}),
                   ("resample", {"new_sample_rate": 22050}), ("resample", {"new_sample_rate": 32000})]
EFFECT_T = [1001, 37]
