"""The spectral-loss test cases shared by tests/test_oracle_specloss.py (CPU: every case is well-conditioned) and
tests/test_gpu_spectral_loss.py / tests/test_gpu_guard.py (GPU: the kernels against the float64 oracle).  A plain module.

Inputs.  x is noise of standard deviation 0.1; wm = gain * x + noise of 0.01, the gain 2 on one half of every clip and 1/2 on the other
(swapped on odd clips).  The gradient of an L1 term jumps where the two spectra are equal, and a float32 transform may land an element
that close to the jump on its other side; with a gain away from 1 almost no element is near it, and
oracle.wv_oracle_specloss.unsafe_elements counts those that are.  test_oracle_specloss.py asserts the count is 0 for every case here, so
a case measures arithmetic and not coin flips at ties.  Seeds are fixed in the tables; one that fails that check is replaced here."""
import math

import numpy as np

SR = 16000
MEL_N, MEL_W = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]
MEL_DEFAULT, MEL_POW2_MAG = (1.0, 0.0, 1.0, 1e-5), (1.0, 0.5, 2.0, 1e-5)
STFT_MAG = (0.0, 1.0, 2.0, 1e-5)
STFT_LOG_REF = (1.0, 0.0, 2.0, 1e-5)                  # the reference's clamp: the 1 / |X| part that keeps the 2e-3 bar
GRAD_BAR, GRAD_BAR_LOG_REF, TERM_BAR, FLOOR_BAR = 1e-4, 2e-3, 1e-5, 1e-5


def raised_clamp(w):
    """A twentieth of the typical |X| of noise of std 0.1 under a Hann window of length w (sum of hann^2 = 0.375 w)."""
    return 0.05 * 0.1 * math.sqrt(0.375 * w)


def stft_log(w):
    return (1.0, 0.0, 2.0, raised_clamp(w))


def clips(B, T, seed):
    """-> (wm, x) float32 [B, 1, T]."""
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((B, 1, T))
    gain = np.where(np.arange(T) < T // 2, 2.0, 0.5)
    gains = np.stack([gain if b % 2 == 0 else gain[::-1] for b in range(B)])[:, None, :]
    wm = gains * x + 0.01 * rng.standard_normal((B, 1, T))
    return wm.astype(np.float32), x.astype(np.float32)


def stft_scale(w, term):
    return {"w": w, "stft": term, "mel": None}


def mel_scale(w, n, term=MEL_DEFAULT, fmin=0.0, fmax=None):
    return {"w": w, "stft": None, "mel": term, "n_mels": n, "fmin": fmin, "fmax": fmax, "sr": SR}


# seeds replaced because the first draw had an element within the margin of a gradient jump (test_oracle_specloss.py's check)
REPLACED_SEEDS = {"stft-mag-w32-T4800": 14932, "stft-mag-w512-T4800": 15412, "stft-log-raised-w512-T4800": 15512, "mel-w512-n80-T4800": 15712,
                  "w512-n2-p1-B3-T511": 11046}


# ------------------------------------------------------------------------------------------------ per-scale, per-part cases (B = 3)
# (id, part, scale dict, T, seed, gradient bar)
def _part_cases():
    out = []
    for w in (32, 128, 512, 2048):
        for T in (4800, 1100) if w <= 512 else (4800,):
            out.append((f"stft-mag-w{w}-T{T}", "stft", stft_scale(w, STFT_MAG), T, 100 + w + T, GRAD_BAR))
            out.append((f"stft-log-raised-w{w}-T{T}", "stft", stft_scale(w, stft_log(w)), T, 200 + w + T, GRAD_BAR))
            out.append((f"stft-log-ref-w{w}-T{T}", "stft", stft_scale(w, STFT_LOG_REF), T, 300 + w + T, GRAD_BAR_LOG_REF))
    for n, w in zip(MEL_N, MEL_W):
        for T in (4800, 1100) if w <= 512 else (4800,):
            out.append((f"mel-w{w}-n{n}-T{T}", "mel", mel_scale(w, n), T, 400 + w + T, GRAD_BAR))
    out.append(("mel-pow2-mag-w128-n20-T1100", "mel", mel_scale(128, 20, MEL_POW2_MAG), 1100, 500, GRAD_BAR))
    return [(cid, part, scale, T, REPLACED_SEEDS.get(cid, seed), bar) for cid, part, scale, T, seed, bar in out]


PART_B = 3
PART_CASES = _part_cases()
PART_IDS = [c[0] for c in PART_CASES]


# ------------------------------------------------------------------------------------------------ geometry corners
# (id, w, n_mels, mel term, B, T, seed): one scale holding a magnitude-only STFT term and one mel term.  No case is removed by the
# empty-filter rule: none of the (w, n_mels) pairs below has only empty bands (w = 12 with 5 bands has exactly one, w = 8 with 5 bands two).
def _geometry_cases():
    out = []
    i = 0
    for w in (8, 12, 40, 100, 32, 512):
        hop = w // 4
        Ts = [w // 2 + 1, w // 2 + 2, w - 1, w, w + 1, 5 * hop - 1, 5 * hop, 5 * hop + 1, 1001 if w != 100 else 1003]
        for T in sorted(set(Ts)):
            n, B = (1, 2, 5)[i % 3], (1, 2, 3, 7)[i % 4]
            out.append((w, n, (MEL_DEFAULT, MEL_POW2_MAG)[i % 2], B, T, 1000 + i))
            i += 1
    # B * (T // hop + 1) = 255, 256, 257 (a 256-column workgroup's edge) and 255 again from three clips, at hop 8
    for w, n, B, T in ((32, 5, 1, 2035), (32, 5, 2, 1019), (32, 5, 1, 2051), (32, 2, 3, 675)):
        out.append((w, n, MEL_DEFAULT, B, T, 1000 + i))
        i += 1
    out.append((12, 5, MEL_DEFAULT, 3, 1001, 1000 + i))           # exactly one empty band, the padding columns of 3 * 334 = 1002 frames
    ided = [(f"w{w}-n{n}-{'p2' if t is MEL_POW2_MAG else 'p1'}-B{B}-T{T}", w, n, t, B, T, seed) for w, n, t, B, T, seed in out]
    return [c[:6] + (REPLACED_SEEDS.get(c[0], c[6]),) for c in ided]


GEOMETRY_CASES = _geometry_cases()
GEOMETRY_IDS = [c[0] for c in GEOMETRY_CASES]
ONE_EMPTY_BAND = (12, 5)                                           # (w, n_mels): band 0 holds no bin


def geometry_scale(w, n, mel_term):
    return dict(mel_scale(w, n, mel_term), stft=STFT_MAG)


def n_columns(w, B, T):
    return B * (T // (w // 4) + 1)


# ------------------------------------------------------------------------------------------------ one plan of three kinds of scale
MIXED = dict(stft_windows=[64, 128], mel_windows=[40, 128], n_mels=[5, 20], B=3, T=1001, seed=77)


def mixed_scales():
    """The scales SpectralLosses builds for MIXED: mel-only w = 40, shared w = 128, STFT-only (magnitude part) w = 64."""
    return [mel_scale(40, 5), dict(mel_scale(128, 20), stft=STFT_MAG), stft_scale(64, STFT_MAG)]


# ------------------------------------------------------------------------------------------------ wm = gain * x exactly
# (w, gain, seed), B = 3, T = 1101: a magnitude-only and a raised-clamp STFT scale, and the default mel term of that window
GAIN_CASES = [(32, 2.0, 21), (32, 0.5, 22), (512, 2.0, 23), (512, 0.5, 24)]
GAIN_B, GAIN_T = 3, 1101


def gain_clips(gain, seed):
    x = (0.1 * np.random.default_rng(seed).standard_normal((GAIN_B, 1, GAIN_T))).astype(np.float32)
    return (np.float32(gain) * x).astype(np.float32), x                 # a power of two: exact in float32


# ------------------------------------------------------------------------------------------------ independent clips of one batch
# five clips of different content, clip 1 silent on both sides; a conditioned plan (magnitude-only STFT at 64 and 512, mel at 32 / 128 / 512)
BATCH = dict(stft_windows=[64, 512], mel_windows=[32, 128, 512], n_mels=[5, 20, 80], B=5, T=1201, seed=94, silent=1)      # seeds 91..93 had an element at a gradient jump


def batch_clips():
    wm, x = clips(BATCH["B"], BATCH["T"], BATCH["seed"])
    wm[BATCH["silent"]] = 0.0
    x[BATCH["silent"]] = 0.0
    return wm, x


def batch_scales():
    return [mel_scale(32, 5), mel_scale(128, 20), dict(mel_scale(512, 80), stft=STFT_MAG), stft_scale(64, STFT_MAG)]


# ------------------------------------------------------------------------------------------------ guard-band plans
# (id, scales, B, T, seed, bar of the combined gradient): the default plan holds the reference's clamp and keeps its bar
def guard_cases():
    return [("default-B2-T4800", default_scales(), 2, 4800, 31, GRAD_BAR_LOG_REF), ("default-B3-T1100", default_scales(), 3, 1100, 32, GRAD_BAR_LOG_REF),
            ("stft-only-B3-T1100", [stft_scale(512, STFT_MAG), stft_scale(100, STFT_MAG)], 3, 1100, 33, GRAD_BAR),
            ("mel-only-w40-B2-T1001", [mel_scale(40, 5)], 2, 1001, 34, GRAD_BAR)]


def default_scales():
    """The scales of the default SpectralLosses: the seven mel scales, 512 and 2048 shared with the STFT loss."""
    ref = (1.0, 1.0, 2.0, 1e-5)
    return [dict(mel_scale(w, n), stft=ref if w in (2048, 512) else None) for n, w in zip(MEL_N, MEL_W)]


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
REFUSAL = dict(B=2, T=400, seed=3, T_short=33)


def refusal_scales():
    return [geometry_scale(32, 5, MEL_DEFAULT), stft_scale(64, STFT_MAG)]


def refusal_clips():
    """-> (wm, x [B, 1, T], and the [B, 1, T_short] clips a call with T = T_short reads from the same buffers)."""
    m = REFUSAL
    wm, x = clips(m["B"], m["T"], m["seed"])
    short = lambda a: a.reshape(-1)[: m["B"] * m["T_short"]].reshape(m["B"], 1, m["T_short"]).copy()      # noqa: E731
    return wm, x, short(wm), short(x)


def c_call(plan, wm, x, terms, totals, dwm, ws, stft_scale=1.0, mel_scale=1.0, B=None, T=None, ws_bytes=None):
    """wv_specloss through ctypes on device tensors (None passes a null pointer) -> the return code."""
    import ctypes as C
    import torch
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    B, T = (wm.shape[0] if B is None else B), (wm.shape[-1] if T is None else T)
    return plan._lib.wv_specloss(plan._h, ptr(wm), ptr(x), B, T, ptr(terms), ptr(totals), ptr(dwm), float(stft_scale), float(mel_scale), ptr(ws),
                                 (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


def rel_err(got, ref):
    """max |got - ref| / max |ref| over the tensor (0 when both are all zero)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = float(np.abs(ref).max())
    e = float(np.abs(got - ref).max())
    return e / m if m > 0 else e
