"""Cases and float64 restatements shared by the validation-metric tests (a plain module: `from validation_cases import ...`).

tests/golden/validation_metrics.npz (make_golden_validation.py) holds what the reference's SISNR and BER returned; tests/golden/metrics.npz
(make_golden_metrics.py) the scalar BER and the MIOU of earlier cases.  Everything here is computed once and must not be modified."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAL = np.load(os.path.join(GOLDEN, "validation_metrics.npz"))
MET = np.load(os.path.join(GOLDEN, "metrics.npz"))
GRID = 32768.0
EPS = 1e-8


# ---- SI-SNR -------------------------------------------------------------------------------------------------------------------------
def sisnr_f64(est: np.ndarray, ref: np.ndarray, eps: float = EPS) -> np.ndarray:
    """SISNR.forward of the reference, statement by statement (two passes: the means first), in float64 -> per-clip dB.  [..., T]."""
    out, ref = est.astype(np.float64), ref.astype(np.float64)
    ref = ref - ref.mean(axis=-1, keepdims=True)
    out = out - out.mean(axis=-1, keepdims=True)
    ref_energy = (ref ** 2).sum(axis=-1, keepdims=True) + eps
    proj = (ref * out).sum(axis=-1, keepdims=True) * ref / ref_energy
    noise = out - proj
    ratio = (proj ** 2).sum(axis=-1) / ((noise ** 2).sum(axis=-1) + eps)
    return 10 * np.log10(ratio + eps)


def _si_case(i: int):
    ref_q, diff_q, dc = VAL[f"si{i}_ref"].astype(np.int64), VAL[f"si{i}_diff"].astype(np.int64), VAL[f"si{i}_dc"].astype(np.int64)
    est = ((ref_q + diff_q + dc[0]) / GRID).astype(np.float32)
    ref = ((ref_q + dc[1]) / GRID).astype(np.float32)
    f64 = float(sisnr_f64(est, ref))
    return dict(i=i, kind=str(VAL[f"si{i}_kind"]), T=est.shape[0], est=est, ref=ref, ref_f32=float(VAL[f"si{i}_out"]), f64=f64,
                d=abs(float(VAL[f"si{i}_out"]) - f64))


SI_CASES = [_si_case(i) for i in range(int(VAL["n_si"]))]      # d = the reference's own float32 distance from float64, the tolerance source
SI_BATCH = [int(i) for i in VAL["si_batch_cases"]]
SI_BATCH_MEAN = float(VAL["si_batch_mean"])


def sisnr_bound(f64_db: float) -> float:
    """Bound on |one-pass f64 - two-pass f64| in dB: 1e-6 dB below 60 dB.  Products of two float32 are exact in float64, so a moment of
    <= 16000 samples errs only by its additions: 16 in a thread, 8 tree levels in the workgroup, a few chunks, about 30 x 2^-53 = 3e-15
    relative.  The noise power is a difference of such moments that cancels by the signal-to-noise ratio itself, at most 10^6 below
    60 dB: three moments x 3e-15 x 10^6 = 1e-8 relative on the ratio, 4e-8 dB -- inside 1e-6 dB with room for the log10.  Above 60 dB the
    cancellation, and with it the bound, grows as 10^((dB - 60) / 10)."""
    return 1e-6 * max(1.0, 10.0 ** ((f64_db - 60.0) / 10.0))


# ---- BER ----------------------------------------------------------------------------------------------------------------------------
def ber_f64(logits: np.ndarray, mask, eps: float = EPS):
    """-> (avg [B,W] float64 of the float32 logits, valid [B,W] bool)."""
    B, W, T = logits.shape
    p = 1.0 / (1.0 + np.exp(-logits.astype(np.float32).astype(np.float64)))
    if mask is None:
        return p.sum(axis=2) / T, np.ones((B, W), bool)
    m = mask.astype(np.float64)
    n = np.broadcast_to(m.sum(axis=2), (B, W))
    return (p * m).sum(axis=2) / (n + eps), n > 0


def _val_ber_case(i: int):
    k = f"ber{i}_"
    return dict(name=f"val{i}", logits=VAL[k + "logits"], bits=VAL[k + "bits"], mask=VAL[k + "mask"] if k + "mask" in VAL.files else None,
                thr=float(VAL[k + "thr"]), out=float(VAL[k + "out"]), clip=VAL[k + "clip"], wrong=VAL[k + "wrong"], decoded=VAL[k + "decoded"],
                valid=VAL[k + "valid"])


def _met_ber_case(i: int):
    k = f"ber{i}_"
    return dict(name=f"met{i}", logits=MET[k + "logits"], bits=MET[k + "bits"].astype(np.float32), mask=MET[k + "mask"] if k + "mask" in MET.files else None,
                thr=float(MET[k + "thr"]), out=float(MET[k + "out"]))


VAL_BER = [_val_ber_case(i) for i in range(int(VAL["n_ber"]))]
MET_BER = [c for c in (_met_ber_case(i) for i in range(int(MET["n_ber"]))) if not np.isnan(c["out"])]     # the 17 cases the reference does not refuse


def ulp32(v: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def check_decode(case, errors, valid, avg):
    """errors [B], valid [B], avg [B,W] of one case against the reference's records and the float64 value."""
    errors, valid, avg = np.asarray(errors), np.asarray(valid), np.asarray(avg)
    thr = np.float32(case["thr"])
    decoded = (avg.astype(np.float32) >= thr).astype(np.int32)
    a64, ok64 = ber_f64(case["logits"], case["mask"])
    assert np.array_equal(valid, ok64.sum(axis=1)), (case["name"], valid, ok64.sum(axis=1))
    assert np.all(np.abs(avg.astype(np.float64) - a64) <= 2 * ulp32(a64)), (case["name"], float(np.abs(avg - a64).max()))
    if "decoded" in case:                                         # per-bit records of the reference
        assert np.array_equal(valid, case["valid"].sum(axis=1)), case["name"]
        assert np.array_equal(decoded, case["decoded"]), (case["name"], np.argwhere(decoded != case["decoded"]))
        assert np.array_equal(errors, case["wrong"].sum(axis=1)), (case["name"], errors, case["wrong"].sum(axis=1))
        for b in range(len(errors)):                             # and the reference's scalar of every clip on its own
            assert abs((errors[b] / valid[b] if valid[b] else 0.0) - case["clip"][b]) < 1e-7, (case["name"], b)
    total = int(valid.sum())
    got = errors.sum() / total if total else 0.0
    assert abs(got - case["out"]) < 1e-7, (case["name"], got, case["out"])           # the reference's scalar is a float32 ratio of integers
    if "decoded" not in case and total:                           # metrics.npz keeps the scalar only: the integer error count follows from it
        assert int(errors.sum()) == int(round(case["out"] * total)), case["name"]


# ---- MIOU ---------------------------------------------------------------------------------------------------------------------------
def _miou_cases():
    out = []
    for i in range(int(MET["n_miou"])):
        p, g, ref = MET[f"miou{i}_p"], MET[f"miou{i}_g"], float(MET[f"miou{i}_out"])
        if np.isnan(ref):
            continue
        out.append(dict(name=f"miou{i}", p=np.asarray(p, np.float32).reshape(-1, 1, p.shape[-1]), g=np.asarray(g, np.float32).reshape(-1, 1, g.shape[-1]), out=ref))
    return out


MIOU_CASES = _miou_cases()                                        # binary predictions: as a raw locator output they binarise to themselves


def iou_counts_np(p: np.ndarray, g: np.ndarray) -> np.ndarray:
    fg, g1, g0 = p[:, 0] > 0.5, g[:, 0] == 1, g[:, 0] == 0
    return np.stack([(fg & g1).sum(1), (fg | g1).sum(1), (~fg & g0).sum(1), (~fg | g0).sum(1)], axis=1).astype(np.int32)
