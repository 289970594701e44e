"""Cases of the learnable-STFT-basis tests (a plain module: `import spec_learnable_cases as SLC`), shared by the fixture script
(tests/golden/make_golden_spec_learnable.py), the CPU self-checks and the GPU tests: the unit shapes, the seeded inputs (numpy Philox
streams, the same everywhere), which rows of a large gradient the fixture stores, and a torch restatement of the gradient formula
the kernels implement."""
from __future__ import annotations

import os

import numpy as np

UNIT_SHAPES = [(64, 1, 3, 67), (64, 1, 2, 1), (128, 2, 2, 131), (256, 8, 2, 100), (512, 40, 2, 4800), (1024, 320, 2, 4800)]   # n_fft, hop, B, T
VARIANTS = ("dft", "noisy")
MEAN, STD = -4.3, 2.8
NOISE_REL = 0.05
SUBSET_FROM, SUBSET_ROWS = 256, 32          # n_fft >= SUBSET_FROM: the fixture stores SUBSET_ROWS seeded rows + the two side rows
STORED_BYTES = 48 << 10                     # a larger wav / dP is rebuilt from its seed (the fixture holds its sum and sum of squares)
NET = dict(channels_enc=8, channels_dec=8, n_residual_dec=2, dimension=16, strides=[2, 2], n_fft_base=16, zero_init=True)
NET_SEED, NET_B, NET_T, NET_LR, NET_MAX_NORM = 7, 2, 64, 1e-4, 1000.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_learnable.npz")


def rng(tag: str) -> np.random.Generator:
    from waveverify_amd.init import _rng
    return _rng(0, "spec_learnable/" + tag)


def unit_inputs(i: int):
    """(wav [B,1,T] float32, dP [B,F,Tf] float32) of unit shape i: shared by the two bases.  One clip holds exact silence: n_fft + hop
    (or, in a clip too short for that, n_fft + 1) samples in its middle, or the first 9/10 of a clip no longer than n_fft + 1; at T = 1
    its only sample is 1.4e-4 (some bins of the noisy basis under the clamp, all of the analytic one's)."""
    n_fft, hop, B, T = UNIT_SHAPES[i]
    wav = (0.1 * rng(f"u{i}/wav").standard_normal((B, 1, T))).astype(np.float32)
    if T == 1:
        wav[1, 0, 0] = 1.4e-4
    elif T > n_fft + 1:
        L = n_fft + hop if T >= n_fft + hop + 2 else n_fft + 1            # n_fft + hop: a whole frame falls inside whatever the phase
        wav[1, 0, (T - L) // 2: (T - L) // 2 + L] = 0.0
    else:
        wav[1, 0, : (9 * T) // 10] = 0.0
    dP = rng(f"u{i}/dP").standard_normal((B, n_fft // 2 + 1, -(-T // hop))).astype(np.float32)
    return wav, dP


def unit_basis(n_fft: int, variant: str) -> np.ndarray:
    """[2F, n_fft] float32: the reference's buffer ("dft"), or it plus NOISE_REL * peak * N(0, 1) on every row ("noisy")."""
    from waveverify_amd.checkpoint import stft_basis
    b = stft_basis(n_fft).numpy()[:, 0, :]
    if variant == "dft":
        return b
    b64 = b.astype(np.float64)
    return (b64 + NOISE_REL * float(np.abs(b64).max()) * rng(f"basis/{n_fft}").standard_normal(b64.shape)).astype(np.float32)


def sums(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return np.array([a.sum(), (a * a).sum()])


def check_rows(n_fft: int):
    """Rows of a noisy basis the fixture keeps to check the rebuilt one: sin_0, sin_{F-1}, cos_1, sin_1."""
    F = n_fft // 2 + 1
    return [F, 2 * F - 1, 1, F + 1]


def subset_rows(n_fft: int) -> np.ndarray:
    """The stored rows of a large gradient: sin_0, sin_{F-1} and SUBSET_ROWS seeded others, ascending."""
    F = n_fft // 2 + 1
    rest = np.setdiff1d(np.arange(2 * F), [F, 2 * F - 1])
    pick = rng(f"rows/{n_fft}").choice(rest, SUBSET_ROWS, replace=False)
    return np.sort(np.concatenate([pick, [F, 2 * F - 1]])).astype(np.int64)


def formula_grad(basis: np.ndarray, wav: np.ndarray, dP: np.ndarray, n_fft: int, hop: int, std: float = STD):
    """The four formulas of the kernels in float64, no autograd:  C = Basis @ frames(wav);  p = re^2 + im^2;
    dC = dP * {re, im} / (std * p) where p > 1e-10 else 0;  dBasis[m][n] = sum_{b,t} dC[b][m][t] * frames[b][n][t].
    -> (dBasis [2F, n_fft] float64, share of bins with p <= 1e-10)."""
    import torch
    import torch.nn.functional as Fn
    F = n_fft // 2 + 1
    w = Fn.pad(torch.from_numpy(wav).double(), (n_fft - 1, 0))                     # causal: n_fft - 1 zeros in front
    frames = w.unfold(-1, n_fft, hop)[:, 0].transpose(1, 2)                        # [B, n_fft, Tf]
    Cm = torch.einsum("mn,bnt->bmt", torch.from_numpy(basis).double(), frames)
    re, im = Cm[:, :F], Cm[:, F:]
    p = re * re + im * im
    live = p > 1e-10
    g = torch.where(live, torch.from_numpy(dP).double() / (std * torch.where(live, p, torch.ones_like(p))), torch.zeros_like(p))
    dC = torch.cat([g * re, g * im], dim=1)
    return torch.einsum("bmt,bnt->mn", dC, frames).numpy(), float((~live).double().mean())


def load_unit(g, i: int, variant: str):
    """One unit case of the loaded fixture `g` -> dict(n_fft, hop, B, T, wav, dP, basis, rows (None = all), dBasis (the stored rows),
    peak, fro, ref32, silent_share); what the fixture does not store in full is rebuilt from its seed and checked against what it does."""
    n_fft, hop, B, T = (int(v) for v in g["unit_shapes"][i])
    assert (n_fft, hop, B, T) == UNIT_SHAPES[i]
    k = f"u{i}_{variant}_"
    wav, dP = unit_inputs(i)
    for name, a in (("wav", wav), ("dP", dP)):
        if f"u{i}_{name}" in g.files:
            assert np.array_equal(a, g[f"u{i}_{name}"]), name
        else:
            assert np.array_equal(sums(a), g[f"u{i}_{name}_sums"]), name
    basis = unit_basis(n_fft, variant)
    if variant == "noisy":
        assert np.array_equal(basis[check_rows(n_fft)], g[k + "basis_check"])
    rows = g[k + "rows"] if k + "rows" in g.files else None
    assert rows is None or np.array_equal(rows, subset_rows(n_fft))
    return dict(n_fft=n_fft, hop=hop, B=B, T=T, wav=wav, dP=dP, basis=basis, rows=rows, dBasis=g[k + "dBasis"].astype(np.float64),
                stored_f64=g[k + "dBasis"].dtype == np.float64, peak=float(g[k + "peak"]), fro=float(g[k + "fro"]), ref32=float(g[k + "ref32"]),
                silent_share=float(g[k + "silent_share"]))
