"""The cases of tests/test_gpu_aug_backward.py (a plain module), shared with tests/test_oracle_fx_dense.py, which holds the backward oracle
to torch's autograd on the CPU.  A map is (kind, mode, a, b, c, perm, t_out) with the WV_SEQ_* mode numbers of include/waveverify_hip.h."""
from __future__ import annotations

import numpy as np

IDENTITY, REVERSE, ROLL, PERMUTE, CHUNK_SWAP = range(5)

SHAPES = [(4, 1, 1600, 160),       # T % 4 == 0: the forward's 16-byte run path
          (3, 2, 999, 50),         # ragged last segment
          (2, 3, 5, 2),
          (1, 1, 1, 1600)]


def maps(T: int):
    """Every map the clip length allows, by name."""
    out = [("identity", IDENTITY, 0, 0, 0, None, T), ("reverse", REVERSE, 0, 0, 0, None, T)]
    if T > 1:
        out += [(f"roll_{n}", ROLL, a, 0, 0, None, T) for n, a in (("1", 1), ("Tm1", T - 1), ("Tdiv3", max(1, T // 3)))]
    for n, sz in (("Tdiv7", max(1, T // 7)), ("2", 2)):
        if T >= 2 * sz:                                        # t_out = (T // sz) * sz < T where T allows: the tail is dropped
            k = T // sz
            perm = np.random.default_rng(T * 31 + sz).permutation(k).astype(np.int32)
            out.append((f"permute_{n}", PERMUTE, sz, 0, 0, perm, k * sz))
    if T >= 4:
        c = T // 4
        out += [("swap_a_lt_b_adjacent", CHUNK_SWAP, 1, 1 + c, c, None, T),          # a + c == b
                ("swap_b_lt_a_to_the_end", CHUNK_SWAP, T - c, 0, c, None, T)]
    return out


def cases():
    return [(shape, m) for shape in SHAPES for m in maps(shape[2])]


def case_id(case) -> str:
    (B, C, T, seg), m = case
    return f"B{B}C{C}T{T}seg{seg}-{m[0]}"


def forced_codes(B: int, nseg: int):
    """Clip 0's first segments: keep, revert, zero and, with a second clip, clip 1's original -- as many as the clip has segments."""
    return ([0, 1, 2] + ([3 + 1] if B >= 2 else []))[:nseg]


def plan(B: int, T: int, seg: int, seed: int) -> np.ndarray:
    """A seeded plan [B][nseg] (0 keep, 1 revert, 2 zero, 3 + j clip j's original) with clip 0's first segments forced to `forced_codes`
    and at least a third of all segments kept, so that the expected gradient is not mostly zeros."""
    rng = np.random.default_rng(seed)
    nseg = -(-T // seg)
    p = rng.integers(0, 3 + B, (B, nseg)).astype(np.int32)
    p[rng.random((B, nseg)) < 0.4] = 0
    forced = forced_codes(B, nseg)
    p[0, :len(forced)] = forced
    free = [(b, s) for b in range(B) for s in range(nseg) if not (b == 0 and s < len(forced))]
    while 3 * int((p == 0).sum()) < p.size:
        b, s = free[int(rng.integers(len(free)))]
        p[b, s] = 0
    return p
