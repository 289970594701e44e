"""Seeded case lists of the training-kernel geometry fuzz (tests/test_gpu_train_fuzz.py), and next to them a short Python restatement of
the shape dispatch in waveverify_amd/csrc/wv_train.hip -- which dW-GEMM tile / loader / split plan, which stencil-backward kernel, which
ConvTranspose and tail kernel a shape gets.  tests/test_train_fuzz_cases_cpu.py asserts on these lists that every route keeps its cases:
a change to a launcher (restate it here) or to a generator that silently empties a route fails there, by the route's name.
Pure Python: no GPU, no library."""
import numpy as np

# ---- the launchers' shape dispatch, restated ---------------------------------------------------------------------------------------
NT_TC = 512                                                       # nt_plan: samples per (clip, chunk) work item


def nt_tile(M, K):
    """wv::nt_tile: 128-row tiles unless they pad the matrix much more than 64-row tiles do."""
    if M <= 64 or K <= 64:
        return 64
    p128 = -(-M // 128) * -(-K // 128) * 128 * 128
    p64 = -(-M // 64) * -(-K // 64) * 64 * 64
    return 128 if p128 * 100 <= p64 * 115 else 64


def nt_plan(B, T, M, K):
    """nt_plan + launch_gemm_nt: dW[M, K] = sum over B clips x T samples -> dict(tile, tiles, items, S, vec, last)."""
    te = nt_tile(M, K)
    tiles = -(-M // te) * -(-K // te)
    items = B * -(-T // NT_TC)
    S = min(items, max(1, 1024 // tiles))
    while S > 1 and S * M * K > (32 << 20):
        S //= 2
    return dict(tile=te, tiles=tiles, items=items, S=S, vec=T % 4 == 0, last=T - (-(-T // NT_TC) - 1) * NT_TC)


DW_ROUTES = ("vec51", "down2", "down4", "down5", "down8", "k5s1", "k1s1", "k4s2", "k8s4", "k10s5", "k16s8", "generic")
_PAIRS = {(5, 1): "k5s1", (1, 1): "k1s1", (4, 2): "k4s2", (8, 4): "k8s4", (10, 5): "k10s5", (16, 8): "k16s8"}


def dw_bwd_route(ks, stride, Tin, fused_dot=False, dh=True, h_shared=False):
    """launch_dw_bwd for a causal stencil (pad = ks - stride, Tout = ceil(Tin / stride)) on 16-byte aligned operands."""
    Tout = -(-Tin // stride)
    if fused_dot:
        return "fused_dot"
    if ks == 5 and stride == 1 and dh and not h_shared and Tin % 4 == 0:
        return "vec51"
    if dh and not h_shared and ks == 2 * stride and Tout * stride == Tin and stride in (2, 4, 5, 8):
        return f"down{stride}"
    return _PAIRS.get((ks, stride), "generic")


def up_route(r):
    """wv_train_up_backward: per-frame ConvTranspose kernels for the net's ratios, convtr_fwd_kernel / convtr_bwd_kernel otherwise."""
    return f"frame{r}" if r in (2, 4, 5, 8) else "generic"


def tail_route(ks, Tin, T):
    """wv_train_tail_backward."""
    return "vec5" if ks == 5 and T % 4 == 0 and Tin % 4 == 0 else "generic"


def block_backward_routes(T):
    """wv_train_block_backward on 16-byte aligned operands (dw_bwd_can_fuse_scale: T % 4 == 0, which the block demands anyway):
    -> (stencil-backward route of the second half, of the first half)."""
    fuse = T % 4 == 0
    return dw_bwd_route(5, 1, T, fused_dot=fuse), dw_bwd_route(5, 1, T)


def block_forward_route(C, T):
    """wv_train_block_forward: the one-launch kernel (rb_supported) or two unit launches."""
    return "one_launch" if C in (64, 96, 128, 192) and T >= 4 and T % 4 == 0 else "two_launch"


# ---- generators ------------------------------------------------------------------------------------------------------------------------
UNIT_BOUND = 6e6                                                  # B * max(K, M) * T: keeps a case's float64 oracle in the low seconds


# the forms a plain draw of the recipe rarely reaches under the size bound (the 128-row tile needs M, K > 64; with the vector loader also
# T % 4 == 0): written out, so that the coverage conditions live in tests/test_train_fuzz_cases_cpu.py alone
UNIT_EXPLICIT = [(2, 128, 192, 1280, 10, 5, True, True),          # down5, tile 128, vector loader
                 (3, 130, 129, 1028, 5, 1, True, False),          # 5/1 vector kernel, tile 128 with clamped rows, vector loader
                 (17, 200, 256, 64, 16, 8, False, True),          # down8 at B = 17, tile 128 with clamped columns, vector loader
                 (9, 96, 97, 63, 4, 2, False, True)]              # k4s2 (odd T leaves the down2 kernel), tile 64, scalar loader


def unit_cases(n=64, seed=2025):
    """-> [(B, K, M, T, ks, stride, elu, need_dx)]: n - 4 plain seeded draws of the recipe, then UNIT_EXPLICIT."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n - len(UNIT_EXPLICIT):
        r = int(rng.choice([1, 1, 2, 3, 4, 5, 8]))
        ks = int(rng.choice([1, 3, 5, 5, 7, 16])) if r == 1 else int(rng.choice([2 * r, 2 * r, r, min(16, 2 * r + 1)]))
        K = int(rng.choice([1, 3, 8, 17, 32, 33, 64, 65, 96, 100, 128, 130, 192, 200, 256]))
        M = int(rng.choice([1, 4, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 192, 256, 260]))
        T = int(rng.choice([1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1028, 1541])) * int(rng.choice([1, r]))
        B = int(rng.choice([1, 2, 3, 7, 8, 9, 17]))
        elu = bool(rng.integers(0, 2))
        if B * max(K, M) * T > UNIT_BOUND:
            continue
        out.append((B, K, M, T, ks, r, elu, len(out) % 4 != 3))
    return out + UNIT_EXPLICIT


def block_cases(n=12, seed=2026):
    """-> [(B, C, T, with_param)], T % 4 == 0"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        C = int(rng.choice([8, 24, 40, 64, 96, 100, 128, 160, 192, 256]))
        T = int(rng.choice([4, 8, 36, 52, 256, 508, 512, 516, 1028]))
        B = int(rng.choice([1, 3, 8, 9]))
        if B * C * T > UNIT_BOUND / 2:
            continue
        out.append((B, C, T, len(out) % 2 == 0))
    return out


def up_cases(seed=2027):
    """-> [(B, K, M, Tin, r)]: r = 1..8 three times each."""
    rng = np.random.default_rng(seed)
    out = []
    for r in [1, 2, 3, 4, 5, 6, 7, 8] * 3:
        K = int(rng.choice([2, 6, 16, 30, 48, 64, 100, 128]))
        M = int(rng.choice([1, 8, 24, 40, 64, 96, 100]))
        Tin = int(rng.choice([1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257]))
        out.append((int(rng.choice([1, 2, 7, 9])), K, M, Tin, r))
    return out


def tail_cases():
    """-> [(B, C, Tin, T, ks)]: every kernel size; T = Tin, T = Tin - 3, T < ks; at ks = 5 both sides of T % 4 and Tin % 4."""
    return [(2, 8, 40, 40, 1), (3, 1, 5, 2, 1), (2, 96, 67, 64, 3), (1, 8, 2, 2, 3), (3, 8, 44, 44, 5), (2, 96, 47, 44, 5), (2, 1, 48, 45, 5),
            (9, 8, 4, 4, 5), (2, 8, 300, 297, 7), (1, 96, 5, 5, 7), (2, 8, 515, 512, 16), (3, 96, 16, 13, 16), (2, 1, 1, 1, 16)]


def head_cases():
    """-> [(B, D, O, nb, hop, N, T)], T in ((N - 1) * hop, N * hop]: one frame, hop - 1 / hop + 1 samples, odd D / O / nb."""
    return [(1, 3, 5, 1, 4, 1, 1), (2, 7, 3, 3, 6, 1, 5), (3, 9, 5, 5, 6, 2, 7), (2, 5, 7, 16, 2, 9, 18), (7, 33, 9, 3, 21, 3, 43), (9, 17, 3, 1, 1, 5, 5)]


def convpre_cases():
    """-> [(B, C, T, ks)]"""
    return [(1, 3, 1, 3), (2, 5, 2, 5), (9, 7, 33, 7), (3, 6, 513, 5), (8, 13, 511, 3), (17, 10, 5, 7)]


def convpost_cases():
    """-> [(B, C, D, T, ks, l2norm)]"""
    return [(1, 3, 5, 1, 3, True), (2, 6, 3, 2, 5, True), (9, 10, 7, 5, 7, True), (3, 65, 9, 33, 5, False), (8, 129, 33, 7, 3, True), (2, 7, 1, 65, 5, False)]


def spec_cases():
    """-> [(B, C, F, T)], F = n_fft / 2 + 1 for n_fft in {8, 12, 64, 130}"""
    return [(1, 3, 5, 1), (2, 6, 7, 3), (9, 10, 33, 5), (3, 65, 66, 31), (8, 5, 66, 513), (2, 130, 33, 65)]


def film_cases():
    """-> [(embedding_dim, embedding_layers, strides, B, C, T, scale)]"""
    return [(8, 1, [2, 2], 1, 8, 5, 0), (16, 2, [3, 2], 5, 12, 33, 1), (256, 3, [2, 3, 2], 9, 20, 7, 2), (256, 1, [4, 2], 5, 4, 1, 1),
            (8, 3, [2, 2, 2], 9, 36, 64, 0), (16, 2, [5, 2], 1, 100, 129, 1)]


def split_plan_cases():
    """The dW GEMM's item loop with more items than splits -> [(kind, B, C (= M), F (= K), T)]"""
    return [("spec", 17, 129, 129, 3076), ("spec", 17, 129, 129, 3077), ("spec", 17, 200, 201, 7684), ("unit", 17, 129, 129, 3076)]


NET_STRIDES = [[3, 2], [2, 3, 2], [5, 2], [7, 3], [6, 5], [2, 2, 2, 2], [4, 4], [8, 2]]


def net_cases(seed=2028):
    """Eight whole-net configurations, one per stride set -> [(idx, cfg kwargs, T, B)]; T = 4 * hop * n (blocks need T % 4 == 0 at every stage)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, strides in enumerate(NET_STRIDES):
        nbits = int(rng.choice([3, 5, 16]))
        kw = dict(strides=list(strides), channels_enc=int(rng.choice([4, 8, 12, 16])), channels_dec=int(rng.choice([4, 8, 12])),
                  dimension=int(rng.choice([8, 16, 24])), n_fft_base=int(rng.choice([8, 16])),
                  n_residual_enc=int(rng.integers(1, 4)), n_residual_dec=int(rng.integers(1, 4)),
                  kernel_size=int(rng.choice([3, 5, 7])), last_kernel_size=int(rng.choice([3, 5, 7])),
                  residual_kernel_size=5, dilation_base=1, embedding_dim=int(rng.choice([8, 16])), embedding_layers=int(rng.integers(1, 4)),
                  output_dim=int(rng.choice([4, 8])), nbits=nbits, msg_dimension=nbits)
        hop = int(np.prod(strides))
        out.append((i, kw, 4 * hop * int(rng.choice([1, 2, 5])), int(rng.integers(1, 4))))
    return out
