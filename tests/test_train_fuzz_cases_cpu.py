"""Coverage conditions of the training-geometry fuzz (tests/train_fuzz_cases.py), checked on the generated lists without a GPU: every
kernel route that wv_train.hip's launchers can pick keeps its cases.  A statement of intent about shapes (the routes are restated in
train_fuzz_cases.py from the launchers' source); it does not inspect binaries.  Also: the oracle's SpecBlock backward after its
contractions moved from einsum to matmul."""
from collections import Counter

import numpy as np

import train_fuzz_cases as FC


def _need(count, route, n, what):
    assert count.get(route, 0) >= n, f"{what}: route '{route}' has {count.get(route, 0)} case(s), needs {n}"


def test_lists_are_deterministic_and_bounded():
    assert FC.unit_cases() == FC.unit_cases() and FC.block_cases() == FC.block_cases() and FC.up_cases() == FC.up_cases()
    assert FC.net_cases() == FC.net_cases()
    assert len(FC.unit_cases()) == 64 and len(FC.block_cases()) == 12 and len(FC.up_cases()) == 24 and len(FC.net_cases()) == 8
    for B, K, M, T, ks, stride, elu, need_dx in FC.unit_cases():
        assert B * max(K, M) * T <= FC.UNIT_BOUND and 1 <= stride <= ks <= 16


def test_unit_cases_reach_every_stencil_backward_route():
    routes = Counter(FC.dw_bwd_route(ks, stride, T) for B, K, M, T, ks, stride, elu, need_dx in FC.unit_cases())
    print("ROUTES launch_dw_bwd (unit cases):", dict(routes))
    assert set(routes) <= set(FC.DW_ROUTES)
    for r in FC.DW_ROUTES:
        _need(routes, r, 2, "launch_dw_bwd")
    # the run-time <0,0> form at many (ks, stride) pairs, not at one
    generic = {(ks, stride) for B, K, M, T, ks, stride, elu, need_dx in FC.unit_cases() if FC.dw_bwd_route(ks, stride, T) == "generic"}
    assert len(generic) >= 6, generic


def test_unit_cases_reach_every_dw_gemm_form():
    cases = FC.unit_cases()
    forms = Counter((p["tile"], p["vec"]) for p in (FC.nt_plan(B, T, M, K) for B, K, M, T, *_ in cases))
    print("ROUTES gemm_nt (tile, vector loader) (unit cases):", dict(forms))
    for tile in (64, 128):
        for vec in (True, False):
            _need(forms, (tile, vec), 3, "gemm_nt (tile, vector loader)")
    assert sum(B > 8 for B, *_ in cases) >= 8, "dw_param_grads_kernel: clip groups past the eighth need B > 8"
    assert {7, 8, 9, 17} <= {B for B, *_ in cases}
    for edge in (0, 1, 511):
        assert any(T % 512 == edge for B, K, M, T, *_ in cases), f"chunk edge T % 512 == {edge} is gone"
    assert sum(not need_dx for *_, need_dx in cases) >= 15
    assert any(K == 1 for B, K, *_ in cases) and any(ks == 1 for B, K, M, T, ks, *_ in cases)     # one-element weight-norm rows
    # rows clamped: M or K that is no multiple of the tile, in both tile sizes
    for tile in (64, 128):
        assert any(FC.nt_tile(M, K) == tile and (M % tile or K % tile) for B, K, M, *_ in cases), tile


def test_split_plan_cases_run_the_item_loop():
    plans = []
    for kind, B, M, K, T in FC.split_plan_cases():
        p = FC.nt_plan(B, T, M, K)
        plans.append(p)
        assert p["items"] > p["S"], f"gemm_nt item loop: {kind} {(B, M, K, T)} has one item per split ({p})"
    assert plans[0] == dict(tile=64, tiles=9, items=119, S=113, vec=True, last=4)
    assert plans[1]["vec"] is False and plans[1]["S"] == 113
    assert plans[2] == dict(tile=128, tiles=4, items=272, S=256, vec=True, last=4) and 200 % 128 and 201 % 128
    assert plans[3] == plans[0]
    # ... and nowhere else at the unit level: what the hand-picked lists never reached
    assert all(FC.nt_plan(B, T, M, K)["items"] == FC.nt_plan(B, T, M, K)["S"] for B, K, M, T, *_ in FC.unit_cases())


def test_block_cases_reach_both_forward_routes():
    cases = FC.block_cases()
    routes = Counter(FC.block_forward_route(C, T) for B, C, T, wp in cases)
    print("ROUTES block forward:", dict(routes))
    _need(routes, "one_launch", 3, "wv_train_block_forward")
    _need(routes, "two_launch", 3, "wv_train_block_forward")
    assert all(T % 4 == 0 for B, C, T, wp in cases)
    assert {wp for *_, wp in cases} == {True, False} and any(B > 8 for B, *_ in cases)
    # by the restated wv_train_block_backward: the second half takes the fused-dot stencil backward, the first the 5/1 vector kernel
    back = Counter(FC.block_backward_routes(T) for B, C, T, wp in cases)
    print("ROUTES block backward (second half, first half):", dict(back))
    _need(back, ("fused_dot", "vec51"), len(cases), "wv_train_block_backward")


def test_up_cases_reach_the_generic_convtranspose_kernels():
    cases = FC.up_cases()
    per_r = Counter(r for *_, r in cases)
    routes = Counter(FC.up_route(r) for *_, r in cases)
    print("ROUTES ConvTranspose:", dict(routes))
    for r in range(1, 9):
        _need(per_r, r, 3 if r in (1, 3, 6, 7) else 2, "TrainUp ratio")
    for r in (2, 4, 5, 8):
        _need(routes, f"frame{r}", 2, "convtr_*_frame_kernel")
    _need(routes, "generic", 12, "convtr_fwd_kernel / convtr_bwd_kernel")
    assert any(B > 8 for B, *_ in cases) and any(Tin == 1 for B, K, M, Tin, r in cases) and any(Tin * r > 512 for B, K, M, Tin, r in cases)


def test_tail_cases_reach_both_kernels_and_the_edges():
    cases = FC.tail_cases()
    routes = Counter(FC.tail_route(ks, Tin, T) for B, C, Tin, T, ks in cases)
    print("ROUTES tail backward:", dict(routes))
    _need(routes, "vec5", 2, "tail_bwd5_vec_kernel")
    _need(routes, "generic", 2, "tail_bwd_kernel")
    assert {ks for *_, ks in cases} == {1, 3, 5, 7, 16} and {C for B, C, *_ in cases} == {1, 8, 96}
    for ks in (1, 3, 5, 7, 16):
        mine = [(Tin, T) for B, C, Tin, T, k in cases if k == ks]
        assert any(T == Tin for Tin, T in mine) and any(T == Tin - 3 for Tin, T in mine), ks
        assert ks == 1 or any(T < ks for Tin, T in mine), ks
    five = [(Tin % 4 == 0, T % 4 == 0) for B, C, Tin, T, k in cases if k == 5]
    assert {(True, True), (False, True), (True, False)} <= set(five)


def test_small_family_shapes_are_ragged():
    for B, D, O, nb, hop, N, T in FC.head_cases():
        assert (N - 1) * hop < T <= N * hop and D % 2 and O % 2
    assert {1} <= {N for *_, N, T in FC.head_cases()} and any(T == hop - 1 for B, D, O, nb, hop, N, T in FC.head_cases())
    assert any(T == hop + 1 for B, D, O, nb, hop, N, T in FC.head_cases())
    assert {F for B, C, F, T in FC.spec_cases()} == {n // 2 + 1 for n in (8, 12, 64, 130)}
    assert any(C % 4 for B, C, F, T in FC.spec_cases()) and any(C % 4 for B, C, D, T, ks, l2 in FC.convpost_cases())
    assert {l2 for *_, l2 in FC.convpost_cases()} == {True, False}
    assert {E for E, *_ in FC.film_cases()} == {8, 16, 256} and {L for E, L, *_ in FC.film_cases()} == {1, 2, 3}
    assert {len(s) for E, L, s, *_ in FC.film_cases()} == {2, 3} and {B for E, L, s, B, *_ in FC.film_cases()} == {1, 5, 9}
    assert all(C % 4 == 0 and sc < len(s) for E, L, s, B, C, T, sc in FC.film_cases())


def test_net_cases_hold_what_the_trained_nets_never_combined():
    cases = FC.net_cases()
    assert [kw["strides"] for i, kw, T, B in cases] == FC.NET_STRIDES
    for i, kw, T, B in cases:
        hop = int(np.prod(kw["strides"]))
        assert T % (4 * hop) == 0 and kw["residual_kernel_size"] == 5 and kw["dilation_base"] == 1 and (2 * kw["channels_enc"]) % 4 == 0
    assert {kw["kernel_size"] for i, kw, T, B in cases} - {5} and {kw["last_kernel_size"] for i, kw, T, B in cases} - {5}
    assert 3 in {kw["n_residual_enc"] for i, kw, T, B in cases} and 3 in {kw["n_residual_dec"] for i, kw, T, B in cases}
    assert {1, 3} <= {kw["embedding_layers"] for i, kw, T, B in cases}
    ratios = Counter(r for i, kw, T, B in cases for r in kw["strides"])
    for r in (3, 6, 7):
        _need(ratios, r, 1, "whole-net stride (generic ConvTranspose / stencil kernels)")


def test_oracle_matmul_contractions_equal_einsum():
    """oracle.wv_oracle_train contracts channels with matmul (the split-plan cases are 100 MB tensors; einsum took seconds there):
    the two helpers and spec_add_backward against the einsum forms they replaced, to 1e-12."""
    from oracle import wv_oracle_train as OT
    rng = np.random.default_rng(0)
    W, a, dh = rng.standard_normal((7, 5)), rng.standard_normal((3, 5, 19)), rng.standard_normal((3, 7, 19))
    assert np.abs(OT._apply(W, a) - np.einsum("mk,bkt->bmt", W, a)).max() <= 1e-12
    assert np.abs(OT._apply(W.T, dh) - np.einsum("mk,bmt->bkt", W, dh)).max() <= 1e-12
    assert np.abs(OT._outer(dh, a) - np.einsum("bmt,bkt->mk", dh, a)).max() <= 1e-12
    B, C, F, T = 3, 7, 5, 19
    x, P, dy = (rng.standard_normal(s).astype(np.float32) for s in ((B, C, T), (B, F, T), (B, C, T)))
    g = (0.5 + np.abs(rng.standard_normal((C, 1, 1)))).astype(np.float32)
    v = rng.standard_normal((C, F, 1)).astype(np.float32)
    for sp in (None, np.array([0.7], np.float32)):
        got = OT.spec_add_backward(x, P, g, v, sp, 0.57, dy)
        s = 0.57 * (1.0 if sp is None else float(sp[0]))
        W = OT.fold(g.astype(np.float64), v.astype(np.float64))[:, :, 0]
        z = np.einsum("cf,bft->bct", W, P.astype(np.float64))
        G = np.einsum("bct,bft->cf", dy.astype(np.float64), P.astype(np.float64))
        dg, dv = OT.fold_backward(g.astype(np.float64), v.astype(np.float64), (s * G)[:, :, None])
        assert np.abs(got["y"] - (x + s * z)).max() <= 1e-12 and np.abs(got["dg"] - dg).max() <= 1e-12 and np.abs(got["dv"] - dv).max() <= 1e-12
        assert abs(got["d_scale_param"] - 0.57 * float((dy.astype(np.float64) * z).sum())) <= 1e-12
