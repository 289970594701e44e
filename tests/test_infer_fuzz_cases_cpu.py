"""The case lists of the exact-inference fuzz (tests/infer_fuzz_cases.py) keep every route of the restated launchers and of the launch
plan: at least two cases per route, one where the route comes from a written-out list.  A launcher or generator change that empties a
route fails here by the route's name.  Also on record: which routes the older lists of tests/test_gpu_fuzz.py miss, and that the float64
evaluation of the forward oracle is the float32 one (the one pinned to the golden outputs) to float32 rounding.  No GPU, no library."""
import collections

import numpy as np

import infer_fuzz_cases as F
from oracle import wv_oracle as O


def _need(counts, route, n=2):
    assert counts.get(route, 0) >= n, f"route {route!r}: {counts.get(route, 0)} case(s), need {n}; all routes: {dict(sorted(counts.items(), key=str))}"


def _report(title, counts):
    print(f"\n{title}: " + ", ".join(f"{k}: {v}" for k, v in sorted(counts.items(), key=str)))


def _pw_dw_routes(cases, args):
    c = collections.Counter()
    for case in cases:
        a = args(case)
        name, i = F.launch_pw_dw(a)
        c[("core", i["core"])] += 1
        c[("name", name)] += 1
        if i["core"] == "k1":
            c[("k1 window", i["bn"])] += 1
            c[("k1 tile height", i["bm"])] += 1
            c[("k1 epilogue", {0: "k5 resid" if a.resid else "k5", 1: "generic"}.get(i["epi"], f"stride {i['epi']}"))] += 1
            c[("k1 loader", i["ldr"])] += 1
            c[("k1 stages", i["stages"])] += 1
            if i["flat"]:
                c[("k1 flat", "r8" if i["epi"] == 8 else "convtr" if a.ct else "k5")] += 1
            if i["epi"] == 1 and a.film and a.M // a.bands % i["bm"]:
                c[("k1 FiLM", "band edge inside a tile")] += 1
            if not a.pre_elu and a.pre_scale == 1.0 and not a.ct:
                c[("k1 operand", "copy")] += 1
            if a.Yact:
                c[("k1 second output", i["base"])] += 1
        else:
            c[("r1 tile", (i["bm"], i["bn"]))] += 1
            c[("r1 instance", i["inst"])] += 1
    return c


def test_pw_dw_list_keeps_every_route():
    c = _pw_dw_routes(F.pw_dw_cases(), F.pw_dw_args)
    _report("pw_dw", c)
    for route in [("core", "k1"), ("core", "r1"), ("k1 window", 64), ("k1 window", 128), ("k1 tile height", 64), ("k1 tile height", 96),
                  ("k1 tile height", 128), ("k1 epilogue", "k5"), ("k1 epilogue", "k5 resid"), ("k1 epilogue", "generic"), ("k1 epilogue", "stride 2"),
                  ("k1 epilogue", "stride 4"), ("k1 epilogue", "stride 8"), ("k1 loader", 0), ("k1 loader", 1), ("k1 stages", 2), ("k1 stages", 3),
                  ("k1 operand", "copy"), ("k1 second output", "pw_dw"), ("k1 second output", "pw_dw_s"), ("k1 second output", "pw_dw_k5"),
                  ("k1 flat", "k5"), ("r1 instance", "generic"), ("r1 instance", "k5_nr"), ("r1 tile", (32, 64)), ("r1 tile", (32, 128)),
                  ("r1 tile", (128, 128))]:
        _need(c, route)
    # from PW_DW_EXPLICIT (one case is enough): the flat r = 8 stencil, the r = 5 epilogue, FiLM bands that end inside an m-tile, k5 with residual
    for route in [("k1 flat", "r8"), ("k1 epilogue", "stride 5"), ("k1 FiLM", "band edge inside a tile"), ("r1 instance", "k5"),
                  ("name", "pw_dw_k5<128,128,dma3>"), ("name", "pw_dw_k5<128,128,dma3,flat>"), ("name", "pw_dw_k5_nr<128,128,dma,flat>"),
                  ("name", "pw_dw_s<128,128,dma,flat>"), ("name", "pw_dw_k5<128,128,reg>"), ("r1 tile", (64, 64)), ("r1 tile", (128, 64))]:
        _need(c, route, 1)
    assert all(B * max(K, M) * T <= F.BOUND for B, K, M, T, *_ in F.pw_dw_cases())


def test_smallest_shapes_of_the_named_routes():
    """The shapes the routes are named by: K = 256 takes the three-stage pipeline at T = 124 (at T = 128 three 64-column tiles compute fewer
    columns than two 128-column ones), (B, C, T) = (7, 128, 36) is flat, the one-launch SpecBlock starts at 68 frames."""
    assert F.launch_pw_dw(F.pwdw(2, 256, 128, 124))[0] == "pw_dw_k5_nr<128,128,dma3>"
    assert F.launch_pw_dw(F.pwdw(2, 256, 128, 128))[0] == "pw_dw_k5_nr<128,64,dma>"
    assert F.launch_pw_dw(F.pwdw(7, 128, 128, 36))[0] == "pw_dw_k5_nr<128,128,dma,flat>"
    assert F.launch_pw_dw(F.pwdw(1, 128, 128, 36))[0] == "pw_dw_k5_nr<128,64,dma>"
    assert F.launch_stft_spec(64, 1, 68, 64) == "stft_spec<64,128,k1>" and F.launch_stft_spec(64, 1, 64, 64) is None
    assert F.launch_stft_spec(64, 1, 67, 64) is None and F.launch_stft_spec(128, 2, 136, 64) is None


def test_upsample_list_keeps_every_route():
    c = _pw_dw_routes(F.up_cases(), F.up_args)
    _report("upsample", c)
    for route in [("core", "k1"), ("core", "r1"), ("k1 loader", 2), ("k1 loader", 3), ("k1 loader", 5), ("k1 loader", 7),
                  ("k1 window", 64), ("k1 window", 128), ("r1 instance", "convtr4"), ("r1 instance", "convtr2"), ("r1 instance", "convtr1"),
                  ("r1 instance", "convtr0"), ("k1 flat", "convtr")]:
        _need(c, route)
    _need(c, ("k1 tile height", 256), 1)
    _need(c, ("k1 loader", 6), 1)                                 # UP_EXPLICIT
    _need(c, ("name", "convtr_pw_lds<64,64,win>"), 1)


def test_dw_pw_stft_and_block_lists_keep_every_route():
    c = collections.Counter(F.launch_dw_pw(M, T, 1, l2) for B, K, M, T, ks, l2 in F.convpost_cases())
    _report("conv_post", c)
    for name in ["dwconv_pw<64,64,2,2>", "dwconv_pw<128,64,2,2>"]:
        _need(c, name)
    assert sum(v for k, v in c.items() if k.endswith(",128,1,4>")) >= 2
    assert sum(1 for *_, l2 in F.convpost_cases() if l2) >= 2 and sum(1 for *_, l2 in F.convpost_cases() if not l2) >= 2
    c = collections.Counter(F.specadd_route(case)[0].split("<")[0] + ("/flat" if "flat" in F.specadd_route(case)[0] else "") for case in F.specadd_cases())
    c.update(F.specadd_route(case)[1]["core"] for case in F.specadd_cases())
    _report("SpecBlock add", c)
    for route in ["pw", "spec_add", "k1", "r1", "plain"]:
        _need(c, route)
    _need(c, "spec_add/flat", 1)
    c = collections.Counter()
    for B, n_fft, hop, T in F.stft_cases():
        name = F.launch_stft_logmag(n_fft, hop, T)
        c[name] += 1
        if name.endswith("k1>"):
            c["k1 with interior tiles" if F.stft_interior_tiles(n_fft, hop, T) else "k1 without interior tiles"] += 1
    _report("STFT", c)
    for name in ["stft_logmag<128,64,2,2>", "stft_logmag<64,128,1,4>", "stft_logmag<128,128,k1>", "stft_logmag<64,128,k1>", "k1 with interior tiles",
                 "k1 without interior tiles"]:
        _need(c, name)
    assert c["stft_logmag<96,128,1,4>"] + c["stft_logmag<128,128,1,4>"] >= 2
    c = collections.Counter(F.launch_stft_spec(n, hop, T, n) for B, n, hop, T in F.specblock_cases())
    _report("one-launch SpecBlock", c)
    _need(c, "stft_spec<64,128,k1>")
    _need(c, "stft_spec<128,128,k1>")
    c = collections.Counter()
    for B, C, T, outs in F.resblock_cases():
        assert F.rb_supported(C, T)
        g = F.rb_geometry(C)
        c[g["name"]] += 1
        c[outs] += 1
        c["one tile" if T <= g["TTO"] else "several tiles"] += 1
    _report("one-launch ResnetBlock", c)
    for route in ["resblock<64,252>", "resblock<96,244>", "resblock<128,252>", "resblock<192,124>", "raw", "act", "both", "one tile", "several tiles"]:
        _need(c, route)


def test_persistent_grid():
    """rb_launch / rh_launch: per_cu from the configurations, and the walk cases have three tiles per clip, more tiles than the cap, and a
    tile count that is no multiple of the grid."""
    assert [F.rb_geometry(C)["per_cu"] for C in (64, 96, 128, 192)] == [2, 1, 1, 1]
    assert [F.rb_geometry(C)["TTO"] for C in (64, 96, 128, 192)] == [244, 236, 244, 116]
    assert [F.rh_geometry(C)["per_cu"] for C in (64, 96, 128, 192)] == [2, 5, 2, 1]
    # the largest kernel-level case of the older tests never gives a workgroup a second tile
    assert F.persistent_grid(F.rb_geometry(192), 3, 8000, 256) == (207, 207)
    for cus in (256, 304, 64):
        for geo in [F.rb_geometry(C) for C in (64, 96, 128, 192)] + [F.rh_geometry(C) for C in (64, 96, 128, 192)]:
            B, T = F.persistent_walk_case(geo, cus)
            tiles, grid = F.persistent_grid(geo, B, T, cus)
            assert tiles == 3 * B and grid == cus * geo["per_cu"] and grid < tiles < 2 * grid + 3 * 3 and tiles % grid and T % 4 == 0, (geo, cus)


def _plan_routes(cases):
    c = collections.Counter()
    for idx, kw, T, B in cases:
        for generator in (True, False):
            plan = F.net_plan(F.net_cfg_dict(kw), B, T, generator)
            for r in plan["stages"]:
                for b in r["blocks"]:
                    c[(r["net"], "block", b["route"])] += 1
                    if b["route"] == "one":
                        c[("one-launch block", r["C"])] += 1
                    c[("block", "want_raw" if b["want_raw"] else "act alone", "next_scale" if b["next_scale"] else "no copy")] += 1
                if r["net"] == "enc":
                    c[("spec", r["spec"])] += 1
                    if r["spec"] == "one":
                        c[("one-launch SpecBlock", r["C"])] += 1
                    if "down_reads" in r:
                        c[("down reads", r["down_reads"])] += 1
                        c[("next_has_blocks", r["next_has_blocks"])] += 1
                    if r.get("stft_interior"):
                        c["STFT interior tiles"] += 1
                else:
                    c[("upsample writes", r["up_writes"], "blocks take the copy" if r["blocks_act"] else "")] += 1
                    c[("upsample", r["up"]["core"], r["up"].get("ldr", r["up"].get("inst")))] += 1
                if r["empty"] and not (r["net"] == "enc" and r["stage"] == len(kw["strides"])):
                    c[(r["net"], "empty block list")] += 1
    return c


def test_whole_net_list_reaches_every_plan_route():
    cases = F.net_cases()
    c = _plan_routes(cases)
    _report("whole nets", c)
    for route in [("enc", "block", "one"), ("enc", "block", "two_self"), ("enc", "block", "two_act"), ("dec", "block", "one"), ("dec", "block", "two_self"),
                  ("dec", "block", "two_act"), ("one-launch block", 64), ("one-launch block", 96), ("one-launch block", 128), ("one-launch block", 192),
                  ("spec", "one"), ("spec", "k1_add"), ("spec", "plain"), ("one-launch SpecBlock", 64), ("one-launch SpecBlock", 128),
                  ("down reads", "act"), ("next_has_blocks", True), ("next_has_blocks", False),
                  ("block", "want_raw", "next_scale"), ("block", "want_raw", "no copy"), ("block", "act alone", "next_scale"),
                  ("upsample writes", "Y", ""), ("upsample writes", "+Yact", ""), ("upsample writes", "Y+Yact", "blocks take the copy"),
                  ("enc", "empty block list"), ("dec", "empty block list"), "STFT interior tiles"]:
        _need(c, route)
    stage_channels = {r["C"] for idx, kw, T, B in cases for r in F.net_plan(F.net_cfg_dict(kw), B, T)["stages"]}
    assert {64, 96, 128, 192, 256, 384} <= stage_channels
    for idx, kw, T, B in cases:
        assert 1 <= B <= 3 and T <= 1300 and kw["residual_kernel_size"] in (3, 5) and kw["dilation_base"] in (1, 2)
    assert {kw["residual_kernel_size"] for _, kw, _, _ in cases} == {3, 5} and {kw["dilation_base"] for _, kw, _, _ in cases} == {1, 2}


# ---- what the older lists of tests/test_gpu_fuzz.py reach (on record; they stay as they are) -------------------------------------------------
def _old_pw_dw_args():
    from test_gpu_fuzz import _pw_dw_cases
    from test_gpu_ops import rnd
    out = []
    for K, M, Tin, ks, stride, dil, B in _pw_dw_cases(60, 2024):
        rng = np.random.default_rng(K * 131 + M * 17 + Tin + ks)                  # the draws of test_pw_dw_fuzz's body, in its order
        rnd(rng, B, K, Tin), rnd(rng, M, K, 1), rnd(rng, M, 1, ks), rnd(rng, M)
        pre_elu = bool(rng.integers(0, 2))
        pre = float(rng.uniform(0.5, 1.0))
        mode = int(rng.integers(0, 3))
        out.append(F.pwdw(B, K, M, Tin, ks=ks, stride=stride, dil=dil, pre_elu=pre_elu, pre_scale=pre, resid=mode == 1 and stride == 1,
                          film=mode == 2 and M % 4 == 0, bands=4 if mode == 2 and M % 4 == 0 else 1))
    return out


def test_what_the_old_pw_dw_fuzz_reaches():
    args = _old_pw_dw_args()
    routes = [F.launch_pw_dw(a) for a in args]
    k1 = [(a, i) for a, (_, i) in zip(args, routes) if i["core"] == "k1"]
    assert len(args) == 60 and len(k1) == 14
    assert sum(1 for a in args if a.M < 33 or a.Tin % 4) == 46
    k5 = [(a, i) for a, i in k1 if a.ks == 5 and a.stride == 1 and a.dil == 1]
    assert len(k5) == 2 and all(i["bn"] == 64 for _, i in k5)                      # two k5 stencils, both narrow-window; no wide k5
    assert not any(a.K >= 256 for a in args)                                      # no dma3
    assert not any(i["flat"] for _, i in k1) and not any(i["epi"] == 8 for _, i in k1)
    assert all(a.pre_scale != 1.0 for a in args) and not any(i["ldr"] == 0 for _, i in k1)   # the DMA'd operand is never taken
    assert not any(a.Yact for a in args)


def test_what_the_old_whole_net_fuzz_reaches():
    from test_gpu_fuzz import _net_cases
    beyond = {}
    for idx, kw, T, B in _net_cases(16, 99):
        c = _plan_routes([(idx, kw, T, B)])
        beyond[idx] = {k for k in c if k in {("enc", "block", "one"), ("dec", "block", "one"), ("spec", "k1_add"), ("spec", "one"), ("enc", "block", "two_act"),
                                             ("dec", "block", "two_act"), ("next_has_blocks", True)} or (isinstance(k, tuple) and k[0] == "one-launch block")}
    assert [i for i, b in beyond.items() if b] == [0]
    assert {k for k in beyond[0] if k[0] == "one-launch block"} == {("one-launch block", 96)} and ("spec", "k1_add") in beyond[0]
    assert not any(k[-1] == "two_act" or k == ("spec", "one") or k == ("next_has_blocks", True) for b in beyond.values() for k in b)


# ---- the float64 oracle is the float32 one ---------------------------------------------------------------------------------------------
def _tie(f64, f32, what, ulps=64):
    """float32 rounding of a short chain: a few dozen ulps of the tensor's magnitude."""
    assert f64.dtype == np.float64 and f32.dtype == np.float32, what
    lim = ulps * 2.0 ** -24 * float(np.abs(f64).max())
    assert float(np.abs(f64 - f32).max()) <= lim, (what, float(np.abs(f64 - f32).max()), lim)


def test_float64_oracle_agrees_with_the_float32_one():
    rng = np.random.default_rng(7)
    r = lambda *s, scale=1.0: (scale * rng.standard_normal(s)).astype(np.float32)
    D = np.float64
    x = r(2, 12, 37)
    _tie(O.elu(x, D), O.elu(x), "elu", 2)
    w, b = r(8, 12, 1, scale=12 ** -0.5), r(8)
    _tie(O.sconv1d(x, w, b, dtype=D), O.sconv1d(x, w, b), "sconv1d 1x1")
    wd, bd = r(12, 1, 4, scale=0.5), r(12)
    _tie(O.sconv1d(x, wd, bd, stride=2, groups=12, dtype=D), O.sconv1d(x, wd, bd, stride=2, groups=12), "sconv1d depth-wise")
    wk = r(8, 12, 3, scale=1 / 6)
    _tie(O.sconv1d(x, wk, b, dilation=2, dtype=D), O.sconv1d(x, wk, b, dilation=2), "sconv1d dense")
    wt = r(12, 1, 6, scale=0.4)
    _tie(O.sconvtr1d_depthwise(x, wt, 3, dtype=D), O.sconvtr1d_depthwise(x, wt, 3), "sconvtr1d_depthwise")
    wav = r(2, 1, 300, scale=0.1)
    _tie(O.causal_stft_mag(wav, 32, 3, dtype=D), O.causal_stft_mag(wav, 32, 3), "causal_stft_mag")
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict, synthetic_clips
    kw = dict(strides=[2, 3], channels_enc=8, channels_dec=4, dimension=8, n_fft_base=8, n_residual_enc=2, n_residual_dec=2, output_dim=4,
              embedding_dim=8, embedding_layers=2)
    cg = default_config("generator", **kw)
    sd = random_state_dict(cg, 5, parametrized=True)
    n32, n64 = O._Net(cg, sd), O._Net(cg, sd, D)
    xb = r(2, 8, 41)
    _tie(O.resnet_block(n64, "encoder.blocks.0.1", xb, 2, cg.res_scale_enc, [1, 1]), O.resnet_block(n32, "encoder.blocks.0.1", xb, 2, cg.res_scale_enc, [1, 1]),
         "resnet_block", 256)
    wv, msg = synthetic_clips(2, 41, seed=3)
    _tie(O.spec_block(n64, "encoder.spec_blocks.0", xb, wv, 8, 1, -4.0, 2.5, cg.res_scale_enc),
         O.spec_block(n32, "encoder.spec_blocks.0", xb, wv, 8, 1, -4.0, 2.5, cg.res_scale_enc), "spec_block", 256)
    e32, e64 = O.msg_embedding(n32, msg), O.msg_embedding(n64, msg)
    _tie(O.film_params(n64, e64), O.film_params(n32, e32), "film_params", 256)
    x, msg = synthetic_clips(2, 131, seed=4)
    _tie(O.encoder_forward(n64, x.astype(D), msg), O.encoder_forward(n32, x, msg), "encoder_forward", 1024)
    z = O.encoder_forward(n32, x, msg)
    _tie(O.decoder_forward(n64, z), O.decoder_forward(n32, z), "decoder_forward", 1024)
    _tie(O.generator_forward(cg, sd, x, msg, dtype=D), O.generator_forward(cg, sd, x, msg), "generator_forward", 1024)
    cd = default_config("detector", **{k: v for k, v in kw.items() if k not in ("channels_dec", "embedding_dim", "embedding_layers")})
    sdd = random_state_dict(cd, 6)
    d32, d64 = O._Net(cd, sdd), O._Net(cd, sdd, D)
    zz = r(2, 8, 22)
    _tie(O.head_forward(d64, zz, 130), O.head_forward(d32, zz, 130), "head_forward", 256)
    _tie(O.detector_forward(cd, sdd, x, dtype=D), O.detector_forward(cd, sdd, x), "detector_forward", 1024)


def test_float32_oracle_takes_its_operands_as_before():
    """The default dtype leaves the caller's arrays alone (float64 operands are still evaluated in float64 and then rounded, as before the
    functions took a dtype); tests/test_oracle_golden.py, unchanged, holds the float32 evaluation to the reference."""
    x = np.linspace(-2, 2, 24).reshape(1, 2, 12)
    w = np.linspace(-1, 1, 6).reshape(3, 2, 1)
    assert O._in(x, O.F32) is x and O._in(None, np.float64) is None
    assert np.array_equal(O.sconv1d(x, w, None), np.matmul(w[:, :, 0], x).astype(np.float32))
    assert O.elu(x).dtype == np.float32 and O.elu(x, np.float64).dtype == np.float64
