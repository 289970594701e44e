"""The case lists of the f16 mode's fuzz (tests/h16_fuzz_cases.py) keep every route and edge of the restated launch_conv16 and of the
persistent ResnetBlock kernel's walk: at least two cases each.  A launcher or generator change that empties a route fails here by the
route's name.  Also on record: which routes and edges the older lists of tests/test_gpu_h16.py and the f16 cases of tests/test_gpu_guard.py
reach (their parameter lists are imported as they stand), and the boundaries of the restatement.  No GPU, no library."""
import collections

import h16_fuzz_cases as H


def _need(counts, route, n=2):
    assert counts.get(route, 0) >= n, f"{route!r}: {counts.get(route, 0)} case(s), need {n}"


def _report(title, counts):
    print(f"\n{title}: " + ", ".join(f"{k}: {v}" for k, v in sorted(counts.items(), key=str)))


def _count(args_list):
    c = collections.Counter()
    for a in args_list:
        r = H.launch_conv16(a)
        assert r is not None, f"the launcher refuses {vars(a)}"
        c.update(H.conv16_edges(a, r[1]))
    return c


STAGED = [f"conv16s<{k},{f}>" for k in (8, 10, 16) for f in ("short", "long")]
GENERIC = ["conv16<1,4,flat>", "conv16<2,2,flat>", "conv16<4,1>", "conv16<2,2>", "conv16<1,4>"]
# every route and edge the fuzz is there for; the new lists reach each at least twice
WANTED = ([("route", r) for r in STAGED + GENERIC + ["conv16u<short>", "conv16u<long>"]] +
          [("staged Tout", (k, t)) for k in (8, 10, 16) for t in (64, 65)] + [("staged Tout", 128), ("staged Tout", 129)] +
          [("staged", "ragged last row block"), ("staged", "ragged last row block, FiLM band edge inside a block"),
           ("staged", "short: the last tile holds one clip"), ("staged steps", 1), ("staged steps", 2), ("staged steps", 3)] +
          [("staged FiLM", r) for r in STAGED] +
          [("ups Tin", t) for t in (1, 64, 65, 128, 129)] + [("ups row block", rb) for rb in (128, 192, 240, 256)] +
          [("ups", "short: the last tile holds one clip"), ("ups", "short: every tile holds two clips")] + [("ups steps", n) for n in (1, 2, 3, 4)] +
          [("generic FiLM", r) for r in GENERIC] + [("generic residual", r) for r in GENERIC] + [("generic up", r) for r in GENERIC] +
          [("generic taps and stride", r) for r in GENERIC] + [("generic up", "Kp % 32 != 0"), ("generic up", "96-row block")] +
          [("flat tile spans a clip boundary", "conv16<2,2,flat> FiLM"), ("flat tile spans a clip boundary", "conv16<1,4,flat> FiLM"),
           ("generic Tout", 511), ("generic Tout", 512), ("generic", "rows outside c8 (f32 output only)"),
           ("generic chunks", "below the ring"), ("generic chunks", "the ring"), ("generic chunks", "above the ring"), ("generic chunks", "zero-padded"),
           ("f32 output", "conv16"), ("f32 output", "conv16s"), ("outputs", "raw"), ("outputs", "+act"), ("outputs", "raw+act"), ("outputs", "")])


def _new_lists():
    return ([H.dense_args(c) for c in H.dense_cases() + H.DENSE_EXPLICIT], [H.up_args(c) for c in H.up_cases() + H.UP_EXPLICIT])


def test_new_lists_reach_every_route_and_edge():
    dense, up = _new_lists()
    c = _count(dense + up)
    _report("f16 fuzz, all four lists", c)
    for route in WANTED:
        _need(c, route)
    # the written-out lists alone (they also run between guard bands): every kernel instance and every placed edge
    w = _count([H.dense_args(c) for c in H.DENSE_EXPLICIT] + [H.up_args(c) for c in H.UP_EXPLICIT])
    _report("f16 fuzz, the written-out lists", w)
    for route in WANTED:
        if route[0] in ("route", "staged Tout", "ups Tin", "ups row block", "generic Tout", "staged FiLM", "flat tile spans a clip boundary") or \
                route in (("staged", "ragged last row block, FiLM band edge inside a block"), ("generic up", "Kp % 32 != 0"), ("generic up", "96-row block")):
            _need(w, route)
    for route in [("ups", "short: the last tile holds one clip"), ("staged", "short: the last tile holds one clip"), ("generic FiLM", "conv16<4,1>"),
                  ("generic FiLM", "conv16<2,2,flat>"), ("generic taps and stride", "conv16<4,1>")]:
        _need(w, route)


def test_the_draws_keep_their_spread():
    """The dense draw: 60 cases inside the size bound, B 1..7, every K of the recipe, at least a third off the flat route; the upsample
    draw: 24 cases, every ratio, odd and even B, the LDS kernel and the generic one both flat and per clip."""
    d = H.dense_cases()
    assert len(d) == 60 and all(B * max(K, M) * T <= H.BOUND for B, K, M, T, *_ in d)
    assert {c[0] for c in d} == set(range(1, 8)) and {c[1] for c in d} == {8, 16, 24, 32, 48, 64, 100, 144}
    routes = collections.Counter(H.launch_conv16(H.dense_args(c))[1]["route"] for c in d)
    _report("dense draw", routes)
    assert sum(v for k, v in routes.items() if not k.endswith("flat>")) * 3 >= len(d), routes
    assert {c[7] for c in d} == {"none", "resid", "film3", "film4"} and {c[8] for c in d} == {"raw", "act", "both", "all", "f32"}
    assert any(c[2] % 16 for c in d) and any(c[2] % 16 == 0 for c in d)
    u = H.up_cases()
    assert len(u) == 24 and {c[4] for c in u} == {2, 3, 4, 5, 8} and {c[0] % 2 for c in u} == {0, 1}
    routes = collections.Counter(H.launch_conv16(H.up_args(c))[1]["route"] for c in u)
    _report("upsample draw", routes)
    assert routes["conv16u<short>"] + routes["conv16u<long>"] >= 2
    assert sum(v for k, v in routes.items() if k.startswith("conv16<") and k.endswith("flat>")) >= 2
    assert sum(v for k, v in routes.items() if k.startswith("conv16<") and not k.endswith("flat>")) >= 2


# ---- the older lists, as they stand ---------------------------------------------------------------------------------------------------------
def _params(fn, names):
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise KeyError(names)


def _old_lists():
    """-> {family: [Conv16Args]} of tests/test_gpu_h16.py and of the f16 unit cases of tests/test_gpu_guard.py, and [(B, C, T)] of their blocks."""
    import test_gpu_guard as TG
    import test_gpu_h16 as T16
    fam = collections.defaultdict(list)
    for K, M, Tin, r in _params(T16.test_downsample_as_one_conv, "K,M,Tin,r"):
        fam["downsample"].append(H.conv16(3, K, M, Tin, 2 * r, r, r, Y=True, Yact=True, Yf32=True))
    for F, M, T in _params(T16.test_spec_add, "F,M,T"):
        fam["spec add"].append(H.conv16(3, F, M, T, resid=True, Y=True, Yact=True))
    for seed in _params(T16.test_conv16_generic_geometries, "seed"):
        _, B, K, ks, stride, pad, Tin, c8, M = T16._generic_geometry(seed)
        fam["sweep"].append(H.conv16(B, K, M, Tin, ks, stride, pad, resid=c8, Y=c8, Yact=c8, Yf32=True))
    for K, M, Tin, r in _params(T16.test_downsample_with_film, "K,M,Tin,r"):
        fam["film"].append(H.conv16(3, K, M, Tin, 2 * r, r, r, film=True, bands=4, Y=True, Yact=True))
    for K, M, Tin, r in _params(T16.test_upsample_as_one_conv, "K,M,Tin,r"):
        fam["upsample"].append(H.up16(2, K, M, Tin, r, Y=True, Yact=True))
    for K, M, Tin, r in _params(TG.test_h16_conv_film_guarded, "K,M,Tin,r"):
        fam["guard film"].append(H.conv16(2, K, M, Tin, 2 * r, r, r, film=True, bands=4, Y=True, Yact=True))
    for K, M, Tin, ks, stride, pad in _params(TG.test_h16_conv_guarded, "K,M,Tin,ks,stride,pad"):
        fam["guard conv"].append(H.conv16(2, K, M, Tin, ks, stride, pad, resid=True, Y=True, Yact=True, Yf32=True))
    for K, M, Tin, r in _params(TG.test_h16_upsample_guarded, "K,M,Tin,r"):
        fam["guard upsample"].append(H.up16(2, K, M, Tin, r, Y=True, Yact=True))
    blocks = [(3, C, T) for C, T in _params(T16.test_resblock, "C,T")]
    blocks += [(B, C, T) for _, C, T, B in (T16._random_block_shape(s) for s in _params(T16.test_resblock16_random_lengths, "seed"))]
    blocks += [(2, C, T) for C, T in _params(TG.test_h16_resblock_guarded, "C,T")]
    return fam, blocks


def test_what_the_older_lists_reach():
    """The gap this fuzz closes, as numbers.  The seeded sweep of the generic conv: 23 of 24 seeds flat, one <1,4> per clip.  Over all older
    unit lists: <4,1> once (the SpecBlock add, no taps), <2,2> per clip with taps twice; conv16s<16,long>, conv16s<8,short>, a ragged row
    block, a short upsample tile with one clip, the up form per clip or on <2,2,flat>, the Kp % 32 fall-through, FiLM on <4,1> or <1,4>,
    and every placed Tout / Tin edge but Tin = 1: never; FiLM on <2,2,flat> once."""
    fam, _ = _old_lists()
    sweep = collections.Counter(H.launch_conv16(a)[1]["route"] for a in fam["sweep"])
    _report("test_conv16_generic_geometries", sweep)
    assert sweep == {"conv16<1,4,flat>": 14, "conv16<2,2,flat>": 9, "conv16<1,4>": 1}
    c = _count([a for v in fam.values() for a in v])
    _report("older f16 unit lists", c)
    assert c[("route", "conv16<4,1>")] == 1 and c[("generic taps and stride", "conv16<4,1>")] == 0
    assert c[("generic taps and stride", "conv16<2,2>")] == 2 and c[("route", "conv16<2,2>")] == 3
    never = [("route", "conv16s<16,long>"), ("route", "conv16s<8,short>"), ("staged", "ragged last row block"), ("ups", "short: the last tile holds one clip"),
             ("generic up", "conv16<4,1>"), ("generic up", "conv16<2,2>"), ("generic up", "conv16<1,4>"), ("generic up", "conv16<2,2,flat>"),
             ("generic up", "Kp % 32 != 0"), ("generic FiLM", "conv16<4,1>"), ("generic FiLM", "conv16<1,4>"),
             ("staged steps", 1), ("staged steps", 2), ("ups steps", 1), ("ups steps", 2), ("ups steps", 3), ("ups row block", 128),
             ("generic Tout", 511), ("generic Tout", 512), ("staged Tout", 128), ("staged Tout", 129)] + \
            [("staged Tout", (k, t)) for k in (8, 10, 16) for t in (64, 65)] + [("ups Tin", t) for t in (64, 65, 128, 129)]
    for route in never:
        assert c[route] == 0, (route, c[route])
    assert c[("generic FiLM", "conv16<2,2,flat>")] == 1 and c[("generic up", "conv16<1,4,flat>")] == 2
    missed = [r for r in WANTED if c[r] < 2]
    print(f"\n{len(missed)} of {len(WANTED)} routes and edges have fewer than two older cases: {missed}")
    assert len(missed) >= len(never)


def test_older_blocks_never_walk_at_the_other_widths():
    """At C = 32 / 256 / 384 / 512 / 768 every older ResnetBlock case has no more tiles than rh_launch's grid at 256 CUs: no workgroup takes
    a second tile there (C = 64 .. 192 have the walk of tests/test_gpu_infer_fuzz.py)."""
    _, blocks = _old_lists()
    seen = collections.Counter()
    for B, C, T in blocks:
        if C in H.WALK_WIDTHS:
            tiles, grid = H.persistent_grid(H.rh_geometry(C), B, T, 256)
            assert tiles == grid, (B, C, T, tiles, grid)
            seen[C] += 1
    assert all(seen[C] >= 2 for C in H.WALK_WIDTHS), seen


# ---- the restatement's own boundaries ---------------------------------------------------------------------------------------------------------
def _route(a):
    r = H.launch_conv16(a)
    return None if r is None else r[1]["route"]


def test_length_boundaries():
    """64 | 65: the two-clip SHORT forms end at 64 outputs (staged) / 64 input frames (ups); 511 | 512: the flat run ends at 511 outputs."""
    for ks, s in ((8, 4), (10, 5), (16, 8)):
        assert _route(H.conv16(3, 16, 256, 64 * s, ks, s, s)) == f"conv16s<{ks},short>"
        assert _route(H.conv16(3, 16, 256, 64 * s + 1, ks, s, s)) == f"conv16s<{ks},long>"
    assert H.launch_conv16(H.conv16(3, 16, 256, 256, 8, 4, 4))[1]["grid"] == (2, 1)            # three clips in two two-clip tiles
    assert H.launch_conv16(H.conv16(3, 16, 320, 260, 8, 4, 4))[1]["grid"] == (3, 2)            # 65 outputs: one tile per clip, a ragged second row block
    assert H.launch_conv16(H.conv16(2, 32, 256, 1032, 16, 8, 8))[1]["grid"] == (4, 1)          # 129 outputs: two column tiles per clip
    assert _route(H.up16(3, 32, 32, 64, 8)) == "conv16u<short>" and _route(H.up16(3, 32, 32, 65, 8)) == "conv16u<long>"
    assert H.launch_conv16(H.up16(3, 32, 32, 64, 8))[1]["grid"] == (2, 1) and H.launch_conv16(H.up16(3, 32, 32, 129, 8))[1]["grid"] == (6, 1)
    for M, f, p in ((64, "conv16<1,4,flat>", "conv16<1,4>"), (128, "conv16<2,2,flat>", "conv16<2,2>"), (320, "conv16<2,2,flat>", "conv16<4,1>")):
        assert _route(H.conv16(2, 16, M, 511, 5, 1, 4)) == f and _route(H.conv16(2, 16, M, 512, 5, 1, 4)) == p
    assert H.launch_conv16(H.conv16(2, 16, 128, 511, 5, 1, 4))[1]["grid"] == (8 * 1, 1)        # 1022 flat columns in 128-column tiles
    assert H.launch_conv16(H.conv16(2, 16, 128, 512, 5, 1, 4))[1]["grid"] == (2 * 4, 1)


def test_row_boundaries():
    """M = 127 | 128 | 255 | 256 | 511 | 512: flat stacks two waves from 128 rows and none again from 512; per clip two from 128, four from
    256; the staged kernel starts at 256."""
    flat = {M: _route(H.conv16(2, 16, M, 100, 3, 1, 2, Y=False, Yf32=True)) for M in (127, 128, 255, 256, 511, 512)}
    assert flat == {127: "conv16<1,4,flat>", 128: "conv16<2,2,flat>", 255: "conv16<2,2,flat>", 256: "conv16<2,2,flat>", 511: "conv16<2,2,flat>",
                    512: "conv16<1,4,flat>"}
    clip = {M: _route(H.conv16(2, 16, M, 600, 3, 1, 2, Y=False, Yf32=True)) for M in (127, 128, 255, 256, 511, 512)}
    assert clip == {127: "conv16<1,4>", 128: "conv16<2,2>", 255: "conv16<2,2>", 256: "conv16<4,1>", 511: "conv16<4,1>", 512: "conv16<4,1>"}
    for Tin in (200, 2400):
        assert _route(H.conv16(2, 16, 255, Tin, 8, 4, 4, Y=False, Yf32=True)).startswith("conv16<")
        assert _route(H.conv16(2, 16, 256, Tin, 8, 4, 4, Y=False, Yf32=True)).startswith("conv16s<8,")
    assert _route(H.conv16(2, 16, 256, 200, 8, 4, 4, resid=True)) == "conv16<2,2,flat>"          # a residual, other taps or another pad: generic
    assert _route(H.conv16(2, 16, 256, 200, 8, 4, 3)) == "conv16<2,2,flat>" and _route(H.conv16(2, 16, 256, 200, 4, 2, 2)) == "conv16<2,2,flat>"


def test_upsample_row_block_boundaries():
    """up * up_mb = 120 | 128 | 256 | 264: the LDS kernel takes row blocks of 128 .. 256 rows; up16_block never offers more than 256."""
    def with_block(Mo, r, mb):
        a = H.up16(2, 32, Mo, 100, r)
        a.up_mb = mb
        return _route(a)
    assert with_block(48, 5, 24) == "conv16<2,2,flat>"                                            # 120 rows
    assert with_block(16, 8, 16) == "conv16u<long>" and with_block(32, 8, 32) == "conv16u<long>"  # 128, 256
    assert with_block(176, 3, 88) == "conv16<1,4,flat>"                                           # 264 rows (M = 528: one wave row per workgroup)
    assert with_block(32, 8, 4) == "conv16<2,2,flat>" and with_block(32, 8, 6) is None           # up_mb % 8 != 0: generic; % 4 != 0: refused
    assert [H.up16_block(Mo, r) for Mo, r in ((32, 8), (48, 5), (16, 8), (64, 2), (96, 2), (32, 3), (96, 3), (48, 8), (24, 16), (20, 2))] == \
        [32, 48, 16, 64, 96, 32, 48, 24, 8, 0]
    for Mo, r in ((32, 8), (48, 5), (16, 8), (64, 2), (96, 2)):
        assert _route(H.up16(2, 32, Mo, 100, r)) == "conv16u<long>" and _route(H.up16(2, 48, Mo, 100, r)).startswith("conv16<")   # Kp = 48
    assert _route(H.up16(2, 32, 32, 100, 3)) == "conv16<1,4,flat>" and _route(H.up16(2, 32, 24, 100, 2)) is None                # 96 rows; Mo % 16


def test_packers_names_and_refusals():
    w = H.pack_h16(33, 100, 5)
    assert (w.Kp, w.Mp, w.nchunks) == (112, 64, 40)
    assert H.pack_h16(16, 8, 1).nchunks == 8 and H.pack_h16(16, 16, 8).nchunks == 8 and H.pack_h16(16, 24, 5).nchunks == 16
    u = H.pack_up16(48, 100, 5)
    assert (u.M, u.Kp, u.Mp, u.nchunks) == (240, 112, 256, 16)
    assert H.launch_conv16(H.conv16(3, 128, 256, 501, 8, 4, 4, film=True, bands=4))[0] == "conv16<k8,s4,256x128,lds>"
    assert H.launch_conv16(H.conv16(3, 33, 64, 77, resid=True))[0] == "conv16<k1,s1,64x33,flat>"
    assert H.launch_conv16(H.conv16(3, 64, 128, 16000, 4, 2, 2))[0] == "conv16<k4,s2,128x64>"
    assert H.launch_conv16(H.up16(2, 1536, 768, 50, 8))[0] == "conv16<k2,s1,6144x1536,up8,lds>"
    assert H.launch_conv16(H.up16(2, 64, 32, 37, 3))[0] == "conv16<k2,s1,96x64,up3,flat>"
    assert H.launch_conv16(H.conv16(2, 16, 33, 100)) is None and H.launch_conv16(H.conv16(2, 16, 33, 100, Y=False, Yf32=True)) is not None   # c8 outputs need M % 16
    assert H.launch_conv16(H.conv16(2, 16, 48, 100, film=True, bands=5)) is None and H.launch_conv16(H.conv16(2, 16, 40, 100, Y=False, Yf32=True, film=True, bands=5)) is not None
    assert H.launch_conv16(H.conv16(2, 16, 24, 100, Y=False, Yf32=True, film=True, bands=4)) is None                                      # 6-row bands
    assert H.launch_conv16(H.conv16(1, 16, 16, 0x7f000000 // 32)) is None


def test_resblock16_rows_and_walk():
    """The RH<...> rows of launch_resblock16, rh_launch's workgroups per CU, and the three walk conditions at every width and CU count."""
    import infer_fuzz_cases as F
    rows = {C: H.rh_geometry(C) for C in F.RH_CFG}
    assert [C for C in range(8, 1025, 8) if H.rh16_width(C)] == [32, 64, 96, 128, 192, 256, 384, 512, 768]
    assert {C: (g["TTO"], g["SMEM"], g["waves"], g["per_cu"]) for C, g in rows.items()} == {
        32: (476, 32512, 8, 2), 64: (236, 34304, 8, 2), 96: (56, 16896, 3, 5), 128: (116, 37888, 8, 2), 192: (116, 56832, 12, 1),
        256: (56, 45056, 8, 2), 384: (56, 67584, 12, 1), 512: (56, 90112, 16, 1), 768: (56, 135168, 12, 1)}
    assert [H.persistent_walk_case(rows[C], 256) for C in H.WALK_WIDTHS] == [(172, 972), (172, 132), (87, 132), (87, 132), (87, 132)]
    for cus in (256, 304, 64, 8):
        for C in F.RH_CFG:
            B, T = H.persistent_walk_case(rows[C], cus)
            tiles, grid = H.persistent_grid(rows[C], B, T, cus)
            assert tiles == 3 * B and tiles > cus * rows[C]["per_cu"] == grid and tiles % grid, (C, cus, B, T, tiles, grid)
            assert B * C * T * 2 <= 24e6 * max(1, cus / 256)
