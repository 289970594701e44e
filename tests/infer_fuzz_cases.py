"""Seeded case lists of the exact-inference geometry fuzz (tests/test_gpu_infer_fuzz.py), and next to them a short Python restatement of
the shape dispatch of the exact f32 path: launch_pw_dw / launch_k1 / launch_dw_pw / the STFT launchers (csrc/wv_kernels.hip,
csrc/wv_k1.hip), launch_resblock (csrc/wv_rb.hip), the grid of the two persistent block kernels, and the launch plan of run_encoder /
wv_generator_forward / run_resblock (csrc/wv_model.hip).  Every restated launcher returns the kernel name wv::prof records, so the GPU
test can hold the restatement to the library; tests/test_infer_fuzz_cases_cpu.py asserts on the lists that every route keeps its cases.
A changed launcher is restated here.  Operands are taken as 16-byte aligned (fresh torch allocations).  Pure Python: no GPU, no library."""
from math import gcd
from types import SimpleNamespace

import numpy as np

OOB_VOFF = 0x40000000


def _tdiv(a, b):
    """C++ integer division (towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _cdiv(a, b):
    return -(-a // b)


def _best_bm(M):
    """The K1 tile height that pads M least, 128 on a tie."""
    bm, best = 128, _cdiv(M, 128) * 128
    for cand in (96, 64):
        if _cdiv(M, cand) * cand < best:
            best, bm = _cdiv(M, cand) * cand, cand
    return bm


# ---- pw_dw: 1x1 -> depth-wise stencil (and the upsample / SpecBlock-add forms that run on it) ----------------------------------------
def pwdw(B, K, M, Tin, ks=5, stride=1, dil=1, pre_elu=False, pre_scale=1.0, resid=False, film=False, bands=1, Y=True, Yact=False,
         ratio=0, spec_add=False):
    """PwDwArgs as wv_op_pw_dw / wv_op_dw_pw / the model fill them.  ratio > 0: the upsample unit (ConvTranspose producer, identity k5)."""
    a = SimpleNamespace(B=B, K=K, M=M, Tin=Tin, ks=ks, stride=stride, dil=dil, pre_elu=bool(pre_elu), pre_scale=float(np.float32(pre_scale)),
                        resid=bool(resid), film=bool(film), bands=bands, Y=bool(Y), Yact=bool(Yact), ct=ratio > 0, ratio=ratio,
                        spec_add=bool(spec_add))
    a.Tout = Tin * ratio if a.ct else _cdiv(Tin, stride)
    a.pad = (ks - 1) * dil - (stride - 1)
    return a


def pw_dw_geometry(a, BN):
    """-> (ok, tto, off): outputs per time tile and the stencil offset that puts every tile's window on a multiple of 4 samples."""
    span = (a.ks - 1) * a.dil + 1
    off = (4 - a.pad % 4) % 4
    tto = _tdiv(BN - off - span, a.stride) + 1
    q = 4 // gcd(a.stride, 4)
    tto -= tto - q * _tdiv(tto, q)
    if tto < 1:
        off = 0
        tto = _tdiv(BN - span, a.stride) + 1
    return tto >= 1, tto, off


def _narrow_by_columns(a):
    ok128, t128, _ = pw_dw_geometry(a, 128)
    ok64, t64, _ = pw_dw_geometry(a, 64)
    return ok128 and ok64 and _cdiv(a.Tout, t64) * 64 * 100 < _cdiv(a.Tout, t128) * 128 * 95


def k1_supported(a):
    if a.M < 33 or ((a.Tout if a.ct else a.Tin) & 3) or a.K < 1:
        return False
    if a.K * a.Tin * 4 >= OOB_VOFF or a.M * a.Tout * 4 >= OOB_VOFF:
        return False
    if a.ks < 1 or a.ks > 16 or (a.ks - 1) * a.dil + 1 + 3 > 64:
        return False
    return not (a.ct and a.ratio == 1)


LOADERS = {0: "dma", 1: "reg", 2: "reg", 3: "reg", 5: "reg", 6: "win", 7: "win"}


def _k1_name(a, bm, bn, base, epi, ldr, stages, flat):
    name = f"{base}<{bm},{bn},{'dma3' if ldr == 0 and stages == 3 else LOADERS[ldr]}{',flat' if flat else ''}>"
    return name, dict(core="k1", bm=bm, bn=bn, epi=epi, ldr=ldr, stages=stages, flat=flat, base=base)


def _k1_pick_ldr(a, bm, nt, epi, res, flat):
    bn, bkc = 32 * nt, (16 if nt == 4 else 32)
    if a.ct:
        assert epi == 0 and not res
        if not flat and a.pre_scale == 1.0 and not a.pre_elu and a.K % bkc == 0 and a.Tin % 4 == 0 and bm <= 128:
            if a.ratio % 4 == 0:
                return _k1_name(a, bm, bn, "convtr_pw_lds", 0, 6, 2, flat)
            if a.ratio == 2:
                return _k1_name(a, bm, bn, "convtr_pw_lds", 0, 7, 2, flat)
        return _k1_name(a, bm, bn, "convtr_pw", 0, 2 if a.ratio % 4 == 0 else 3 if a.ratio == 2 else 5, 2, flat)
    base = "spec_add" if a.spec_add else (("pw_dw_k5" if res else "pw_dw_k5_nr") if epi == 0 else "pw_dw" if epi == 1 else "pw_dw_s")
    if a.pre_elu or a.pre_scale != 1.0:
        return _k1_name(a, bm, bn, base, epi, 1, 2, flat)
    if nt == 4 and bm == 128 and epi == 0 and a.K >= 256:
        return _k1_name(a, bm, bn, base, epi, 0, 3, flat)
    return _k1_name(a, bm, bn, base, epi, 0, 2, flat)


def _k1_pick_epi(a, bm, nt, k5, tto, off, flat):
    """k1_pick_epi: 0 = the k5 DPP epilogue, 2 / 4 / 8 / 5 = the net's downsample stencils, 1 = generic."""
    if k5:
        return _k1_pick_ldr(a, bm, nt, 0, a.resid, flat)
    if nt == 4 and not a.resid and not a.ct and a.dil == 1:
        if a.ks == 2 * a.stride and a.pad == a.stride and off == (2 if a.stride == 2 else 0) and a.stride in (2, 4, 8):
            return _k1_pick_ldr(a, bm, nt, a.stride, False, flat)
        if a.ks == 10 and a.stride == 5 and tto <= 32:
            return _k1_pick_ldr(a, bm, nt, 5, False, flat)
    return _k1_pick_ldr(a, bm, nt, 1, a.resid, flat)


def launch_k1(a):
    """-> (name, info) or None (hipErrorNotSupported: the round-1 core takes the launch)."""
    k5 = a.ks == 5 and a.stride == 1 and a.dil == 1 and a.pad == 4 and not a.film
    narrow = (a.Tout if a.ct else a.Tin) + a.pad + 3 <= 64
    if not narrow and _narrow_by_columns(a):
        narrow = True
    flat = False
    if k5 and a.B > 1 and a.Tout % 4 == 0:                       # flat (clip, time) tiles of the k5 stencil: >= 2 % fewer columns
        bm = _best_bm(a.M)
        flat_cols = _cdiv(a.B * (a.Tout + 4) - 4, 124) * 128
        bn = 64 if narrow else 128
        ok, tto, _ = pw_dw_geometry(a, bn)
        clip_cols = a.B * _cdiv(a.Tout, tto) * bn if ok else -1
        if a.M % bm == 0 and a.B * a.M * a.Tout * 4 < 0x7fffffff and clip_cols > 0 and flat_cols * 100 < clip_cols * 98:
            flat, narrow = True, False
    ok, tto, off = pw_dw_geometry(a, 64 if narrow else 128)
    if not ok:
        return None
    if (not narrow and not flat and not a.resid and not a.ct and a.ks == 16 and a.stride == 8 and a.dil == 1 and a.pad == 8 and off == 0 and
            a.B > 1 and a.Tin % 8 == 0 and a.Tout * 8 == a.Tin and a.M % 128 == 0 and (not a.film or (a.M // a.bands) % 128 == 0) and
            not a.pre_elu and a.pre_scale == 1.0 and a.B * a.M * a.Tout * 4 < 0x7fffffff and a.B * a.K * a.Tin * 4 < 0x7fffffff):
        if _cdiv(a.B * ((a.Tin + 8) // 8), tto) * 100 < a.B * _cdiv(a.Tout, tto) * 98:      # the r = 8 stencil over the flat input axis
            flat = True
    if (tto * a.stride) % 4 or (a.pad + off) % 4:
        return None
    bm = _best_bm(a.M)
    if narrow:
        return _k1_pick_epi(a, bm, 2, k5, tto, off, flat)
    if a.ct and k5 and not a.resid and a.M % 256 == 0:
        return _k1_pick_ldr(a, 256, 4, 0, False, flat)
    return _k1_pick_epi(a, bm, 4, k5, tto, off, flat)


def pick_bm(M):
    if M <= 32:
        return 32
    if M <= 64:
        return 64
    if M <= 96:
        return 96
    if M % 128 == 0:
        return 128
    if M == 192:
        return 64
    return 96 if M % 96 == 0 else 128


def launch_pw_dw(a):
    """-> (kernel name as wv::prof records it, info).  info["core"]: "k1" (the LDS-DMA core) or "r1" (the round-1 core)."""
    if k1_supported(a):
        r = launch_k1(a)
        if r is not None:
            return r
    need = (a.ks - 1) * a.dil + 1
    narrow = a.Tin + a.pad + 3 <= 64 and need + 3 <= 64
    if not narrow and need + 3 <= 64 and _narrow_by_columns(a):
        narrow = True
    bm, bn = pick_bm(a.M), 64 if narrow else 128
    assert pw_dw_geometry(a, bn)[0], "the round-1 core refuses this stencil (hipErrorInvalidValue)"
    ks5 = a.ks == 5 and a.stride == 1 and a.dil == 1 and a.pad == 4
    if ks5 and a.ct:
        base, inst = "convtr_pw", f"convtr{4 if a.ratio % 4 == 0 else a.ratio if a.ratio in (1, 2) else 0}"
    elif ks5 and a.spec_add and a.resid:
        base, inst = "spec_add", "spec_add"
    elif ks5 and not a.resid:
        base, inst = "pw_dw_k5_nr", "k5_nr"
    else:
        base, inst = ("pw_dw_k5", "k5") if ks5 else ("pw_dw", "generic")
    return f"{base}<{bm},{bn},{bm // 32},1>", dict(core="r1", bm=bm, bn=bn, inst=inst, base=base)


def launch_dw_pw(M, Tout, mode, l2norm=False):
    """The plain 1x1 kernel (mode 0) and conv_post's depth-wise -> 1x1 (mode 1) -> kernel name."""
    bm = pick_bm(M)
    if l2norm:
        bm = 64 if M <= 64 else 128
    base = "pw" if mode == 0 else "dwconv_pw"
    if Tout <= 64:
        return f"{base}<{64 if bm <= 64 else 128},64,2,2>"
    return f"{base}<{bm},128,1,4>"


def op_dw_pw_route(B, K, M, Tin, mode, ratio=0, pre_elu=False, pre_scale=1.0, l2norm=False, accumulate=False, bias=True, Yact=False):
    """wv_op_dw_pw: the upsample and the SpecBlock add (M >= 128, no bias) run on pw_dw, the rest on the plain kernels."""
    if mode == 2:
        return launch_pw_dw(pwdw(B, K, M, Tin, pre_elu=pre_elu, pre_scale=pre_scale, Yact=Yact, ratio=ratio))
    if mode == 0 and accumulate and not l2norm and not bias and M >= 128:
        return launch_pw_dw(pwdw(B, K, M, Tin, pre_elu=pre_elu, pre_scale=pre_scale, resid=True, Yact=Yact, spec_add=True))
    return launch_dw_pw(M, Tin, mode, l2norm), dict(core="plain")


# ---- STFT ------------------------------------------------------------------------------------------------------------------------------
def stft_interior_tiles(n_fft, hop, T):
    """Tiles of stft_k1_kernel that take the `interior` fast path (every sample of the 128-frame window exists)."""
    Tf = _cdiv(T, hop)
    if n_fft % 16:
        return 0
    return sum(1 for t0 in range(0, Tf, 128) if t0 + 128 <= Tf and t0 * hop - (n_fft - 1) >= 0 and (t0 + 127) * hop < T)


def launch_stft_logmag(n_fft, hop, T):
    Tf = _cdiv(T, hop)
    F = n_fft // 2 + 1
    if F * Tf * 4 < OOB_VOFF and Tf > 64 and Tf % 4 == 0:
        return f"stft_logmag<{_best_bm(n_fft)},128,k1>"
    if Tf <= 64:
        return "stft_logmag<128,64,2,2>"
    if n_fft <= 64:
        return "stft_logmag<64,128,1,4>"
    return "stft_logmag<96,128,1,4>" if _cdiv(n_fft, 96) * 96 < _cdiv(n_fft, 128) * 128 else "stft_logmag<128,128,1,4>"


def launch_stft_spec(n_fft, hop, T, M):
    """The whole SpecBlock in one launch -> name, or None (hipErrorNotSupported: STFT + add)."""
    Tf = _cdiv(T, hop)
    if n_fft != M or n_fft not in (64, 128) or Tf <= 64 or Tf & 3 or M * Tf * 4 >= OOB_VOFF:
        return None
    return f"stft_spec<{n_fft},128,k1>"


# ---- the one-launch ResnetBlock and the persistent grids -------------------------------------------------------------------------------
# <C>: (NG, NT, WPS) of RB_CFG* (wv_rb.hip) and of the RH<> instances launch_resblock16 picks (wv_h16.hip)
RB_CFG = {64: (2, 4, 2), 96: (4, 2, 3), 128: (2, 4, 2), 192: (2, 2, 3)}
RH_CFG = {32: (8, 2, 4, 1), 64: (4, 2, 4, 1), 96: (1, 2, 4, 1), 128: (2, 2, 4, 1), 192: (2, 2, 3, 1), 256: (1, 2, 4, 1), 384: (1, 2, 3, 1),
          512: (1, 2, 4, 1), 768: (1, 2, 3, 2)}


def rb_geometry(C):
    """-> dict(WD, TTO, per_cu, name) of rb_kernel at C channels."""
    NG, NT, WPS = RB_CFG[C]
    WD = NG * (32 * NT - 4) + 4
    smem = (C * WD + 2 * C * 8) * 4
    nwaves = C // 32 * NG
    return dict(WD=WD, TTO=WD - 8, per_cu=max(1, min(160 * 1024 // smem, 4 * WPS // nwaves)), name=f"resblock<{C},{WD}>")


def rh16_width(C):
    """rh16_width (wv_kernels.h): the widths rh_kernel is built for, one RH<> row each in launch_resblock16's switch."""
    return C in RH_CFG


def rh_geometry(C):
    """-> dict(WD, TTO, SMEM, waves, per_cu, name) of the f16 rh_kernel at C channels: the RH<...> row and rh_launch's workgroups per CU."""
    NG, NT, WPS, SPW = RH_CFG[C]
    WD = NG * (32 * NT - 4) + 4
    smem = C // 8 * WD * 16 + 2 * (C // 2 * 12) * 4
    nwaves = C // (32 * SPW) * NG
    return dict(WD=WD, TTO=WD - 8, SMEM=smem, waves=nwaves, per_cu=max(1, min(160 * 1024 // smem, 4 * WPS // nwaves)), name=f"resblock16<{C},{WD}>")


def persistent_grid(geo, B, T, cus):
    """rb_launch / rh_launch -> (tiles, grid): a workgroup walks tile += grid."""
    tiles = _cdiv(T, geo["TTO"]) * B
    return tiles, min(tiles, cus * geo["per_cu"])


def rb_supported(C, T):
    return C in RB_CFG and T >= 4 and T % 4 == 0 and C * T * 4 < 0x7f000000


def persistent_walk_case(geo, cus):
    """The smallest (B, T) with three tiles per clip, more tiles than the grid cap and a tile count that is no multiple of the grid."""
    T = 2 * geo["TTO"] + 20
    B = cus * geo["per_cu"] // 3 + 2
    while (3 * B) % (cus * geo["per_cu"]) == 0:
        B += 1
    return B, T


# ---- the launch plan of the nets -------------------------------------------------------------------------------------------------------
def fused_block(cfg, C, T):
    return C in (64, 96, 128, 192) and cfg["residual_kernel_size"] == 5 and cfg["dilation_base"] == 1 and T % 4 == 0 and C * T * 4 < 0x7f000000


def wants_act_copy(cfg, C, T):
    return C >= 129 and not fused_block(cfg, C, T)


def _run_resblock(plan, cfg, st, C, T, B, dil1, want_raw, next_on, role):
    """run_resblock -> route: "one" (one launch), "two_self" (two launches, the first activates x itself), "two_act" (fed by a copy)."""
    ks = cfg["residual_kernel_size"]
    if st["raw"] and ks == 5 and dil1 == 1 and rb_supported(C, T):
        plan["launches"].append((role, rb_geometry(C)["name"]))
        st["raw"], st["act"] = want_raw, next_on
        return "one"
    route = "two_act" if st["act"] else "two_self"
    a = pwdw(B, C, C, T, ks=ks, dil=dil1, pre_elu=not st["act"], pre_scale=1.0 if st["act"] else 0.9, Y=False, Yact=True)
    b = pwdw(B, C, C, T, ks=ks, resid=True, Y=want_raw, Yact=next_on)
    plan["launches"] += [(role, launch_pw_dw(a)[0]), (role, launch_pw_dw(b)[0])]
    st["raw"], st["act"] = want_raw, next_on
    return route


def net_plan(cfg, B, T, generator=True):
    """run_encoder (+ the decoder of wv_generator_forward) -> dict(launches=[(role, kernel)], stages=[per-stage record]).
    cfg: dict of the NetConfig fields the plan reads.  A block's pre_scale is never 1 (idx >= 1 in the encoder; the decoder's idx = 0
    block has pre_scale 1 and is restated as such)."""
    plan = dict(launches=[], stages=[])
    strides = list(cfg["strides"])
    S = len(strides)
    ratios = strides[::-1]
    nre, nrd = cfg["n_residual_enc"], cfg["n_residual_dec"]
    C, Tl = cfg["channels_enc"], T
    if generator:
        plan["launches"].append(("enc.film", "film"))
    st = dict(raw=True, act=nre > 0 and wants_act_copy(cfg, C, T))
    plan["launches"].append(("enc.conv_pre", "conv_pre"))
    mult, hop = 1, 1
    for s in range(S + 1):
        post = s == S
        rec = dict(net="enc", stage=s, C=C, T=Tl, blocks=[], empty=nre == 0 or post)
        if not post:
            for j in range(1, nre + 1):
                last = j == nre
                nxt = not (last or not wants_act_copy(cfg, C, Tl))
                route = _run_resblock(plan, cfg, st, C, Tl, B, cfg["dilation_base"] ** j, True, nxt, "enc.resblock")
                rec["blocks"].append(dict(route=route, want_raw=True, next_scale=nxt))
        n_fft = mult * cfg["n_fft_base"]
        F = n_fft // 2 + 1
        fused = launch_stft_spec(n_fft, hop, T, C)
        if fused:
            plan["launches"].append(("enc.spec", fused))
            rec["spec"] = "one"
            if not post:
                st["raw"], st["act"] = False, True
        else:
            stft = launch_stft_logmag(n_fft, hop, T)
            plan["launches"].append(("enc.spec", stft))
            rec["stft"], rec["stft_interior"] = stft, stft_interior_tiles(n_fft, hop, T) if stft.endswith("k1>") else 0
            if C < 33 or Tl & 3:
                plan["launches"].append(("enc.spec", launch_dw_pw(C, Tl, 0)))
                rec["spec"] = "plain"
                st["act"] = not post
            else:
                acc = pwdw(B, F, C, Tl, resid=True, Y=post, Yact=not post, spec_add=True)
                nm, info = launch_pw_dw(acc)
                plan["launches"].append(("enc.spec", nm))
                rec["spec"] = "k1_add" if info["core"] == "k1" else "r1_add"
                if not post:
                    st["raw"], st["act"] = False, True
        if post:
            plan["stages"].append(rec)
            break
        r = ratios[s]
        rec["down_reads"] = "act" if st["act"] else "raw"
        Tn = _cdiv(Tl, r)
        nhb = s + 1 < S and nre > 0 and wants_act_copy(cfg, 2 * C, Tn)
        rec["next_has_blocks"] = nhb
        d = pwdw(B, C, 2 * C, Tl, ks=2 * r, stride=r, pre_elu=not st["act"], pre_scale=1.0 if st["act"] else 0.9, film=generator,
                 bands=cfg.get("freq_bands", 4), Yact=nhb)
        plan["launches"].append(("enc.down_film" if generator else "enc.down", launch_pw_dw(d)[0]))
        st["raw"], st["act"] = True, nhb
        Tl, C, mult, hop = Tn, 2 * C, 2 * mult, hop * r
        plan["stages"].append(rec)
    plan["launches"].append(("enc.conv_post", launch_dw_pw(cfg["dimension"], Tl, 1, l2norm=True)))
    if not generator:
        plan["launches"].append(("head", "head<64,64,2,2>"))
        return plan
    Cd = cfg["channels_dec"] * 2 ** S
    h = pwdw(B, cfg["dimension"], Cd, Tl, ks=cfg["kernel_size"], Y=False, Yact=True)
    plan["launches"].append(("dec.head", launch_pw_dw(h)[0]))
    st = dict(raw=False, act=True)
    for i, r in enumerate(strides):
        last_up = i + 1 == S
        M = Cd // 2
        has_blocks = nrd > 0
        blocks_act = has_blocks and wants_act_copy(cfg, M, Tl * r)
        yact = blocks_act if has_blocks else not last_up
        u = pwdw(B, Cd, M, Tl, Y=has_blocks or last_up, Yact=yact, ratio=r)
        nm, info = launch_pw_dw(u)
        plan["launches"].append(("dec.upsample", nm))
        st["raw"], st["act"] = has_blocks or last_up, yact
        Tl *= r
        rec = dict(net="dec", stage=i, C=M, T=Tl, blocks=[], empty=not has_blocks, up=info, up_writes=("Y" if u.Y else "") + ("+Yact" if yact else ""),
                   blocks_act=blocks_act)
        for j in range(nrd):
            last = j + 1 == nrd
            nxt = (not last_up) if last else wants_act_copy(cfg, M, Tl)
            want_raw = not last or last_up
            route = _run_resblock(plan, cfg, st, M, Tl, B, cfg["dilation_base"] ** j, want_raw, nxt, "dec.resblock")
            rec["blocks"].append(dict(route=route, want_raw=want_raw, next_scale=nxt))
        plan["stages"].append(rec)
        Cd = M
    plan["launches"].append(("dec.tail", "tail"))
    return plan


# ---- generators ------------------------------------------------------------------------------------------------------------------------
BOUND = 6e6                                                       # B * max(K, M) * T: keeps a case's float64 oracle in the low seconds

# (B, K, M, Tin, ks, stride, dil, pre, epi, act): pre in "elu" (scale -> ELU in the loader), "scale" (scale alone), "copy" (pre_elu = 0,
# pre_scale = 1: the DMA'd operand); epi in "none", "resid", "film4", "film3" (3 bands: M / bands is no multiple of the tile height).
# The forms a plain draw under the size bound rarely reaches, at the smallest shapes that have them:
PW_DW_EXPLICIT = [
    (2, 256, 128, 124, 5, 1, 1, "copy", "resid", True),           # dma3 at K = 256, one 128-column tile per clip (T = 128 is three 64-column ones)
    (7, 128, 128, 36, 5, 1, 1, "copy", "none", False),            # flat k5: 7 clips x 40 columns in 3 tiles against 7 narrow ones
    (7, 256, 128, 36, 5, 1, 1, "copy", "resid", True),            # flat k5 with dma3
    (3, 64, 128, 200, 16, 8, 1, "copy", "none", False),           # the r = 8 stencil, per-clip tiles (2 x 15 outputs for 25)
    (3, 64, 128, 400, 16, 8, 1, "copy", "film4", True),           # flat r = 8 refused by FiLM (32-row bands): per-clip
    (3, 64, 512, 400, 16, 8, 1, "copy", "film4", True),           # flat r = 8 with FiLM, 128-row bands
    (3, 64, 128, 400, 16, 8, 1, "copy", "none", False),           # flat r = 8: 11 tiles of 15 outputs against 3 x 4
    (2, 96, 192, 204, 10, 5, 1, "copy", "none", True),            # the r = 5 epilogue (tto <= 32), 96-row tiles
    (2, 64, 96, 132, 5, 1, 1, "copy", "film3", False),            # FiLM on a k5 stencil: generic epilogue, 32-row bands in a 96-row tile
    (2, 33, 192, 260, 4, 2, 1, "elu", "film3", True),             # stride 2, 64-row bands in 96-row tiles, K % 16 != 0
    (1, 512, 384, 124, 5, 1, 1, "copy", "none", False),           # one clip at K = 512: dma3, never flat
    (2, 300, 130, 60, 5, 1, 1, "copy", "resid", False),           # narrow window, 96-row tiles with clamped rows, K % 32 != 0
    (2, 64, 128, 248, 5, 1, 1, "scale", "resid", True),           # a scale without ELU: the register loader, k5 with residual
    (3, 128, 256, 124, 4, 2, 1, "copy", "film4", True),           # stride 2 / 4 by DMA on 128-column tiles with FiLM and the second output
    (2, 128, 256, 496, 8, 4, 1, "copy", "none", False),
]


def _pre(rng):
    return str(rng.choice(["elu", "elu", "copy", "copy", "scale"]))


def pw_dw_cases(n=72, seed=3024):
    """-> [(B, K, M, Tin, ks, stride, dil, pre, epi, act)]: n plain seeded draws of the recipe, then PW_DW_EXPLICIT."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        stride = int(rng.choice([1, 1, 1, 1, 2, 3, 4, 5, 8]))
        if stride == 1:
            ks, dil = int(rng.choice([1, 3, 5, 5, 5, 5, 7, 16])), int(rng.choice([1, 1, 1, 2, 3]))
        else:
            ks, dil = 2 * stride, 1
        K = int(rng.choice([3, 17, 32, 64, 96, 100, 128, 192, 256, 260, 384, 512, 768]))
        M = int(rng.choice([8, 32, 33, 64, 96, 100, 128, 130, 192, 256, 384, 512]))
        T = int(rng.choice([1, 4, 8, 36, 59, 60, 64, 68, 124, 128, 132, 248, 252, 300, 500, 1000, 1001])) * int(rng.choice([1, stride]))
        B = int(rng.choice([1, 2, 3, 7]))
        pre = _pre(rng)
        epi = str(rng.choice(["none", "resid", "film4", "film3"]))
        act = bool(rng.integers(0, 2))
        if (ks - 1) * dil + 4 > 64 or B * max(K, M) * T > BOUND:
            continue
        if epi == "resid" and stride != 1:
            epi = "none"
        if epi.startswith("film") and M % int(epi[4]):
            epi = "none"
        out.append((B, K, M, T, ks, stride, dil, pre, epi, act))
    return out + PW_DW_EXPLICIT


PRE_SCALE = {"elu": 0.8125, "scale": 0.6875, "copy": 1.0}


def pw_dw_args(case):
    B, K, M, T, ks, stride, dil, pre, epi, act = case
    return pwdw(B, K, M, T, ks=ks, stride=stride, dil=dil, pre_elu=pre == "elu", pre_scale=PRE_SCALE[pre], resid=epi == "resid",
                film=epi.startswith("film"), bands=int(epi[4]) if epi.startswith("film") else 1, Yact=act)


# (B, K, M, Tin, r, pre, act): the upsample unit.  Written out: the LDS-window loaders and the 256-row tile at their smallest shapes
UP_EXPLICIT = [(2, 64, 128, 32, 4, "copy", True),                 # loader 6 (ratio % 4 == 0, window through LDS)
               (2, 64, 96, 64, 2, "copy", False),                 # loader 7 (ratio 2)
               (1, 512, 256, 60, 8, "copy", True),                # the 256-row tile: loader 2, not the LDS window
               (2, 96, 64, 44, 3, "copy", False),                 # loader 5 on a copied operand
               (1, 32, 64, 8, 2, "copy", True),                   # narrow window, K % 32 == 0: loader 7 on the 64-column core
               (2, 48, 64, 4, 4, "copy", False)]                  # narrow window, K % 32 != 0: loader 2


def up_cases(n=34, seed=3027):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        r = i % 8 + 1
        K = int(rng.choice([6, 16, 48, 64, 96, 100, 128, 192, 256, 384]))
        M = int(rng.choice([1, 8, 32, 40, 64, 96, 100, 128, 192, 256]))
        Tin = int(rng.choice([1, 2, 3, 4, 8, 15, 16, 17, 32, 63, 64, 100, 128]))
        out.append((int(rng.choice([1, 2, 3, 7])), K, M, Tin, r, str(rng.choice(["elu", "copy", "scale"])), bool(rng.integers(0, 2))))
    return out + UP_EXPLICIT


def up_args(case):
    B, K, M, Tin, r, pre, act = case
    return pwdw(B, K, M, Tin, pre_elu=pre == "elu", pre_scale=PRE_SCALE[pre], Yact=act, ratio=r)


def convpost_cases(seed=3028):
    """-> [(B, K, M, T, ks, l2norm)]: conv_post (ELU -> depth-wise k -> 1x1 + bias [-> L2Norm]); M <= 128 with the norm."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(12):
        l2 = i % 2 == 0
        M = int(rng.choice([1, 8, 33, 64, 65, 128] if l2 else [8, 32, 64, 96, 100, 192, 256]))
        out.append((int(rng.choice([1, 2, 3])), int(rng.choice([3, 16, 64, 100, 256, 768])), M, int(rng.choice([1, 5, 50, 64, 65, 129, 300])),
                    int(rng.choice([3, 5, 7])), l2))
    return out


def specadd_cases(seed=3029):
    """-> [(B, F, C, T, act)]: the SpecBlock add x += s * (W @ P) as wv_op_dw_pw runs it (pw_dw with an identity stencil from C = 128)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(14):
        F = int(rng.choice([9, 17, 33, 65, 129, 257]))
        C = int(rng.choice([8, 32, 64, 96, 128, 192, 256, 384]))
        T = int(rng.choice([3, 50, 64, 68, 100, 128, 250, 252, 401, 1000]))
        out.append((int(rng.choice([1, 2, 3, 7])), F, C, T, C >= 128 and bool(rng.integers(0, 2))))
    return out + [(7, 65, 128, 36, True), (3, 257, 256, 132, True)]   # flat tiles with the identity stencil; dma3 (K = 257 >= 256)


def specadd_route(case):
    B, F, C, T, act = case
    return op_dw_pw_route(B, F, C, T, 0, accumulate=True, bias=False, Yact=act)


def stft_cases(seed=3030):
    """-> [(B, n_fft, hop, T)]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(20):
        n_fft = int(rng.choice([4, 16, 30, 64, 96, 128, 130, 192, 256, 512]))
        hop = int(rng.choice([1, 2, 3, 4, 8, 40]))
        T = int(rng.choice([1, 63, 64, 65, 260, 272, 1000, 1024, 1300, 2048, 4000]))
        out.append((int(rng.choice([1, 2, 3])), n_fft, hop, T))
    # interior tiles at the smallest lengths (128 frames after the n_fft - 1 pad); 136 frames: two tiles, neither interior; 96-row tiles
    return out + [(2, 64, 1, 388), (1, 256, 2, 1040), (2, 128, 2, 272), (3, 96, 4, 544)]


def specblock_cases():
    """-> [(B, n_fft, hop, T)]: the one-launch SpecBlock, n_fft = C in {64, 128}, more than 64 frames, Tf % 4 == 0; Tf = 68 is the smallest."""
    return [(1, 64, 1, 68), (2, 128, 1, 68), (3, 64, 2, 263), (2, 128, 2, 520), (3, 64, 1, 388), (1, 128, 4, 2045), (2, 64, 4, 1024), (2, 128, 1, 132)]


def resblock_cases(seed=3031):
    """-> [(B, C, T, outs)]: the one-launch ResnetBlock; outs in "raw", "act", "both"."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(16):
        C = (64, 96, 128, 192)[i % 4]
        T = int(rng.choice([4, 8, 12, 112, 116, 120, 236, 240, 244, 248, 252, 476, 488, 492, 736]))
        out.append((int(rng.choice([1, 2, 3, 7])), C, T, ("raw", "act", "both")[i % 3]))
    return out


# what a draw of the recipe rarely lines up: n_fft_base == channels_enc with T % (4 hop) == 0 (one-launch SpecBlocks at 64 and 128 between one-launch
# ResnetBlocks at 64 / 128), and a 384-channel decoder stage with blocks at a length that is a multiple of 4
NET_EXPLICIT = [
    (dict(strides=[2, 2, 2], channels_enc=16, channels_dec=24, dimension=32, n_fft_base=16, n_residual_enc=2, n_residual_dec=2, kernel_size=5,
          last_kernel_size=5, residual_kernel_size=5, dilation_base=1, output_dim=8, embedding_dim=16, embedding_layers=1), 1280, 2),
    (dict(strides=[2, 2, 2], channels_enc=32, channels_dec=48, dimension=16, n_fft_base=32, n_residual_enc=1, n_residual_dec=3, kernel_size=7,
          last_kernel_size=3, residual_kernel_size=5, dilation_base=1, output_dim=4, embedding_dim=8, embedding_layers=2), 1088, 1),
    (dict(strides=[4, 2, 2], channels_enc=48, channels_dec=48, dimension=64, n_fft_base=16, n_residual_enc=2, n_residual_dec=2, kernel_size=3,
          last_kernel_size=7, residual_kernel_size=5, dilation_base=1, output_dim=8, embedding_dim=8, embedding_layers=1), 1024, 3),
]


def net_cases(n=14, seed=3032):
    """-> [(idx, cfg kwargs, T, B)]: n drawn whole-net configurations with stages at C = 64 .. 384, then NET_EXPLICIT."""
    rng = np.random.default_rng(seed)
    out = []
    stride_sets = [[2, 2, 2], [2, 3, 2], [4, 2, 2], [2, 2, 2, 2], [5, 2, 2], [8, 2, 2], [2, 2, 4], [3, 2, 2, 2]]
    for i in range(n):
        strides = stride_sets[int(rng.integers(0, len(stride_sets)))]
        ce = int(rng.choice([16, 24, 32, 48]))
        kw = dict(strides=list(strides), channels_enc=ce, channels_dec=int(rng.choice([12, 24, 48])), dimension=int(rng.choice([16, 32, 64])),
                  n_fft_base=int(rng.choice([ce, ce, 16, 32])), n_residual_enc=int(rng.integers(0, 4)), n_residual_dec=int(rng.integers(0, 4)),
                  kernel_size=int(rng.choice([3, 5, 7])), last_kernel_size=int(rng.choice([3, 5, 7])),
                  residual_kernel_size=int(rng.choice([5, 5, 5, 5, 3])), dilation_base=int(rng.choice([1, 1, 1, 1, 2])),
                  output_dim=int(rng.choice([4, 8])), embedding_dim=int(rng.choice([8, 16])), embedding_layers=int(rng.integers(1, 3)))
        hop = int(np.prod(strides))
        T = int(rng.choice([4 * hop * (1300 // (4 * hop)), 4 * hop * max(1, 650 // (4 * hop)), 2 * hop * (1300 // (2 * hop)), 1041, 777]))
        out.append((i, kw, T, int(rng.integers(1, 4))))
    return out + [(n + i, kw, T, B) for i, (kw, T, B) in enumerate(NET_EXPLICIT)]


def net_cfg_dict(kw):
    """The fields net_plan reads, with the defaults of default_config."""
    d = dict(freq_bands=4)
    d.update(kw)
    return d
