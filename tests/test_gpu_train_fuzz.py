"""Seeded geometry fuzz of the training kernels (waveverify_amd/csrc/wv_train.hip) against the float64 oracles: the case lists of
tests/train_fuzz_cases.py -- every stencil-backward route, the generic ConvTranspose kernels, the dW GEMM's tiles / loaders / split plan
with more items than splits, clip counts past the eight clip groups, ragged heads / tails / FiLM, and whole nets at configurations the
trained nets never combined (tests/test_train_fuzz_cases_cpu.py holds the coverage conditions).

Bars (the project's own): forward 2e-5, every gradient 1e-4, of the REFERENCE tensor's largest magnitude -- no floor at 1.0, so a small
tensor is held to its own size; whole nets: test_gpu_trainer.check_grads at 5e-4, loss and watermarked audio at 2e-5.  Every backward
runs twice and must be bit-equal."""
import numpy as np
import pytest
import torch

import train_fuzz_cases as FC
from oracle import wv_oracle_train as OT

pytestmark = pytest.mark.gpu
FWD, GRAD = 2e-5, 1e-4


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rn(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)


def _gain(rng, n):
    return (0.5 + np.abs(rng.standard_normal((n, 1, 1)))).astype(np.float32)


class Case:
    """Errors of one case's tensors, each relative to |ref|max of that tensor (no floor).  Two kinds of tensor need care:
    - a gradient that is ZERO IN EXACT ARITHMETIC (dv of a one-element weight-norm row: dv = g / |v| * (dW - dW v^2 / v^2); the oracle
      returns ~1e-14 there): `scale=` is given by the caller -- the size of the terms that cancel, max over rows of |g| / ||v|| * |dW|
      (wn_zero_scale, row by row) -- instead of dividing by 1e-14 or skipping the tensor;
    - a reference that IS zero / absent (dx with need_dx=False, FiLM heads of the other scales): `zero()` demands exactly that."""

    def __init__(self, cid):
        self.cid, self.items = cid, []

    def add(self, name, got, ref, bar, scale=None):
        ref = np.asarray(ref, dtype=np.float64)
        got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
        assert np.isfinite(got).all(), (self.cid, name)
        scale = float(np.abs(ref).max()) if scale is None else np.asarray(scale, np.float64).reshape(ref.shape)      # per tensor, or per element
        assert np.all(scale > 0.0), (self.cid, name, "zero reference: use zero() or give the scale of the cancelling terms")
        self.items.append((float((np.abs(got - ref) / scale).max()), bar, name))

    def zero(self, name, got):
        assert got is None or float(got.abs().max()) == 0.0, (self.cid, name)

    def done(self):
        fwd, grad = ([it for it in self.items if it[1] == b] for b in (FWD, GRAD))
        (ef, _, nf), (eg, _, ng) = max(fwd), max(grad)
        print(f"MEASURE train fuzz {self.cid}: forward {nf} {ef:.2e} (bar {FWD:.0e}), worst gradient {ng} {eg:.2e} (bar {GRAD:.0e})")
        bad = [(n, f"{e:.2e}") for e, b, n in self.items if e > b]
        assert not bad, (self.cid, bad)


def wn_zero_scale(g, v, dg_ref):
    """One-element weight-norm rows: dW[m] = +-dg[m] there, so the cancelling terms of dv[m] have size |g[m]| / |v[m]| * |dg_ref[m]|.
    -> one scale per row, shaped like dv (each row is held to its own terms: a row with a tiny |v| loosens no other row)."""
    g, v = np.asarray(g, np.float64).reshape(-1), np.asarray(v, np.float64)
    assert v.size == g.size
    return (np.abs(g) / np.abs(v.reshape(-1)) * np.abs(np.asarray(dg_ref, np.float64).reshape(-1))).reshape(v.shape)


def _same(a, b, what):
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), f"{what}: {k} differs between two runs of the same backward"


# ---- the strided unit ---------------------------------------------------------------------------------------------------------------
def _unit_params(rng, K, M, ks):
    return dict(g_pw=_gain(rng, M), v_pw=_rn(rng, M, K, 1, scale=K ** -0.5), g_dw=_gain(rng, M), v_dw=_rn(rng, M, 1, ks, scale=ks ** -0.5),
                b_dw=_rn(rng, M, scale=0.1))


def _unit_case(c, B, K, M, T, ks, stride, elu, need_dx, seed):
    from waveverify_amd.train import TrainUnit
    rng = np.random.default_rng(seed)
    x, p = _rn(rng, B, K, T), _unit_params(rng, K, M, ks)
    dy = _rn(rng, B, M, -(-T // stride))
    s = float(rng.uniform(0.5, 1.0))
    ref = OT.unit_backward(x, s, p["g_pw"], p["v_pw"], p["g_dw"], p["v_dw"], p["b_dw"], dy, stride=stride, elu=elu)
    u = TrainUnit(K, M, ks, stride)
    pt = {k: _cu(v) for k, v in p.items()}
    xt, dyt = _cu(x), _cu(dy)
    c.add("y", u.forward(xt, pt, s, elu), ref["y"], FWD)
    g, g2 = u.backward(xt, pt, s, dyt, elu, need_dx), u.backward(xt, pt, s, dyt, elu, need_dx)
    _same(g, g2, c.cid)
    if need_dx:
        c.add("dx", g["dx"], ref["dx"], GRAD)
    else:
        c.zero("dx", g["dx"])
        assert g["dx"] is None
    for k in ("dg_pw", "dg_dw", "db_dw"):
        c.add(k, g[k], ref[k], GRAD)
    c.add("dv_pw", g["dv_pw"], ref["dv_pw"], GRAD, wn_zero_scale(p["g_pw"], p["v_pw"], ref["dg_pw"]) if K == 1 else None)
    c.add("dv_dw", g["dv_dw"], ref["dv_dw"], GRAD, wn_zero_scale(p["g_dw"], p["v_dw"], ref["dg_dw"]) if ks == 1 else None)


@pytest.mark.parametrize("B,K,M,T,ks,stride,elu,need_dx", FC.unit_cases())
def test_unit_fuzz(B, K, M, T, ks, stride, elu, need_dx):
    c = Case(f"unit B={B} K={K} M={M} T={T} ks={ks} s={stride} elu={int(elu)} dx={int(need_dx)} [{FC.dw_bwd_route(ks, stride, T)}, "
             f"tile {FC.nt_tile(M, K)}{'v' if T % 4 == 0 else 's'}]")
    _unit_case(c, B, K, M, T, ks, stride, elu, need_dx, seed=B * 7919 + K * 131 + M * 17 + T + ks)
    c.done()


# ---- whole block ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,T,with_param", FC.block_cases())
def test_block_fuzz(B, C, T, with_param):
    from waveverify_amd.train import TrainBlock
    c = Case(f"block B={B} C={C} T={T} param={int(with_param)} [{FC.block_forward_route(C, T)}]")
    rng = np.random.default_rng(B * 77 + C + T)
    x, dy = _rn(rng, B, C, T), _rn(rng, B, C, T)
    ps = [_unit_params(rng, C, C, 5) for _ in range(2)]
    rsp = np.array([0.8], np.float32) if with_param else None
    pre, rs = 0.8164966, 0.5773503
    ref = OT.block_backward(x, ps, rsp, pre, rs, dy)
    blk = TrainBlock(C)
    pt = [{k: _cu(v) for k, v in p.items()} for p in ps]
    rt = None if rsp is None else _cu(rsp)
    y, saved = blk.forward(_cu(x), pt, rt, pre, rs)
    c.add("y", y, ref["y"], FWD)
    g = blk.backward(_cu(x), pt, rt, pre, rs, _cu(dy), saved)
    g2 = blk.backward(_cu(x), pt, rt, pre, rs, _cu(dy), saved)
    assert torch.equal(g["dx"], g2["dx"])
    c.add("dx", g["dx"], ref["dx"], GRAD)
    for i in (0, 1):
        _same(g["halves"][i], g2["halves"][i], c.cid)
        for k in ("dg_pw", "dv_pw", "dg_dw", "dv_dw", "db_dw"):
            c.add(f"h{i}.{k}", g["halves"][i][k], ref["halves"][i][k], GRAD)
    if with_param:
        assert torch.equal(g["d_res_scale_param"], g2["d_res_scale_param"])
        c.add("d_res_scale_param", g["d_res_scale_param"], [ref["d_res_scale_param"]], GRAD)
    else:
        assert g["d_res_scale_param"] is None
    c.done()


# ---- upsample unit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,M,Tin,r", FC.up_cases())
def test_upsample_fuzz(B, K, M, Tin, r):
    from waveverify_amd.train import TrainUp
    c = Case(f"up B={B} K={K} M={M} Tin={Tin} r={r} [{FC.up_route(r)}]")
    rng = np.random.default_rng(K * 19 + M * 3 + Tin * 7 + r)
    x, dy = _rn(rng, B, K, Tin), _rn(rng, B, M, Tin * r)
    p = dict(g_ct=_gain(rng, K), v_ct=_rn(rng, K, 1, 2 * r, scale=(2 * r) ** -0.5), g_pw=_gain(rng, M), v_pw=_rn(rng, M, K, 1, scale=K ** -0.5),
             b=_rn(rng, M, scale=0.1))
    elu, s = bool(rng.integers(0, 2)), float(rng.uniform(0.5, 1.0))
    ref = OT.up_backward(x, s, p["g_ct"], p["v_ct"], p["g_pw"], p["v_pw"], p["b"], dy, elu=elu)
    u = TrainUp(K, M, r)
    pt = {k: _cu(v) for k, v in p.items()}
    c.add("y", u.forward(_cu(x), pt, s, elu), ref["y"], FWD)
    g, g2 = u.backward(_cu(x), pt, s, _cu(dy), elu), u.backward(_cu(x), pt, s, _cu(dy), elu)
    _same(g, g2, c.cid)
    for k in ("dx", "dg_ct", "dv_ct", "dg_pw", "dv_pw", "db"):
        c.add(k, g[k], ref[k], GRAD)
    c.done()


# ---- decoder tail ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,Tin,T,ks", FC.tail_cases())
def test_tail_fuzz(B, C, Tin, T, ks):
    """Against torch.nn.functional in float64, as test_decoder_tail_vs_torch_autograd builds the reference's tail."""
    from waveverify_amd.train import TrainTail
    import torch.nn.functional as F
    c = Case(f"tail B={B} C={C} Tin={Tin} T={T} ks={ks} [{FC.tail_route(ks, Tin, T)}]")
    torch.manual_seed(C * 31 + ks + Tin)
    post, wav_std = 0.7071068, 0.1122080159
    # float32 values, held in float64 leaves: the kernels and the oracle see the same numbers
    g = (0.5 + torch.rand(1, 1, 1, dtype=torch.float64)).float().double().requires_grad_(True)
    v = (torch.randn(1, C, ks, dtype=torch.float64) * (C * ks) ** -0.5).float().double().requires_grad_(True)
    b = (0.1 * torch.randn(1, dtype=torch.float64)).float().double().requires_grad_(True)
    x = torch.randn(B, C, Tin, dtype=torch.float64).float().double().requires_grad_(True)
    w = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
    delta = torch.tanh(wav_std * F.conv1d(F.pad(F.elu(x * post), (ks - 1, 0)), w, b))[..., :T]
    dd = torch.randn_like(delta).float().double()
    delta.backward(dd)
    u = TrainTail(C, ks)
    p = dict(g=g.detach().float().cuda(), v=v.detach().float().cuda(), b=b.detach().float().cuda())
    xt = x.detach().float().cuda()
    got = u.forward(xt, p, post, wav_std, T)
    c.add("delta", got, delta.detach().numpy(), FWD)
    gr, gr2 = u.backward(xt, p, post, wav_std, got, dd.float().cuda()), u.backward(xt, p, post, wav_std, got, dd.float().cuda())
    _same(gr, gr2, c.cid)
    for k, ref in (("dx", x.grad), ("dg", g.grad), ("db", b.grad)):
        c.add(k, gr[k], ref.numpy(), GRAD)
    c.add("dv", gr["dv"], v.grad.numpy(), GRAD, wn_zero_scale(g.detach().numpy(), v.detach().numpy(), g.grad.numpy()) if C * ks == 1 else None)
    c.done()


# ---- head, conv_pre, conv_post, SpecBlock add --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,O,nb,hop,N,T", FC.head_cases())
def test_head_fuzz(B, D, O, nb, hop, N, T):
    """Against torch's ConvTranspose1d -> trim -> Conv1d in float64, as test_head_forward_backward_vs_torch_modules."""
    from waveverify_amd.train import TrainHead
    c = Case(f"head B={B} D={D} O={O} nb={nb} hop={hop} N={N} T={T}")
    torch.manual_seed(D * 7 + hop + T)
    rev, last = torch.nn.ConvTranspose1d(D, O, hop, hop), torch.nn.Conv1d(O, nb, 1)           # float32 parameters, then the same values in float64
    p = dict(w_rev=rev.weight.detach().cuda(), b_rev=rev.bias.detach().cuda(), w_last=last.weight.detach().cuda(), b_last=last.bias.detach().cuda())
    rev, last = rev.double(), last.double()
    z32 = torch.randn(B, D, N)
    z = z32.double().requires_grad_(True)
    logits = last(rev(z)[:, :, :T])
    dl = torch.randn(logits.shape).double()
    logits.backward(dl)
    h = TrainHead(D, O, nb, hop)
    c.add("logits", h.forward(z32.cuda(), p, T), logits.detach().numpy(), FWD)
    g, g2 = h.backward(z32.cuda(), p, dl.float().cuda()), h.backward(z32.cuda(), p, dl.float().cuda())
    _same(g, g2, c.cid)
    for k, ref in (("dz", z.grad), ("dw_rev", rev.weight.grad), ("db_rev", rev.bias.grad), ("dw_last", last.weight.grad[:, :, 0]), ("db_last", last.bias.grad)):
        c.add(k, g[k], ref.numpy(), GRAD)
    c.done()


@pytest.mark.parametrize("B,C,T,ks", FC.convpre_cases())
def test_convpre_fuzz(B, C, T, ks):
    from waveverify_amd.train import TrainConvPre
    c = Case(f"conv_pre B={B} C={C} T={T} ks={ks}")
    rng = np.random.default_rng(B + C * 11 + T)
    x, dy = _rn(rng, B, 1, T, scale=0.1), _rn(rng, B, C, T)
    p = dict(g=_gain(rng, C), v=_rn(rng, C, 1, ks, scale=0.45), b=_rn(rng, C, scale=0.1))
    ref = OT.convpre_backward(x, 8.912, p["g"], p["v"], p["b"], dy)
    u = TrainConvPre(C, ks)
    pt = {k: _cu(v) for k, v in p.items()}
    c.add("y", u.forward(_cu(x), pt, 8.912), ref["y"], FWD)
    g, g2 = u.backward(_cu(x), pt, 8.912, _cu(dy), need_dx=True), u.backward(_cu(x), pt, 8.912, _cu(dy), need_dx=True)
    _same(g, g2, c.cid)
    for k in ("dx", "dg", "dv", "db"):
        c.add(k, g[k], ref[k], GRAD)
    g0 = u.backward(_cu(x), pt, 8.912, _cu(dy))
    c.zero("dx (need_dx=False)", g0["dx"])
    assert g0["dx"] is None and torch.equal(g0["dv"], g["dv"])
    c.done()


@pytest.mark.parametrize("B,C,D,T,ks,l2norm", FC.convpost_cases())
def test_convpost_fuzz(B, C, D, T, ks, l2norm):
    from waveverify_amd.train import TrainConvPost
    c = Case(f"conv_post B={B} C={C} D={D} T={T} ks={ks} l2norm={int(l2norm)}")
    rng = np.random.default_rng(B + C * 11 + D * 5 + T)
    x, dy = _rn(rng, B, C, T), _rn(rng, B, D, T)
    p = dict(g_dw=_gain(rng, C), v_dw=_rn(rng, C, 1, ks, scale=0.45), g_pw=_gain(rng, D), v_pw=_rn(rng, D, C, 1, scale=C ** -0.5), b=_rn(rng, D))
    ref = OT.convpost_backward(x, p["g_dw"], p["v_dw"], p["g_pw"], p["v_pw"], p["b"], dy, l2norm=l2norm)
    u = TrainConvPost(C, D, ks, l2norm=l2norm)
    pt = {k: _cu(v) for k, v in p.items()}
    c.add("y", u.forward(_cu(x), pt), ref["y"], FWD)
    g, g2 = u.backward(_cu(x), pt, _cu(dy)), u.backward(_cu(x), pt, _cu(dy))
    _same(g, g2, c.cid)
    for k in ("dx", "dg_dw", "dv_dw", "dg_pw", "dv_pw", "db"):
        c.add(k, g[k], ref[k], GRAD)
    c.done()


def _spec_case(c, B, C, F, T, seed):
    from waveverify_amd.train import TrainSpecAdd
    rng = np.random.default_rng(seed)
    x, P, dy = _rn(rng, B, C, T), _rn(rng, B, F, T), _rn(rng, B, C, T)
    p = dict(g=_gain(rng, C), v=_rn(rng, C, F, 1, scale=F ** -0.5))
    spn = np.array([0.7], np.float32)
    ref = OT.spec_add_backward(x, P, p["g"], p["v"], spn, 0.5773503, dy)
    u = TrainSpecAdd(C, F)
    pt = {k: _cu(v) for k, v in p.items()}
    Pt, dyt, st = _cu(P), _cu(dy), _cu(spn)
    c.add("y", u.forward(_cu(x), Pt, pt, st, 0.5773503), ref["y"], FWD)
    g, g2 = u.backward(Pt, pt, st, 0.5773503, dyt), u.backward(Pt, pt, st, 0.5773503, dyt)
    _same({k: g[k] for k in ("dg", "dv", "d_scale_param")}, g2, c.cid)
    c.add("dg", g["dg"], ref["dg"], GRAD)
    c.add("dv", g["dv"], ref["dv"], GRAD)
    c.add("d_scale_param", g["d_scale_param"], [ref["d_scale_param"]], GRAD)


@pytest.mark.parametrize("B,C,F,T", FC.spec_cases())
def test_spec_add_fuzz(B, C, F, T):
    c = Case(f"spec_add B={B} C={C} F={F} T={T}")
    _spec_case(c, B, C, F, T, seed=B + C * 11 + F * 5 + T)
    c.done()


# ---- the dW GEMM's split plan: more (clip, chunk) items than splits ----------------------------------------------------------------
@pytest.mark.parametrize("kind,B,C,F,T", FC.split_plan_cases())
def test_dw_gemm_split_plan(kind, B, C, F, T):
    """Every split of gemm_nt runs its item loop more than once here (items > S by the restated nt_plan); last chunk of 4 samples, the
    scalar loader at T % 4 == 1, the 128-row tile with clamped rows; through TrainSpecAdd (gemm_nt + sum_parts and little else) and once
    inside a unit."""
    plan = FC.nt_plan(B, T, C, F)
    assert plan["items"] > plan["S"]
    c = Case(f"split plan {kind} B={B} M={C} K={F} T={T} [tile {plan['tile']}, {plan['tiles']} tiles, {plan['S']} splits, {plan['items']} items, "
             f"{'vector' if plan['vec'] else 'scalar'} loader]")
    if kind == "spec":
        _spec_case(c, B, C, F, T, seed=T)
    else:
        _unit_case(c, B, F, C, T, 5, 1, True, True, seed=T + 1)
    c.done()


# ---- message MLP + FiLM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,L,strides,B,C,T,scale", FC.film_cases())
def test_film_fuzz(E, L, strides, B, C, T, scale):
    """Against the float64 torch modules, as test_film_mlp_vs_torch_modules builds them."""
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import FilmMlp
    lin = torch.nn.functional.linear
    c = Case(f"film E={E} L={L} scales={len(strides)} B={B} C={C} T={T} scale={scale}")
    cfg = default_config("generator", embedding_dim=E, embedding_layers=L, strides=list(strides), channels_enc=4, channels_dec=4, dimension=8, n_fft_base=8)
    sd = random_state_dict(cfg, E + L, parametrized=True)
    fm = FilmMlp(cfg)
    params = {k: _cu(np.asarray(sd[k], np.float32)) for k in fm.keys}
    rng = np.random.default_rng(E + B + T)
    msg = rng.integers(0, 2, (B, cfg.msg_dimension)).astype(np.float32)
    x, dy = _rn(rng, B, C, T), _rn(rng, B, C, T)
    leaf = {k: torch.tensor(np.asarray(sd[k], np.float32), dtype=torch.float64, requires_grad=True) for k in fm.keys}
    e = lin(torch.from_numpy(msg).double(), leaf["encoder.msg_embedding.0.weight"], leaf["encoder.msg_embedding.0.bias"])
    for i in range(L):
        e = torch.relu(lin(e, leaf[f"encoder.msg_embedding.{1 + 2 * i}.weight"], leaf[f"encoder.msg_embedding.{1 + 2 * i}.bias"]))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    bw, bands = C // cfg.freq_bands, []
    for b in range(cfg.freq_bands):
        ga = lin(e, leaf[f"encoder.film_layers.{scale}.{b}.gamma_layer.weight"], leaf[f"encoder.film_layers.{scale}.{b}.gamma_layer.bias"]).unsqueeze(-1)
        be = lin(e, leaf[f"encoder.film_layers.{scale}.{b}.beta_layer.weight"], leaf[f"encoder.film_layers.{scale}.{b}.beta_layer.bias"]).unsqueeze(-1)
        bands.append(xt[:, b * bw:(b + 1) * bw] * ga + be)
    y = torch.cat(bands, 1)
    y.backward(torch.from_numpy(dy).double())
    runs = []
    for _ in range(2):
        gviews = {k: torch.zeros_like(v) for k, v in params.items()}
        film = fm.forward(_cu(msg), params)
        got = fm.apply(_cu(x), film, scale)
        dfilm = torch.zeros_like(film)
        dx = fm.apply_backward(_cu(x), film, _cu(dy), dfilm, scale)
        fm.backward(dfilm, gviews)
        runs.append(dict(gviews, dx=dx, dfilm=dfilm))
    _same(runs[0], runs[1], c.cid)
    c.add("y", got, y.detach().numpy(), FWD)
    c.add("dx", dx, xt.grad.numpy(), GRAD)
    for k in fm.keys:
        r = leaf[k].grad
        if r is None or float(r.abs().max()) == 0.0:           # the other scales' heads (and layers behind dead ReLUs): untouched by this loss
            c.zero(k, runs[0][k])
        else:
            c.add(k, runs[0][k], r.numpy(), GRAD)
    c.done()


# ---- whole nets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["generator", "detector", "locator"])
@pytest.mark.parametrize("idx,cfgkw,T,B", FC.net_cases())
def test_whole_net_trainers_fuzz(idx, cfgkw, T, B, kind):
    """EncoderNetTrainer / GeneratorTrainer against oracle/wv_oracle_train_torch.py at configurations no trained net combined: odd and
    three- / four-stage strides, kernel sizes 3 / 7, one to three residual blocks and embedding layers."""
    from oracle import wv_oracle_train_torch as OTT
    from test_gpu_trainer import check_grads
    from waveverify_amd.config import default_config
    from waveverify_amd.init import random_state_dict
    from waveverify_amd.train import EncoderNetTrainer, GeneratorTrainer, bce_logits
    kw = dict(cfgkw)
    if kind != "generator":
        kw = {k: v for k, v in kw.items() if k not in ("channels_dec", "n_residual_dec", "embedding_dim", "embedding_layers")}
    cfg = default_config(kind, **kw)
    sd = random_state_dict(cfg, 31 + idx, parametrized=True)
    rng = np.random.default_rng(1000 + idx)
    x = _rn(rng, B, 1, T, scale=0.1)
    msg = rng.integers(0, 2, (B, cfg.nbits)).astype(np.float32)
    cid = f"net #{idx} {kind} strides={cfgkw['strides']} T={T} B={B}"
    if kind == "generator":
        target = (x + _rn(rng, B, 1, T, scale=0.01)).astype(np.float32)
        ref_loss, ref_wm, ref_grads, _ = OTT.generator_loss_and_grads(cfg, sd, x, msg, target)
        tr = GeneratorTrainer(cfg, sd)
        wm = tr.forward(_cu(x), _cu(msg))
        e_fwd = float(np.abs(wm.cpu().numpy() - ref_wm).max() / np.abs(ref_wm).max())
        loss = float(((wm.double().cpu() - torch.from_numpy(target).double()) ** 2).mean())     # the test's own MSE, on the GPU's audio
        e_fwd = max(e_fwd, abs(loss - ref_loss) / abs(ref_loss))
        tr.backward(2.0 * (wm - _cu(target)) / wm.numel())
        first = tr.grads.clone()
        tr.forward(_cu(x), _cu(msg))
        tr.backward(2.0 * (wm - _cu(target)) / wm.numel())
    else:
        mask = (rng.random((B, 1, T)) < 0.7).astype(np.float32)
        m = msg if kind == "detector" else None
        ref_loss, _, ref_grads, _ = OTT.loss_and_grads(cfg, sd, x, mask, m)
        tr = EncoderNetTrainer(cfg, sd)
        loss, dz = bce_logits(tr.forward(_cu(x)), _cu(mask), None if m is None else _cu(m))
        e_fwd = abs(float(loss.item()) - ref_loss) / abs(ref_loss)
        tr.backward(dz)
        first = tr.grads.clone()
        tr.forward(_cu(x))
        tr.backward(dz)
    assert torch.equal(first, tr.grads), f"{cid}: the backward pass must be deterministic"
    try:
        worst = check_grads(tr, ref_grads, tol=5e-4)
    finally:
        print(f"MEASURE train fuzz {cid}: {'wm / loss' if kind == 'generator' else 'loss'} {e_fwd:.2e} (bar 2e-05)")
    print(f"MEASURE train fuzz {cid}: worst gradient {worst[0]} {worst[1]:.2e} (bar 5e-04)")
    assert e_fwd <= FWD, (cid, e_fwd)
