"""CPU oracle of the f16-operand / f32-accumulate MODE (csrc/wv_h16.hip), torch flavour.  TEST INFRASTRUCTURE ONLY (tests/, tools/).

The mode is a different arithmetic from the reference's (activations and weights cross HBM as f16, sums are f32), so next to the checks
against the reference's own outputs (tests/golden) it gets an oracle of ITS arithmetic: the torch port of the reference path
(oracle/wv_oracle_torch.py, pinned to the reference's outputs) with a round-to-f16 inserted at every point where a kernel of the mode
rounds -- and nowhere else.  Sums here are float64, so what separates this oracle from the GPU is f32 summation order plus the
occasional f16 value that lands on the other side of a rounding boundary.  Rounding points (kernel -> what is rounded):

  conv_pre16          the stream after conv_pre (modules/seanet.py:657-664)
  rh_kernel           per ResnetBlock (seanet.py:245-281): a' = f16(log2e * ELU(c x)), W1 / log2e and W2 / log2e as f16, u' = f16(log2e *
                      ELU(DW5(W1' a') + b1)) -- the kernel keeps both activations times log2(e) and the packer divides the weights by
                      it --, the block's output y (or its activated copy) as f16
  spec16_kernel       per SpecBlock (seanet.py:463-511): the normalised log-magnitude P as f16 (the DFT itself runs on 22-bit split operands:
                      exact here), the 1x1 weight as f16, the output ELU(c x') as f16
  conv16 / conv16s    per downsample unit (seanet.py:724-760): the COMPOSED weight W[m][i][k] = pw[m][k] dw[m][i] as f16, FiLM (seanet.py:928-966)
                      in f32 behind it, the output as f16
  conv16 (conv_post)  ELU(x') as f16, the composed weight pw[m][k] dw[k][i] as f16 (seanet.py:797-823); the latent stays f32
  conv_post16         = the line above: the mean-probability output's conv_post (spec_post's output ELU(x') as f16, composed weight as f16),
                      run only where head16 runs behind it; on the logits outputs spec_post's x' stays f32 and conv_post is the exact path's
  head16_kernel       mean probabilities only (detector.py:300-310): the L2Norm's z = y * sqrt(D) / max(||y||, 1e-12) as f16 (its f32 sum
                      of squares restated operation by operation, so that the f16 roundings coincide), the composed head weight
                      wc[d][bit * hop + j] = sum_o last[bit][o] rev[d][o][j] as f16, logits / sigmoid / time sum in f32 -- see head16()
  l2norm_c8           the normalised latent as f16 (seanet.py:288-318)
  conv16 (dec head)   decoder.model.0/.1 composed, output ELU(.) as f16 (seanet.py:1081-1094)
  conv16u             per upsample unit (seanet.py:1147-1170, conv.py:838-881): the composed weights pw[m][k] ct[k][p] and pw[m][k] ct[k][p + r]
                      as f16, the output as f16
  tail16              nothing (f32 sums over the f16 activated stream; seanet.py:1177-1202)

The detector and locator end in one of two tails, chosen as run_head_model (csrc/wv_model.hip) chooses (head16_gate):
  head16 tail (detect_mean_prob)      spec_post -> f16(ELU(x')) -> conv_post16 -> f32 latent -> head16_kernel
  f32 tail (detect_logits, locate)    spec_post's x' in f32 (not rounded), then conv_post, L2Norm and the head of the exact path; also the
                                      mean-probability output wherever the head16 gate is false
spec_post itself runs on the f16 pipe whenever the top stage's width is a multiple of 16 (spec_post16): fused (spec16_kernel) or as the
exact STFT -> P as f16 -> the 1x1 with an f16 weight -- one arithmetic, restated once here.  Without that plan the last downsample unit
writes f32 and spec_post is the exact path's (not reachable from a configuration the f16 plan accepts: widths there are multiples of 8
doubled at every stage; mirrored for completeness).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import wv_oracle_torch as OT
from .wv_oracle import decoder_layout, dft_basis

L2E = 1.4426950408889634


def h(t: torch.Tensor) -> torch.Tensor:
    return t.half().double()


def _w(net, k):
    return net.w(k).double()


def resnet_block(net, pre, x, idx, rs, act_scale=None):
    """-> y (f16-rounded), or f16(ELU(act_scale * y)) when act_scale is given (the last block of a decoder stage)."""
    C = x.shape[1]
    a = h(L2E * F.elu(x * (1 + idx * rs ** 2) ** -0.5))
    y1 = OT.sconv1d(a, h(_w(net, f"{pre}.block.1.conv.conv.weight") / L2E), None)
    wd = _w(net, f"{pre}.block.2.conv.conv.weight")
    y1 = OT.sconv1d(y1, wd, _w(net, f"{pre}.block.2.conv.conv.bias"), groups=C)
    u = h(L2E * F.elu(y1))
    y2 = OT.sconv1d(u, h(_w(net, f"{pre}.block.4.conv.conv.weight") / L2E), None)
    wd = _w(net, f"{pre}.block.5.conv.conv.weight")
    v = OT.sconv1d(y2, wd, _w(net, f"{pre}.block.5.conv.conv.bias"), groups=C)
    p = net.opt(f"{pre}.res_scale_param")
    y = x + v * float(np.float32(rs) * (np.float32(p.reshape(-1)[0].item()) if p is not None else np.float32(1.0)))
    return h(y) if act_scale is None else h(F.elu(y * act_scale))


def spec_block_raw(net, pre, x, wav, n_fft, hop, mean, std, rs, f16=True):
    """x' = x + scale * (W @ P): P and W rounded to f16 (the f16 pipe), or both exact (f16=False: the exact path's spec block)."""
    r = h if f16 else (lambda t: t)
    basis = net.opt(f"{pre}.spec.weight")
    basis = (OT._t(dft_basis(n_fft))[:, None, :] if basis is None else basis).double()
    c = F.conv1d(F.pad(wav, (n_fft - 1, 0)), basis, None, stride=hop)
    Fq = n_fft // 2 + 1
    mag2 = (c[:, :Fq] ** 2 + c[:, Fq:] ** 2).clamp_min(1e-10)                 # the kernels' 0.5 log(max(p, 1e-10)) form (wv_dev.h stft_logmag)
    P = r((0.5 * mag2.log() - mean) / std)
    y = OT.sconv1d(P, r(_w(net, f"{pre}.layer.conv.conv.weight")), None)
    p = net.opt(f"{pre}.scale_param")
    s = float(np.float32(rs) * (np.float32(p.reshape(-1)[0].item()) if p is not None else np.float32(1.0)))
    return x + y * s


def spec_block_act(net, pre, x, wav, n_fft, hop, mean, std, rs, act_scale):
    return h(F.elu(spec_block_raw(net, pre, x, wav, n_fft, hop, mean, std, rs) * act_scale))


def encoder_stages(net, x, msg, round_last=True):
    """conv_pre ... the last downsample unit (seanet.py:883-968) in the mode's arithmetic -> (the stream spec_post adds to, the waveform,
    spec_post's hop, its n_fft multiple).  round_last=False: the last downsample's output stays f32 (no f16 spec_post plan)."""
    cfg = net.cfg
    rs = cfg.res_scale_enc
    wav = x
    hcur = h(OT.sconv1d(x * float(np.float32(1.0 / cfg.wav_std)), _w(net, "encoder.conv_pre.1.conv.conv.weight"), _w(net, "encoder.conv_pre.1.conv.conv.bias")))
    film = None
    if msg is not None:
        e = F.linear(msg.float(), net.w("encoder.msg_embedding.0.weight"), net.w("encoder.msg_embedding.0.bias"))
        for i in range(cfg.embedding_layers):
            j = 1 + 2 * i
            e = F.relu(F.linear(e, net.w(f"encoder.msg_embedding.{j}.weight"), net.w(f"encoder.msg_embedding.{j}.bias")))
        film = e                                                    # message MLP and FiLM scalars are f32 in the mode too
    stride, mult = 1, 1
    down_scale = (1 + cfg.n_residual_enc * rs ** 2) ** -0.5
    for s, r in enumerate(cfg.ratios_enc):
        for j in range(1, cfg.n_residual_enc + 1):
            hcur = resnet_block(net, f"encoder.blocks.{s}.{j - 1}", hcur, j, rs)
        a = spec_block_act(net, f"encoder.spec_blocks.{s}", hcur, wav, mult * cfg.n_fft_base, stride, cfg.spec_means[s], cfg.spec_stds[s], rs, down_scale)
        stride *= r
        pw = _w(net, f"encoder.downsample.{s}.2.conv.conv.weight")
        wd = _w(net, f"encoder.downsample.{s}.3.conv.conv.weight")
        wc = h((pw[:, :, 0, None].float() * wd[:, 0, None, :].float()).double())          # [M][K][2r]: the packer's f32 product, rounded to f16
        y = OT.sconv1d(a, wc, _w(net, f"encoder.downsample.{s}.3.conv.conv.bias"), stride=r)
        if film is not None:
            bw = y.shape[1] // cfg.freq_bands
            bands = []
            for b in range(cfg.freq_bands):
                g = F.linear(film, net.w(f"encoder.film_layers.{s}.{b}.gamma_layer.weight"), net.w(f"encoder.film_layers.{s}.{b}.gamma_layer.bias")).double().unsqueeze(-1)
                bt = F.linear(film, net.w(f"encoder.film_layers.{s}.{b}.beta_layer.weight"), net.w(f"encoder.film_layers.{s}.{b}.beta_layer.bias")).double().unsqueeze(-1)
                bands.append(y[:, b * bw:(b + 1) * bw] * g + bt)
            y = torch.cat(bands, dim=1)
        hcur = h(y) if round_last or s + 1 < len(cfg.ratios_enc) else y
        mult *= 2
    return hcur, wav, stride, mult


def spec_post_raw(net, x, f16=True):
    """spec_post's x' (f32 in the kernels) behind the encoder stages: on the f16 pipe (f16=True, the stream rounded to f16 before it) or
    the exact path's spec block on the f32 output of the last downsample unit."""
    cfg = net.cfg
    hcur, wav, stride, mult = encoder_stages(net, x, None, round_last=f16)
    return spec_block_raw(net, "encoder.spec_post", hcur, wav, mult * cfg.n_fft_base, stride, cfg.spec_means[-1], cfg.spec_stds[-1],
                          cfg.res_scale_enc, f16=f16)


def encoder_latent(net, x, msg):
    """SEANetEncoder.forward (seanet.py:883-976) in the mode's arithmetic -> the latent BEFORE L2Norm (f32 in the kernels): spec_post on
    the f16 pipe, its ELU(x') as f16, conv_post16."""
    cfg = net.cfg
    rs = cfg.res_scale_enc
    hcur, wav, stride, mult = encoder_stages(net, x, msg)
    a = spec_block_act(net, "encoder.spec_post", hcur, wav, mult * cfg.n_fft_base, stride, cfg.spec_means[-1], cfg.spec_stds[-1], rs, 1.0)
    wd = _w(net, "encoder.conv_post.1.conv.conv.weight")                                  # [C][1][k] depth-wise, then the 1x1
    pw = _w(net, "encoder.conv_post.2.conv.conv.weight")
    wc = h((pw[:, :, 0, None].float() * wd[None, :, 0, :].float()).double())              # [D][C][k]
    return OT.sconv1d(a, wc, _w(net, "encoder.conv_post.2.conv.conv.bias"))


def decoder_forward(net, lat):
    cfg = net.cfg
    rs = cfg.res_scale_dec
    i0, i1, ups, il = decoder_layout(cfg)
    z = h(F.normalize(lat, p=2.0, dim=1, eps=1e-12) * (lat.shape[1] ** 0.5))
    pw, wd = _w(net, f"decoder.model.{i0}.conv.conv.weight"), _w(net, f"decoder.model.{i1}.conv.conv.weight")
    wc = h((pw[:, :, 0, None].float() * wd[:, 0, None, :].float()).double())
    post = (1 + cfg.n_residual_dec * rs ** 2) ** -0.5
    a = h(F.elu(OT.sconv1d(z, wc, _w(net, f"decoder.model.{i1}.conv.conv.bias"))))                # first upsample: no Scale in front (seanet.py:1104)
    for i, (ct, pwk, res, r, C) in enumerate(ups):
        w_ct, w_pw = _w(net, f"decoder.model.{ct}.convtr.convtr.weight"), _w(net, f"decoder.model.{pwk}.conv.conv.weight")
        bias = _w(net, f"decoder.model.{pwk}.conv.conv.bias")
        Bn, K, Lf = a.shape
        M = w_pw.shape[0]
        prev = torch.cat([torch.zeros(Bn, K, 1, dtype=a.dtype), a[:, :, :-1]], dim=2)
        y = torch.zeros(Bn, M, Lf * r, dtype=torch.float64)
        for p in range(r):                                           # out[m][r l + p] = b + sum_k W[m][k] (ct[k][p] a[k][l] + ct[k][p + r] a[k][l - 1])
            w0 = h((w_pw[:, :, 0].float() * w_ct[None, :, 0, p + r].float()).double())
            w1 = h((w_pw[:, :, 0].float() * w_ct[None, :, 0, p].float()).double())
            y[:, :, p::r] = torch.einsum("mk,bkt->bmt", w0, prev) + torch.einsum("mk,bkt->bmt", w1, a)
        y = y + bias[None, :, None]
        stage_next = post                                            # the next upsample's Scale -> ELU, or the tail's
        if not res:
            a = h(F.elu(y * stage_next))
            continue
        hcur = h(y)
        for j, ri in enumerate(res):
            last = j + 1 == len(res)
            hcur = resnet_block(net, f"decoder.model.{ri}", hcur, j, rs, stage_next if last else None)
        a = hcur
    y = OT.sconv1d(a, _w(net, f"decoder.model.{il}.conv.conv.weight"), _w(net, f"decoder.model.{il}.conv.conv.bias"))
    return torch.tanh(y * cfg.wav_std)


@torch.no_grad()
def embed(net: OT.Net, x, msg):
    """wm = G(x, msg)[..., :T] + x in the f16-operand mode's arithmetic (wv_generator_forward_f16)."""
    x, msg = OT._t(x).double(), OT._t(msg).float()
    return (decoder_forward(net, encoder_latent(net, x, msg))[..., : x.shape[-1]] + x).float()


# ---- the detector and the locator: run_head_model's two tails ----------------------------------------------------------------------
def spec_post16(cfg) -> bool:
    """spec_post (and, for the mean output, conv_post) has an f16 plan: the top stage's width is a multiple of 16 (pack_model)."""
    return (cfg.channels_enc << len(cfg.strides)) % 16 == 0


def head16_gate(cfg) -> bool:
    """run_head_model's head16 gate for the mean-probability output of a net that has an f16 plan: head16_kernel runs iff this holds,
    otherwise the f32 tail does (launch_head16's own limits: D % 16 == 0, D <= 128, nb % 4 == 0, nb <= 32, hop % 32 == 0)."""
    D, nb, hop = cfg.dimension, cfg.head_bits, cfg.hop_length
    return cfg.kind != "generator" and spec_post16(cfg) and D % 16 == 0 and D <= 128 and nb % 4 == 0 and nb <= 32 and hop % 32 == 0


def head_weights(net):
    """The composed head (pack_model): wc[d][bit * hop + j] = sum_o last[bit][o] rev[d][o][j], bc = last @ b_rev + b_last; float64 sums
    rounded to f32 -> (wc [D, nb * hop], bc [nb]) float32."""
    w1 = _w(net, "reverse_convolution.weight")                     # [D][O][hop]
    w2 = _w(net, "last_layer.weight")[:, :, 0]                     # [nb][O]
    wc = torch.einsum("no,doj->dnj", w2, w1).reshape(w1.shape[0], -1).float()
    bc = (w2 @ _w(net, "reverse_convolution.bias") + _w(net, "last_layer.bias")).float()
    return wc, bc


def head16_probs(lat, wc, bc, z16=True, shift=0, inv_ulps=0):
    """head16_kernel's per-sample probabilities, restated: lat [B, D, Fr] f32 (the latent before L2Norm), wc [D, nb * hop], bc [nb].
    z = f16(y * inv), inv = sqrt(D) / max(sqrt(sum_m y_m^2), 1e-12) in the kernel's f32 operations (a sequential fmaf over the channels,
    correctly rounded sqrt / divide / product), W = f16(wc), logits z^T W + bc and the sigmoid in float64, t = frame * hop + j.
    -> numpy float64 [B, nb, Fr * hop].  inv_ulps: inv moved by that many f32 ulps (the GPU's f32 sum of squares / sqrt / divide can
    land an ulp away, and then a z near an f16 rounding midpoint rounds the other way: head16_bounds).  z16 = False (z not rounded) and
    shift != 0 (t = frame * hop + j + shift) are deliberately wrong variants, for the tests' sensitivity checks."""
    y = np.ascontiguousarray(OT._t(lat).float().numpy())
    wc, bc = OT._t(wc).float().numpy(), OT._t(bc).double().numpy()
    B, D, Fr = y.shape
    nb = bc.shape[0]
    hop = wc.shape[1] // nb
    ss = np.zeros((B, Fr), np.float32)
    for m in range(D):
        ss = (y[:, m].astype(np.float64) ** 2 + ss).astype(np.float32)
    inv = np.float32(np.sqrt(np.float32(D))) / np.maximum(np.sqrt(ss), np.float32(1e-12))
    for _ in range(abs(inv_ulps)):
        inv = np.nextafter(inv, np.float32(np.inf if inv_ulps > 0 else -np.inf))
    z = y * inv[:, None, :]
    z = z.astype(np.float16).astype(np.float64) if z16 else (y.astype(np.float64) * inv[:, None, :])
    W = wc.astype(np.float16).astype(np.float64)
    lg = (z.transpose(0, 2, 1) @ W).reshape(B, Fr, nb, hop).transpose(0, 2, 1, 3).reshape(B, nb, Fr * hop) + bc[None, :, None]
    p = 1.0 / (1.0 + np.exp(-lg))
    return np.roll(p, shift, axis=-1) if shift else p


def head16(lat, wc, bc, T: int, keep_lo=None, keep_hi=None, **variant):
    """head16_probs reduced as the kernel reduces them -> torch float64 [B, nb]: the mean over t < T, or with keep_lo / keep_hi (one
    per row) the SUM over t in [keep_lo, keep_hi) and t < T (the windowed mode)."""
    p = head16_probs(lat, wc, bc, **variant)
    t = np.arange(p.shape[-1])
    if keep_lo is None:
        return torch.from_numpy(p[..., :T].sum(-1) / T)
    lo, hi = np.asarray(keep_lo).reshape(-1, 1), np.asarray(keep_hi).reshape(-1, 1)
    keep = (t[None] >= lo) & (t[None] < np.minimum(hi, T))                        # [B, Fr * hop]
    return torch.from_numpy((p * keep[:, None, :]).sum(-1))


def head16_bounds(lat, wc, bc, T: int, keep_lo=None, keep_hi=None, ulps=2):
    """head16 as an interval: per frame the least and the greatest contribution over inv moved by -ulps .. +ulps f32 ulps (one inv per
    frame in the kernel, so the variants never mix inside a frame), summed over the frames -> (lo, hi) numpy float64 [B, nb], the mean or
    the window sum as head16 returns it.  lo == hi except where a frame's z lies within those ulps of an f16 rounding midpoint."""
    lo = hi = None
    for u in range(-ulps, ulps + 1):
        p = head16_probs(lat, wc, bc, inv_ulps=u)
        B, nb, n = p.shape
        t = np.arange(n)
        if keep_lo is None:
            keep = np.broadcast_to(t[None] < T, (B, n))
        else:
            keep = (t[None] >= np.asarray(keep_lo).reshape(-1, 1)) & (t[None] < np.minimum(np.asarray(keep_hi).reshape(-1, 1), T))
        f = (p * keep[:, None, :]).reshape(B, nb, -1, n // (lat.shape[-1])).sum(-1)       # per-frame contributions [B, nb, Fr]
        lo, hi = (f, f) if lo is None else (np.minimum(lo, f), np.maximum(hi, f))
    lo, hi = lo.sum(-1), hi.sum(-1)
    return (lo / T, hi / T) if keep_lo is None else (lo, hi)


@torch.no_grad()
def detect_logits(net: OT.Net, x, round_post: bool = False):
    """The f32 tail (the f16 mode's logits outputs, and its mean output wherever head16_gate is false): spec_post's x' in f32 -- from the
    f16 pipe where the net has that plan --, then the exact path's conv_post, L2Norm and head (detector.py:300-310, 366-391) -> [B, nb, T].
    round_post=True: ELU(x') rounded to f16 as the head16 tail rounds it (a deliberately wrong variant, for the tests' sensitivity checks)."""
    cfg = net.cfg
    x = OT._t(x).double()
    xs = spec_post_raw(net, x, f16=spec_post16(cfg))
    a = h(F.elu(xs)) if round_post else F.elu(xs)
    wd = _w(net, "encoder.conv_post.1.conv.conv.weight")
    y = OT.sconv1d(a, wd, None, groups=wd.shape[0])
    y = OT.sconv1d(y, _w(net, "encoder.conv_post.2.conv.conv.weight"), _w(net, "encoder.conv_post.2.conv.conv.bias"))
    z = F.normalize(y, p=2.0, dim=1, eps=1e-12) * (y.shape[1] ** 0.5)
    w1 = _w(net, "reverse_convolution.weight")
    up = F.conv_transpose1d(z, w1, _w(net, "reverse_convolution.bias"), stride=w1.shape[-1])[..., : x.shape[-1]]
    return F.conv1d(up, _w(net, "last_layer.weight"), _w(net, "last_layer.bias"))


locate = detect_logits


@torch.no_grad()
def detect_mean_prob(net: OT.Net, x):
    """mean_t sigmoid(logits) [B, nb] of the f16 mode's mean-probability output (wv_detector_forward_f16 with logits == NULL): the head16
    tail where head16_gate holds (spec_post -> f16(ELU(x')) -> conv_post16 -> f32 latent -> head16), else the f32 tail's logits."""
    x = OT._t(x).double()
    if head16_gate(net.cfg):
        wc, bc = head_weights(net)
        return head16(encoder_latent(net, x, None), wc, bc, x.shape[-1])
    return torch.sigmoid(detect_logits(net, x)).mean(dim=-1)
