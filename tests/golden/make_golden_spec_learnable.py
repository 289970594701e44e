#!/usr/bin/env python3
"""Generate tests/golden/spec_learnable.npz: gradients of the REFERENCE's learnable STFT bases (Generator.spec_learnable: true,
conf/base.yml; `CausalSTFT(learnable=True)`, modules/conv.py:1023-1024) through its own CPU autograd (build container only).
Only data is written.

Unit cases `u{i}_{dft|noisy}`: CausalSTFT(n_fft, hop, learnable=True) -> the SpecBlock's log clamp and normalisation
(seanet.py:484-494) -> <dP, .> for a seeded dP, in float64.  Two bases per shape: the analytic windowed DFT basis and that basis plus
5 % of its peak as seeded noise on every row (waveverify_amd.init.learned_stft_bases' recipe), so that the sin_0 / sin_{F-1} rows carry
a gradient.  One clip of every case holds exact silence (n_fft + hop samples in its middle, n_fft + 1 where it is too short for that, its first 9/10 where it is no longer than n_fft + 1), so bins under
the clamp (|STFT|^2 <= 1e-10, no gradient) occur; their share is asserted to be positive and below 50 %.  (At T = 1 a clip has one
frame and one sample; its sample is 1.4e-4, which puts some bins of the noisy basis under the clamp and -- every bin of the analytic
basis having the same magnitude there -- all bins of that clip for the analytic one: exactly 50 %, the one case allowed to touch it.)

The cases, their seeded inputs and the stored rows are tests/spec_learnable_cases.py's.  Stored per case: wav and dP (above 48 KB their
sum and sum of squares: the tests rebuild them from the seed); four rows of the noisy basis (sin_0, sin_{F-1}, cos_1, sin_1: the tests
rebuild the bases and check them against these; the analytic one is checkpoint.stft_basis, pinned by dft_basis.npz); dBasis -- float64 in full for n_fft = 64, float32 in full for 128, and for n_fft >= 256 a seeded 32-row subset plus the
sin_0 / sin_{F-1} rows (float64 for 256, float32 for 512 and 1024) together with the whole tensor's peak and Frobenius norm in float64
(a committed file stays under 1 MiB: the three subsets in float64 alone would be 975 KB);
`ref32`: max |float32 autograd - float64 autograd| / max |float64|, the reference's own float32 error on that tensor; the share of
clamped bins.

Net case `net_*`: the reference Generator with its five bases registered as parameters (what SEANetEncoder(spec_learnable=True)
does; see the note in main()) at the shrunk configuration of small_T64 / small_T67, B = 2, T = 64 (the
training units' ResnetBlock needs every stage's length to be a multiple of 4, so 67 cannot run there; ragged lengths are the unit
cases'), two clip_grad_norm_ + AdamW steps on mean|delta| + <r, delta> in float64: both losses, the five basis gradients and the total
gradient norm of step 1, the five bases after each step, and the step-1 basis gradients of the same run in float32.

Usage (from repo root, in the build container):  python tests/golden/make_golden_spec_learnable.py"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (sets sys.path to the repository root as well)
import spec_learnable_cases as SLC  # noqa: E402
from spec_learnable_cases import MEAN, NET, NET_B, NET_LR, NET_MAX_NORM, NET_SEED, NET_T, NOISE_REL, STD, SUBSET_FROM, UNIT_SHAPES, rng  # noqa: E402


def unit_grad(torch, CausalSTFT, n_fft, hop, basis, wav, dP, dtype):
    st = CausalSTFT(n_fft=n_fft, hop_size=hop, pad_mode="constant", learnable=True).to(dtype)
    with torch.no_grad():
        st.weight.copy_(torch.from_numpy(basis).to(dtype)[:, None, :])
    mag = st(torch.from_numpy(wav).to(dtype))
    y = mag.clamp_min(1e-5).log_()
    y.sub_(MEAN).div_(STD)
    (y * torch.from_numpy(dP).to(dtype)).sum().backward()
    return st.weight.grad[:, 0, :].numpy().astype(np.float64), float((mag.detach() <= 1e-5).double().mean())


def main():
    from waveverify_amd.config import default_config
    torch, _, Generator, _, _ = MG._import_reference()
    from modules.conv import CausalSTFT
    torch.set_num_threads(8)
    out = {"mean": np.float64(MEAN), "std": np.float64(STD), "noise_rel": np.float64(NOISE_REL),
           "unit_shapes": np.array(UNIT_SHAPES, dtype=np.int64)}
    for i, (n_fft, hop, B, T) in enumerate(UNIT_SHAPES):
        wav, dP = SLC.unit_inputs(i)
        for name, a in (("wav", wav), ("dP", dP)):
            if a.nbytes <= SLC.STORED_BYTES:
                out[f"u{i}_{name}"] = a
            else:
                out[f"u{i}_{name}_sums"] = SLC.sums(a)
        F = n_fft // 2 + 1
        for tag in ("dft", "noisy"):
            basis = SLC.unit_basis(n_fft, tag)
            g64, share = unit_grad(torch, CausalSTFT, n_fft, hop, basis, wav, dP, torch.float64)
            g32, _ = unit_grad(torch, CausalSTFT, n_fft, hop, basis, wav, dP, torch.float32)
            assert share > 0.0 and (share < 0.5 or (T == 1 and tag == "dft" and share == 0.5)), (n_fft, hop, B, T, tag, share)
            if tag == "noisy":
                assert np.abs(g64[[F, 2 * F - 1]]).max() > 1e-3 * np.abs(g64).max(), "side rows carry no gradient"
            k = f"u{i}_{tag}_"
            out[k + "silent_share"] = np.float64(share)
            out[k + "ref32"] = np.float64(np.abs(g32 - g64).max() / np.abs(g64).max())
            out[k + "peak"], out[k + "fro"] = np.float64(np.abs(g64).max()), np.float64(np.sqrt((g64 ** 2).sum()))
            if n_fft >= SUBSET_FROM:
                rows = SLC.subset_rows(n_fft)
                out[k + "rows"], out[k + "dBasis"] = rows, g64[rows] if n_fft == SUBSET_FROM else g64[rows].astype(np.float32)
            else:
                out[k + "dBasis"] = g64 if n_fft == 64 else g64.astype(np.float32)
            if tag == "noisy":
                out[k + "basis_check"] = basis[SLC.check_rows(n_fft)]
            print(f"u{i} {tag}: n_fft {n_fft} hop {hop} B {B} T {T}: clamped share {share:.3f}, peak {np.abs(g64).max():.3e}, "
                  f"side rows {np.abs(g64[[F, 2 * F - 1]]).max():.3e}, float32 autograd off by {out[k + 'ref32']:.2e}")

    # ---- the whole generator, two optimizer steps ----------------------------------------------------------------------------
    cfg = default_config("generator", **NET)
    r = rng("net")
    x = (0.1 * r.standard_normal((NET_B, 1, NET_T))).astype(np.float32)
    msg = r.integers(0, 2, (NET_B, cfg.nbits)).astype(np.float32)
    rr = (r.standard_normal((NET_B, 1, NET_T)) / (NET_B * NET_T)).astype(np.float32)
    out.update(net_x=x, net_msg=msg, net_r=rr, net_cfg=np.array([repr(dict(NET, seed=NET_SEED, lr=NET_LR, max_norm=NET_MAX_NORM))]))
    from waveverify_amd.init import stft_basis_keys
    keys = list(stft_basis_keys(cfg))
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        from waveverify_amd.init import random_state_dict
        model = Generator(**MG._ref_kwargs(cfg), spec_learnable=True).train()
        sd = random_state_dict(cfg, NET_SEED, parametrized=True)
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(m.endswith("spec.weight") for m in missing), (missing[:5], unexpected[:5])
        # Generator.__init__ takes spec_learnable (model/generator.py:95) but does not hand it to SEANetEncoder (:177-209), so its bases
        # are buffers whatever the flag says; SEANetEncoder(spec_learnable=True) -> CausalSTFT(learnable=True) would register them as
        # nn.Parameter(weight) (seanet.py:721,787, conv.py:1023-1024).  Do exactly that here, on the built modules.
        for mod in model.encoder.modules():
            if isinstance(mod, CausalSTFT) and "weight" in mod._buffers:
                w = mod._buffers.pop("weight")
                mod.weight = torch.nn.Parameter(w.clone())
        model = model.to(dtype)
        # the encoder casts the message to float32 (seanet.py:909): hand the MLP its own dtype back
        model.encoder.msg_embedding.register_forward_pre_hook(lambda m, inp, dtype=dtype: (inp[0].to(dtype),))
        named = dict(model.named_parameters())
        assert all(k in named for k in keys), "spec_learnable=True must make the bases parameters"
        opt = torch.optim.AdamW(model.parameters(), lr=NET_LR, betas=(0.8, 0.99))
        xt, mt, rt = torch.from_numpy(x).to(dtype), torch.from_numpy(msg), torch.from_numpy(rr).to(dtype)
        for step in (1, 2):
            opt.zero_grad()
            delta = model.decode(model.encode(xt, mt))[..., :NET_T]
            loss = delta.abs().mean() + (rt * delta).sum()
            loss.backward()
            if step == 1:
                for k in keys:
                    out[f"net_{tag}_g:{k}"] = named[k].grad.numpy().astype(np.float64 if dtype == torch.float64 else np.float32)
                    assert float(named[k].grad.abs().max()) > 0.0, k
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), NET_MAX_NORM)
            opt.step()
            if dtype == torch.float64:
                out[f"net_loss{step}"] = np.float64(float(loss))
                if step == 1:
                    out["net_grad_norm"] = np.float64(float(norm))
                    out["net_delta1"] = delta.detach().numpy().astype(np.float32)
                for k in keys:
                    out[f"net_basis{step}:{k}"] = named[k].detach().numpy().astype(np.float64)
        if dtype == torch.float64:
            print(f"net: losses {out['net_loss1']:.6e} {out['net_loss2']:.6e}, grad norm {out['net_grad_norm']:.6e}")
    for k in keys:
        g64, g32 = out[f"net_f64_g:{k}"], out[f"net_f32_g:{k}"].astype(np.float64)
        print(f"net {k}: peak {np.abs(g64).max():.3e}, float32 autograd off by {np.abs(g32 - g64).max() / np.abs(g64).max():.2e}")
    path = os.path.join(HERE, "spec_learnable.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
