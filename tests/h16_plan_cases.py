"""The launch-plan cases shared by tests/test_gpu_h16_plan.py and tests/golden/make_golden_h16_plan.py: which kernels, under which roles and how
many times, every net-level entry point launches in both precision modes -- or how it refuses.  No numeric test sees a stage of the f16 plan
that falls to its slower route without saying so; these rows do.

A case is (net id, T); B = 2.  Nets: the three defaults, the six configurations of test_gpu_h16's sweep (all three kinds each), a detector
with 36 bits (outside head16's limits: the f16 encoder with the f32 tail) and a detector and a generator with 16 base channels (no f16 plan:
the f16 entry points refuse)."""
from __future__ import annotations

import re

B = 2
LENGTHS = (1600, 801)


def net_configs():
    """{net id: NetConfig}, in a fixed order."""
    from waveverify_amd.config import default_config
    from test_gpu_h16 import _other_configuration
    out = {k: default_config(k) for k in ("generator", "detector", "locator")}
    for seed in range(6):
        gkw, kw, _ = _other_configuration(seed)
        out[f"sweep{seed}.generator"] = default_config("generator", **gkw)
        out[f"sweep{seed}.detector"] = default_config("detector", **kw)
        out[f"sweep{seed}.locator"] = default_config("locator", **kw)
    out["nbits36.detector"] = default_config("detector", nbits=36)
    out["narrow16.detector"] = default_config("detector", channels_enc=16)
    out["narrow16.generator"] = default_config("generator", channels_enc=16)
    return out


def calls(net, x, msg):
    """{call id: thunk(precision) -> tensor} for one HipNet on the clips x [B,1,T] (msg [B,16] for a generator)."""
    import torch
    kind, T = net.cfg.kind, x.shape[-1]
    if kind == "generator":
        return {"generator": lambda p: net.generator(x, msg, add_input=True, precision=p)}
    if kind == "locator":
        return {"locator": lambda p: net.locator(x, precision=p)}
    lo = torch.tensor([0, T // 4], dtype=torch.int32)
    hi = torch.tensor([T - T // 3, T], dtype=torch.int32)
    gate = torch.sin(torch.arange(B * T, dtype=torch.float32, device=x.device) * 0.37).reshape(B, T)
    return {
        "detector": lambda p: net.detector(x, precision=p),
        "detector_mean_prob": lambda p: net.detector_mean_prob(x, precision=p),
        "detector_window_psum": lambda p: net.detector_window_psum(x, lo, hi, precision=p),
        "detector_frame_sums": lambda p: net.detector_frame_sums(x, precision=p),
        "detector_frame_sums.gated": lambda p: net.detector_frame_sums(x, gate=gate, gate_thr=0.25, precision=p),
    }


def run_net(net_id, cfg, keep_outputs=False):
    """Every call of one net at both lengths and precisions -> {"<net id>/T<T>/<call>/<precision>": record}; a record is
    {"rows": sorted [[kernel|role, launches], ...]} or {"refused": code, "error": [exception type, message]}, plus "workspace_bytes" once
    per (net, T) under "<net id>/T<T>".  keep_outputs: also "output" (a CPU tensor) in every record that ran."""
    import torch
    from waveverify_amd import profile
    from waveverify_amd.init import random_state_dict, synthetic_clips
    from waveverify_amd.nets import HipNet
    net = HipNet(cfg, random_state_dict(cfg, 7))
    out = {}
    for T in LENGTHS:
        x_np, msg_np = synthetic_clips(B, T, seed=11)
        x, msg = torch.from_numpy(x_np).cuda(), torch.from_numpy(msg_np).cuda()
        out[f"{net_id}/T{T}"] = {"workspace_bytes": int(net._lib.wv_workspace_bytes(net._h, B, T))}
        for call_id, thunk in calls(net, x, msg).items():
            for precision in ("f32", "f16"):
                profile.enable(True)
                profile.reset()
                try:
                    y = thunk(precision)
                    torch.cuda.synchronize()
                    rec = {"rows": sorted([e["name"], int(e["launches"])] for e in profile.collect())}
                    if keep_outputs:
                        rec["output"] = y.cpu()
                except RuntimeError as e:
                    code = re.search(r"failed \(code (-?\d+)\)", str(e))
                    if not code:                                 # not the library's refusal (a HIP fault surfaces here too): stop
                        raise
                    rec = {"refused": int(code.group(1)), "error": [type(e).__name__, str(e)]}
                finally:
                    profile.enable(False)
                out[f"{net_id}/T{T}/{call_id}/{precision}"] = rec
    return out
