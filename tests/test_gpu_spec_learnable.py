"""Training the generator's STFT bases on the GPU (spec_learnable): wv_stft_plan_basis_grad against the reference's float64 autograd
(tests/golden/spec_learnable.npz, cases of tests/spec_learnable_cases.py), wv_stft_plan_set_basis_device against host-made plans, and
GeneratorTrainer / WatermarkTrainer with the switch on (gradients, two optimizer steps, checkpoint round trip and resume) and off.

Gradient bar: 1e-4 of the tensor's largest magnitude, for every unit case and for the net case."""
import ast

import numpy as np
import pytest
import torch

import spec_learnable_cases as SLC
from guard import Guards
from waveverify_amd.config import default_config
from waveverify_amd.init import random_state_dict, stft_basis_keys

pytestmark = pytest.mark.gpu

CASES = [(i, v) for i in range(len(SLC.UNIT_SHAPES)) for v in SLC.VARIANTS]
BAR = 1e-4


def LOSS_BAR(g):
    """The net case's loss is mean|delta| + <r, delta>: an error of at most e in every sample of delta moves it by at most
    (1 + sum|r|) e, and e = 2e-5 is the bar the generator tests hold the watermarked audio to."""
    return (1.0 + float(np.abs(g["net_r"]).sum())) * 2e-5


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def fixture():
    return np.load(SLC.FIXTURE)


@pytest.mark.parametrize("i,variant", CASES)
def test_basis_gradient_vs_reference_autograd(fixture, i, variant):
    """dBasis of every unit case: the stored rows against the reference's float64 autograd, ALL rows against the float64 formula
    (pinned to that autograd by test_spec_learnable_cpu.py), the side rows sin_0 / sin_{F-1} on their own; twice, bit for bit."""
    from waveverify_amd.train import StftFeatures
    c = SLC.load_unit(fixture, i, variant)
    n, F = c["n_fft"], c["n_fft"] // 2 + 1
    st = StftFeatures(n, c["hop"], SLC.MEAN, SLC.STD, basis=c["basis"])
    wav, dP = _cu(c["wav"]), _cu(c["dP"])
    runs = []
    for _ in range(2):
        d = torch.full((2 * F, 1, n), float("nan"), device="cuda")
        st.basis_grad(wav, dP, d)
        runs.append(d)
    assert torch.equal(runs[0], runs[1])
    got = runs[0][:, 0].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    sub = got if c["rows"] is None else got[c["rows"]]
    e_ref = float(np.abs(sub - c["dBasis"]).max()) / c["peak"]
    full, _ = SLC.formula_grad(c["basis"], c["wav"], c["dP"], n, c["hop"])
    e_all = float(np.abs(got - full).max()) / c["peak"]
    e_side = float(np.abs(got[[F, 2 * F - 1]] - full[[F, 2 * F - 1]]).max()) / c["peak"]
    side_scale = max(float(np.abs(full[[F, 2 * F - 1]]).max()), 1e-30)
    e_side_own = float(np.abs(got[[F, 2 * F - 1]] - full[[F, 2 * F - 1]]).max()) / side_scale
    print(f"MEASURE basis gradient u{i} {variant} (n_fft {n}, hop {c['hop']}, B {c['B']}, T {c['T']}): stored rows {e_ref:.2e}, all rows {e_all:.2e}, "
          f"side rows {e_side:.2e} of the peak / {e_side_own:.2e} of their own; reference float32 autograd {c['ref32']:.2e}")
    assert e_ref <= BAR and e_all <= BAR and e_side <= BAR
    if variant == "noisy":                                     # there the side rows are ordinary rows with a gradient of their own size
        assert e_side_own <= BAR
    assert abs(float(np.abs(got).max()) - c["peak"]) <= BAR * c["peak"] and abs(float(np.sqrt((got ** 2).sum())) - c["fro"]) <= BAR * c["fro"]


@pytest.mark.parametrize("offset", [0, 1])
def test_basis_gradient_guard_bands_and_poisoned_workspace(fixture, offset):
    """One ragged case (n_fft 128, hop 2, T 131, noisy basis) with every operand between guard bands, aligned and one float off, and
    exactly the promised workspace filled with NaN bytes: nothing outside is touched, nothing stale is read, every element written."""
    from waveverify_amd import _lib
    from waveverify_amd.train import StftFeatures
    c = SLC.load_unit(fixture, 2, "noisy")
    n, F = c["n_fft"], c["n_fft"] // 2 + 1
    st = StftFeatures(n, c["hop"], SLC.MEAN, SLC.STD, basis=c["basis"])
    lib = _lib.load()
    ref = torch.empty(2 * F, n, device="cuda")
    st.basis_grad(_cu(c["wav"]), _cu(c["dP"]), ref)
    g = Guards(offset=offset)
    wav, dP, out = g.input(c["wav"], "wav"), g.input(c["dP"], "dP"), g.output((2 * F, n), name="dBasis")
    ws = g.workspace(int(lib.wv_stft_plan_basis_grad_workspace_bytes(st._h, c["B"], c["T"], c["hop"])))
    for _ in range(2):
        g.repoison()
        assert lib.wv_stft_plan_basis_grad(st._h, wav.t.data_ptr(), dP.t.data_ptr(), out.t.data_ptr(), c["B"], c["T"], c["hop"], SLC.STD,
                                           ws.t.data_ptr(), ws.t.numel(), _lib.stream()) == 0
        g.check()
        assert torch.isfinite(out.t).all()
        d = float((out.t - ref).abs().max())
        assert torch.equal(out.t, ref) if offset == 0 else d <= BAR * c["peak"], d     # one float off: the scalar-load path of the GEMM
    assert lib.wv_stft_plan_basis_grad(st._h, wav.t.data_ptr(), dP.t.data_ptr(), out.t.data_ptr(), c["B"], c["T"], c["hop"], SLC.STD,
                                       ws.t.data_ptr(), ws.t.numel() - 1, _lib.stream()) != 0          # a short workspace is refused


@pytest.mark.parametrize("n_fft,hop", [(64, 1), (256, 8), (1024, 320)])
def test_plan_refreshed_on_the_device_equals_a_host_made_plan(n_fft, hop):
    """A plan created from basis A and refreshed to B on the device gives the features and gradients, bit for bit, of a plan created from B."""
    from waveverify_amd.train import StftFeatures
    a, b = SLC.unit_basis(n_fft, "dft"), SLC.unit_basis(n_fft, "noisy")
    T = 2000 + hop + 3
    wav = _cu((0.1 * SLC.rng(f"refresh/{n_fft}").standard_normal((2, 1, T))).astype(np.float32))
    host, dev = StftFeatures(n_fft, hop, SLC.MEAN, SLC.STD, basis=b), StftFeatures(n_fft, hop, SLC.MEAN, SLC.STD, basis=a)
    P_host = host(wav)
    assert not torch.equal(dev(wav), P_host)
    dev.set_basis_device(_cu(b).reshape(n_fft + 2, 1, n_fft))
    assert torch.equal(dev(wav), P_host)
    dP = torch.randn(P_host.shape, generator=torch.Generator().manual_seed(n_fft)).cuda()
    dw = [torch.zeros_like(wav), torch.zeros_like(wav)]
    db = [torch.empty(n_fft + 2, n_fft, device="cuda"), torch.empty(n_fft + 2, n_fft, device="cuda")]
    for k, st in enumerate((host, dev)):
        st.backward(wav, dP, dw[k], accumulate=False)
        st.basis_grad(wav, dP, db[k])
    assert torch.equal(dw[0], dw[1]) and torch.equal(db[0], db[1])
    dev.set_basis_device(_cu(a))                                         # and back
    assert torch.equal(dev(wav), StftFeatures(n_fft, hop, SLC.MEAN, SLC.STD, basis=a)(wav))


def _net(fixture, **kw):
    from waveverify_amd.train import GeneratorTrainer
    c = ast.literal_eval(str(fixture["net_cfg"][0]))
    seed, lr, max_norm = c.pop("seed"), c.pop("lr"), c.pop("max_norm")
    cfg = default_config("generator", **c)
    return cfg, GeneratorTrainer(cfg, random_state_dict(cfg, seed, parametrized=True), lr=lr, max_norm=max_norm, **kw)


def _net_step(tr, g):
    """One step of the net case's objective mean|delta| + <r, delta>: (loss, gradient norm)."""
    x, msg, r = _cu(g["net_x"]), _cu(g["net_msg"]), _cu(g["net_r"])
    delta = tr.forward(x, msg) - x
    loss = float(delta.double().abs().mean() + (r.double() * delta.double()).sum())
    tr.backward(torch.sign(delta) / delta.numel() + r)
    return loss, delta


def test_generator_basis_gradients_vs_reference_autograd(fixture):
    """GeneratorTrainer(spec_learnable=True) on the reference's generator with its bases as parameters: loss, every basis gradient and
    the total gradient norm of step 1."""
    g = fixture
    cfg, tr = _net(g, spec_learnable=True)
    keys = list(stft_basis_keys(cfg))
    assert all(k in tr.params and k in tr.ranges for k in keys)
    loss, delta = _net_step(tr, g)
    assert float(np.abs(delta.cpu().numpy() - g["net_delta1"]).max()) <= 2e-5
    assert abs(loss - float(g["net_loss1"])) <= LOSS_BAR(g)
    for k in keys:
        ref, r32 = g["net_f64_g:" + k], g["net_f32_g:" + k].astype(np.float64)
        got = tr.gviews[k].cpu().numpy().astype(np.float64)
        peak = float(np.abs(ref).max())
        e, e32 = float(np.abs(got - ref).max()) / peak, float(np.abs(r32 - ref).max()) / peak
        print(f"MEASURE net basis gradient {k}: {e:.2e} of the peak {peak:.2e}; reference float32 autograd {e32:.2e}")
        assert e <= BAR, (k, e)
    norm = tr.apply_gradients()
    assert abs(float(norm.item()) - float(g["net_grad_norm"])) <= 5e-4 * float(g["net_grad_norm"])      # the generator tests' bar for the norm


def test_two_optimizer_steps_move_the_bases_and_the_plans(fixture):
    """Two clip + AdamW steps: the bases after each step within 1e-6 of the reference's and both losses right.  That the forward
    runs on the REFRESHED plans is shown bit for bit: it equals the forward of a trainer built (host-packed plans) from the stepped
    state dict, and differs from that of one built from the same weights with the initial bases."""
    g = fixture
    cfg, tr = _net(g, spec_learnable=True)
    keys = list(stft_basis_keys(cfg))
    # (The 1e-6 bar on the bases is weak on its own: AdamW's first step moves an entry by about lr * sign(g) whatever |g| is, so it
    # mostly checks the gradient's sign, the hyper-parameters and that the bases are stepped at all.  The gradient's size is the
    # previous test's business, the plan refresh the bit-level comparison's at the end of this one.)
    l1, _ = _net_step(tr, g)
    tr.apply_gradients()
    for k in keys:
        assert float(np.abs(tr.params[k].cpu().numpy().astype(np.float64) - g["net_basis1:" + k]).max()) <= 1e-6, k
    l2, _ = _net_step(tr, g)
    tr.apply_gradients()
    print(f"MEASURE net losses {l1:.8e} {l2:.8e} vs reference {float(g['net_loss1']):.8e} {float(g['net_loss2']):.8e}")
    assert abs(l1 - float(g["net_loss1"])) <= LOSS_BAR(g) and abs(l2 - float(g["net_loss2"])) <= LOSS_BAR(g)
    for k in keys:
        assert float(np.abs(tr.params[k].cpu().numpy().astype(np.float64) - g["net_basis2:" + k]).max()) <= 1e-6, k
    sd = tr.state_dict()
    for k in keys:
        assert torch.equal(sd[k], tr.params[k].cpu()) and sd[k].shape[1] == 1
    # the plans ARE the arena's bases: a trainer built from this state dict (host-packed plans) gives the same forward, bit for bit
    from waveverify_amd.train import GeneratorTrainer
    tr2 = GeneratorTrainer(cfg, {k: v.numpy() for k, v in tr.state_dict(parametrized=True).items()}, spec_learnable=True)
    x, msg = _cu(g["net_x"]), _cu(g["net_msg"])
    wm = tr.forward(x, msg)
    assert torch.equal(wm, tr2.forward(x, msg))
    stale = {k: v.numpy() for k, v in tr.state_dict(parametrized=True).items() if not k.endswith("spec.weight")}
    assert not torch.equal(wm, GeneratorTrainer(cfg, stale, spec_learnable=True).forward(x, msg))


def test_off_is_off(fixture):
    """spec_learnable=False (the default): the arenas hold exactly the tensors of params.param_specs, the bases are not in them and
    are bit-unchanged by a step; their gradient is nowhere."""
    from waveverify_amd.checkpoint import stft_basis
    from waveverify_amd.params import param_specs
    g = fixture
    cfg, tr = _net(g)
    cfg_on, on = _net(g, spec_learnable=True)
    keys = list(stft_basis_keys(cfg))
    n_wn = sum(1 for _, _, role in param_specs(cfg) if role == "wn")
    assert len(tr.params) == len(list(param_specs(cfg))) + n_wn                     # a weight-normed tensor is two arena entries (g, v)
    assert set(tr.params) == set(random_state_dict(cfg, 0, parametrized=True)) and set(on.params) == set(tr.params) | set(keys)
    assert on.arena.numel() == tr.arena.numel() + sum((n + 2) * n for n in stft_basis_keys(cfg).values())
    assert not any(k.endswith("spec.weight") for k in tr.params) and not tr.spec_learnable
    _net_step(tr, g)
    tr.apply_gradients()
    sd = tr.state_dict()
    for k, n in stft_basis_keys(cfg).items():
        assert torch.equal(sd[k], stft_basis(n)), k
    # and the switch changes nothing else: the other parameters' gradients of step 1 are the same with it on
    _net_step(on, g)
    tr2 = _net(g)[1]
    _net_step(tr2, g)
    for k in tr2.gviews:
        assert torch.equal(tr2.gviews[k], on.gviews[k]), k


def test_detector_and_locator_refuse_the_switch():
    from waveverify_amd.train import EncoderNetTrainer
    for kind in ("detector", "locator"):
        cfg = default_config(kind, channels_enc=8, dimension=16, strides=[2, 2], n_fft_base=16, output_dim=8)
        with pytest.raises(ValueError, match=kind.capitalize()):
            EncoderNetTrainer(cfg, random_state_dict(cfg, 0, parametrized=True), spec_learnable=True)
        EncoderNetTrainer(cfg, random_state_dict(cfg, 0, parametrized=True), spec_learnable=False)


def test_checkpoint_round_trip_and_resume(tmp_path):
    """WatermarkTrainer(spec_learnable=True): 2 steps -> save_checkpoint -> the config says Generator.spec_learnable: True, the file
    holds the trained bases, WaveVerify(path).embed equals the trainer's forward to 2e-6; then the live layout ->
    from_checkpoint(spec_learnable=True): bases, their AdamW moments and the step count are back and the next step is bit-equal."""
    from waveverify_amd import WaveVerify
    from waveverify_amd.checkpoint import load_checkpoint, stft_basis
    from waveverify_amd.train import WatermarkTrainer
    small = dict(channels_enc=16, dimension=32)
    cfgs = [default_config("generator", channels_dec=16, n_residual_dec=1, **small), default_config("detector", **small), default_config("locator")]
    sds = [random_state_dict(c, 3, parametrized=True) for c in cfgs]
    rng = np.random.default_rng(9)
    x = _cu((0.1 * rng.standard_normal((2, 1, 4800))).astype(np.float32))
    msg = _cu(rng.integers(0, 2, (2, 16)).astype(np.float32))
    a = WatermarkTrainer(cfgs[0], sds[0], cfgs[1], sds[1], cfgs[2], sds[2], lr=5e-4, spec_learnable=True)
    assert a.G.spec_learnable and not a.D.spec_learnable and not a.L.spec_learnable
    np.random.seed(0); torch.manual_seed(0)
    for _ in range(2):
        a.step(x, msg)
    keys = stft_basis_keys(cfgs[0])
    path = a.save_checkpoint(tmp_path / "stripped", "best")
    ck = torch.load(str(path), map_location="cpu", weights_only=True)
    assert ck["config"]["Generator.spec_learnable"] is True and "Detector.spec_learnable" not in ck["config"]
    for k, n in keys.items():
        assert torch.equal(ck["models"]["generator"][k], a.G.params[k].cpu())
        assert float((ck["models"]["generator"][k] - stft_basis(n)).abs().max()) > 1e-4            # trained: two steps at lr 5e-4
        assert torch.equal(ck["models"]["detector"][k], stft_basis(n))                              # the detector's stay buffers
    _, cfgs2 = load_checkpoint(tmp_path / "stripped")
    assert cfgs2["generator"].to_dict() == cfgs[0].to_dict()
    wm_t = a.G.forward(x, msg)
    assert float((WaveVerify(str(tmp_path / "stripped")).embed_batch(x, msg) - wm_t).abs().max()) <= 2e-6
    a.save_checkpoint(tmp_path / "live", "latest", parametrized=True)
    b = WatermarkTrainer.from_checkpoint(tmp_path / "live", lr=5e-4, spec_learnable=True)
    assert b.G.opt.t == 2 and set(b.G.ranges) == set(a.G.ranges)
    for k in a.G.ranges:
        (lo, hi), (lo2, hi2) = a.G.ranges[k], b.G.ranges[k]
        assert torch.equal(a.G.arena[lo:hi], b.G.arena[lo2:hi2]) and torch.equal(a.G.opt.m[lo:hi], b.G.opt.m[lo2:hi2]) and torch.equal(a.G.opt.v[lo:hi], b.G.opt.v[lo2:hi2]), k
    assert all(float(b.G.opt.v[slice(*b.G.ranges[k])].abs().max()) > 0.0 for k in keys)             # the bases' moments came back
    for tr in (a, b):
        np.random.seed(5); torch.manual_seed(5)
        tr.step(x, msg)
    for k in a.G.ranges:
        assert torch.equal(a.G.arena[slice(*a.G.ranges[k])], b.G.arena[slice(*b.G.ranges[k])]), k
    assert torch.equal(a.D.arena, b.D.arena) and torch.equal(a.L.arena, b.L.arena)
