"""villandiffusion_amd.defense_ve on the GPU: vd_score_inv_objective against float64, the inversion and removal objectives against the CPU oracle
(NCSNppRef autograd), invert_trigger / remove_backdoor / backdoor_features end to end on a small NCSN++, and the three tools in a child process."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.ncsnpp_ref import NCSNppRef  # noqa: E402
from villandiffusion_amd import defense_ve, mitigation, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=16, block_out_channels=(32, 64, 64),
             down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
             up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)
SIGMA = 380.0

# Measured on the MI355X (the [parity] lines): vd_score_inv_objective's worst loss / dout / dtau_direct errors over the nine cases are
# 6.2e-8 / 1.6e-7 / 1.7e-7; the gate is 10x the worst of them (tighter than an exact-f32 kernel's 1e-5).
OBJECTIVE_GATE = 1.7e-6


def g(seed):
    return torch.Generator().manual_seed(seed)


def _perturb_norms(ref):
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))


def _sched(sigma_max=SIGMA):
    return S.ScoreSdeVeScheduler(num_train_timesteps=2000, sigma_min=0.01, sigma_max=sigma_max, snr=0.075)


@pytest.fixture(scope="module")
def pair():
    torch.manual_seed(1)
    ref = NCSNppRef(**SMALL)
    _perturb_norms(ref)
    net = NCSNppModel(**SMALL)
    net.load_state_dict(ref.state_dict())
    return ref, net


# ------------------------------------------------------------------------------------------------------------ 1. the objective kernel
def _objective(s, tau, sigma, lam):
    loss = torch.empty(1, device=DEV)
    dout = torch.full(s.shape, float("nan"), device=DEV)
    dtau = torch.full_like(tau, float("nan"))
    partial = torch.empty(1024, device=DEV)
    ops.score_inv_objective(s, tau, sigma, lam, loss, dout, dtau, partial)
    torch.cuda.synchronize()
    return loss, dout, dtau


@pytest.mark.parametrize("B", [1, 4, 100])
@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 64, 64), (5, 7, 9)])
def test_objective_kernel_against_float64(B, shape):
    lam, sigma = 0.5, SIGMA
    s = torch.randn((B,) + shape, generator=g(B)) / sigma                     # a score at this noise level: n = -sigma * s is of unit size
    tau = torch.rand(shape, generator=g(B + 1))
    s64 = s.double().requires_grad_(True)
    t64 = tau.double().requires_grad_(True)
    r = (-sigma * s64).mean(0) - lam * t64
    L = r.norm()
    L.backward()
    dtau_direct = -lam * r.detach() / L.detach()
    assert torch.allclose(t64.grad, dtau_direct)
    dout_ref = sigma * s64.grad                                               # pre-multiplied by dx/dtau = sigma
    loss, dout, dtau = _objective(s.to(DEV), tau.to(DEV), sigma, lam)
    e_loss = abs(float(loss) - L.item()) / L.item()
    e_dout = float((dout.double().cpu() - dout_ref).abs().max() / dout_ref.abs().max())
    e_dtau = float((dtau.double().cpu() - dtau_direct).abs().max() / dtau_direct.abs().max())
    print(f"[parity] score-inversion objective B={B} {shape}: loss {e_loss:.2e}, dout {e_dout:.2e}, dtau_direct {e_dtau:.2e}")
    assert e_loss <= OBJECTIVE_GATE and e_dout <= OBJECTIVE_GATE and e_dtau <= OBJECTIVE_GATE
    again = _objective(s.to(DEV), tau.to(DEV), sigma, lam)
    assert torch.equal(again[0], loss) and torch.equal(again[1], dout) and torch.equal(again[2], dtau)     # fixed summation order


def test_objective_kernel_zero_residual_and_strided_input():
    lam, sigma = 0.5, 2.0
    tau = torch.rand(3, 32, 32, generator=g(3)) * 2          # lam * tau, its division by sigma = 2 and the mean of 4 equal images are all exact
    s = (-(lam * tau) / sigma).expand(4, 3, 32, 32).contiguous()
    loss, dout, dtau = _objective(s.to(DEV), tau.to(DEV), sigma, lam)
    assert float(loss) == 0.0 and float(dout.abs().max()) == 0.0 and float(dtau.abs().max()) == 0.0       # no NaN
    buf = torch.randn(4, 8, 32, 32, generator=g(4)).to(DEV)
    a = _objective(buf[:, 2:5], tau.to(DEV), SIGMA, lam)
    b = _objective(buf[:, 2:5].contiguous(), tau.to(DEV), SIGMA, lam)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and float(a[0]) > 0


# ------------------------------------------------------------------------------------------------------------ 2. against the oracle
def _oracle_objective(ref, tau, eps, sigma, lam):
    tr = tau.clone().requires_grad_(True)
    sig = torch.full((eps.shape[0],), sigma)
    n = -sigma * ref(sigma * (eps + tr), sig)[0]
    L = (n.mean(0) - lam * tr).norm()
    L.backward()
    ref.zero_grad()
    return L.item(), tr.grad


@pytest.mark.parametrize("sigma", [380.0, 50.0])
def test_inversion_objective_matches_oracle(pair, sigma):
    """Gates: the VP test's -- loss 1e-5 relative, dtau 1e-3 of its largest entry."""
    ref, net = pair
    B, lam = 4, 0.5
    eps = torch.randn(B, 3, 16, 16, generator=g(5))
    tau = torch.rand(3, 16, 16, generator=g(6))
    L_ref, dtau_ref = _oracle_objective(ref, tau, eps, sigma, lam)
    flags = [p.requires_grad for p in net.parameters()]
    sentinel = (torch.arange(net.flat_grad.numel(), device=DEV, dtype=torch.float32) % 127.0) - 63.0
    net.flat_grad.copy_(sentinel)
    try:
        loss, dtau = defense_ve.inversion_objective(net, tau.to(DEV), eps.to(DEV), sigma, lam)
        assert [p.requires_grad for p in net.parameters()] == flags and net._input_grad is False
        assert torch.equal(net.flat_grad, sentinel)
    finally:
        net.zero_grad()
    e_loss = abs(float(loss) - L_ref) / L_ref
    e_g = float((dtau.double().cpu() - dtau_ref.double()).abs().max() / dtau_ref.double().abs().max())
    print(f"[parity] VE inversion_objective sigma={sigma:g}: L={float(loss):.4f} (oracle {L_ref:.4f}, rel {e_loss:.2e}); dtau rel_err {e_g:.2e} "
          f"(max|dtau_ref| {float(dtau_ref.abs().max()):.3e})")
    assert e_loss <= 1e-5 and e_g <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 3. inversion end to end
@pytest.mark.parametrize("sigma", [380.0, 50.0])
def test_invert_trigger_end_to_end(pair, sigma):
    """On the oracle alone (Adam lr 0.1 from tau0 = rand(seed 3), this noise) the loss goes 14.32 -> 7.27 at sigma 380 and 13.83 -> 7.00 at 50."""
    ref, net = pair
    steps, batch = 8, 4
    noise = torch.randn(steps, batch, 3, 16, 16, generator=g(7))
    sched = _sched(sigma)
    sched.set_sigmas(5)                                                       # an inference table left behind by a pipeline: not what sigma_T is read from
    sentinel = (torch.arange(net.flat_grad.numel(), device=DEV, dtype=torch.float32) % 127.0) - 63.0
    net.flat_grad.copy_(sentinel)
    flags = [p.requires_grad for p in net.parameters()]
    try:
        res = defense_ve.invert_trigger(net, sched, steps=steps, batch=batch, seed=3, noise=noise)
        assert [p.requires_grad for p in net.parameters()] == flags and net._input_grad is False
        assert torch.equal(net.flat_grad, sentinel)
        assert len(res.losses) == steps and all(math.isfinite(x) for x in res.losses)
        print(f"[inversion] VE sigma={sigma:g} losses {['%.4f' % x for x in res.losses]}, ||tau|| {res.trigger_norm:.3f}")
        assert res.losses[-1] < res.losses[0]
        assert res.timestep == 1999 and tuple(res.trigger.shape) == (3, 16, 16) and abs(res.extra["sigma"] - sigma) <= 1e-4 * sigma
        res2 = defense_ve.invert_trigger(net, sched, steps=steps, batch=batch, seed=3, noise=lambda i: noise[i])
        assert res2.losses == res.losses and torch.equal(res2.trigger, res.trigger)
        if sigma == SIGMA:
            # a pipeline is accepted for its scheduler; device noise (Philox): reproducible for the same seed, different for another
            pipe = P.ScoreSdeVePipeline(net, sched)
            a = defense_ve.invert_trigger(net, pipe, steps=2, batch=batch, seed=11)
            b = defense_ve.invert_trigger(net, sched, steps=2, batch=batch, seed=11)
            c = defense_ve.invert_trigger(net, sched, steps=2, batch=batch, seed=12)
            assert a.losses == b.losses and torch.equal(a.trigger, b.trigger) and a.losses != c.losses
            # flags and the switch come back after an exception inside the loop too
            with pytest.raises(ValueError):
                defense_ve.invert_trigger(net, sched, steps=2, batch=batch, noise=lambda i: noise[i][:1])
            assert [p.requires_grad for p in net.parameters()] == flags and net._input_grad is False
            # a lower noise level of the training table
            low = defense_ve.invert_trigger(net, sched, steps=1, batch=batch, seed=3, timestep=1000)
            assert low.timestep == 1000 and 0.01 < low.extra["sigma"] < sigma and math.isfinite(low.losses[0])
    finally:
        net.zero_grad()


# ------------------------------------------------------------------------------------------------------------ 4. removal against the oracle
@pytest.mark.parametrize("math_mode", ["bf16x3", "f32"])
def test_removal_objective_matches_oracle(math_mode):
    """Gates: the VP test's -- terms 1e-5, gradient norm 1e-4, worst parameter gradient 1e-3 of the parameter's own scale."""
    torch.manual_seed(0)
    ref = NCSNppRef(**SMALL)
    _perturb_norms(ref)
    ref_frozen = copy.deepcopy(ref)
    _perturb_norms(ref_frozen)                                  # teacher != student: no term is near zero
    ref_frozen.requires_grad_(False)
    net, frozen = NCSNppModel(**SMALL), NCSNppModel(**SMALL)
    net.load_state_dict(ref.state_dict())
    frozen.load_state_dict(ref_frozen.state_dict())
    net.conv_math = frozen.conv_math = math_mode
    B, wc, ws, sigma = 4, 1.0, 0.5, SIGMA
    eps = torch.randn(B, 3, 16, 16, generator=g(5))
    tau = torch.rand(3, 16, 16, generator=g(6))
    sig = torch.full((2 * B,), sigma)
    with torch.no_grad():
        y = -sigma * ref_frozen(sigma * eps, sig[:B])[0]
    e = -sigma * ref(sigma * torch.cat([eps, eps + tau]), sig)[0]
    clean, shift = ((e[:B] - y) ** 2).mean(), ((e[B:] - y) ** 2).mean()
    (wc * clean + ws * shift).backward()
    want = torch.stack([wc * clean + ws * shift, clean, shift]).detach().double()
    frozen_before = frozen.flat_param.clone()
    flags = [p.requires_grad for p in net.parameters()]
    net.zero_grad()
    terms = defense_ve.removal_objective(net, frozen, tau.to(DEV), eps.to(DEV), sigma, wc, ws)
    assert [p.requires_grad for p in net.parameters()] == flags and not net.time_proj.weight.requires_grad and sum(flags) == len(flags) - 1
    assert torch.equal(frozen.flat_param, frozen_before)
    e_t = float(((terms.double().cpu() - want).abs() / want.abs()).max())
    gref = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    gmax = max(float(v.abs().max()) for v in gref.values())
    worst = (0.0, "")
    for n, p in net.named_parameters():
        if n not in gref:
            continue
        a, b = p.grad.detach().double().cpu(), gref[n].double()
        err = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))
        if err > worst[0]:
            worst = (err, n)
    gn_ref = float(torch.sqrt(sum((v.double() ** 2).sum() for v in gref.values())))
    gn = float(torch.sqrt((net.flat_grad.double() ** 2).sum()))
    e_gn = abs(gn - gn_ref) / gn_ref
    print(f"[parity] VE removal_objective ({math_mode}): terms {[('%.5f' % v) for v in terms.tolist()]} (oracle {[('%.5f' % v) for v in want.tolist()]}, "
          f"rel {e_t:.2e}); grad norm {gn:.4f} (rel {e_gn:.2e}); worst param-grad rel_err {worst[0]:.2e} at {worst[1]}")
    net.zero_grad()
    assert e_t <= 1e-5 and e_gn <= 1e-4 and worst[0] <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 5. removal end to end
@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    ref = NCSNppRef(**SMALL)
    gen = g(7)
    tau = torch.rand(3, 16, 16, generator=gen)
    noise = torch.randn(25, 4, 3, 16, 16, generator=gen)

    def fresh():
        net = NCSNppModel(**SMALL)
        net.load_state_dict(ref.state_dict())
        return net
    return ref, fresh, tau, noise


def test_remove_backdoor_end_to_end(small):
    """Held-out total after 24 steps at most 0.5 x its value before.  (The CPU oracle alone gives 0.225: 0.3247 -> 0.0732.)"""
    ref, fresh, tau, noise = small
    steps, B, lr = 24, 4, 5e-5
    net = fresh()
    start = net.flat_param.clone()
    fourier = net.time_proj.weight.detach().clone()
    held = noise[24].to(DEV)
    flags = [p.requires_grad for p in net.parameters()]
    res = defense_ve.remove_backdoor(net, _sched(), tau, steps=steps, batch=B, lr=lr, max_grad_norm=1.0, w_clean=1.0, w_shift=1.0, noise=noise[:steps])
    assert [p.requires_grad for p in net.parameters()] == flags and not net.time_proj.weight.requires_grad
    assert torch.equal(res.frozen.flat_param, start) and not any(p.requires_grad for p in res.frozen.parameters())     # the teacher: the state at entry
    assert not torch.equal(net.flat_param, start) and torch.equal(net.time_proj.weight, fourier)
    assert len(res.total) == len(res.clean) == len(res.shift) == steps and all(math.isfinite(v) for v in res.total + res.clean + res.shift)
    assert res.clean[0] <= 1e-6 and abs(res.total[0] - (res.clean[0] + res.shift[0])) <= 1e-5 * res.total[0]
    assert res.timestep == 1999 and abs(res.sigma - SIGMA) <= 1e-4 * SIGMA
    before = defense_ve.removal_objective(fresh(), res.frozen, tau, held, SIGMA).tolist()
    after = defense_ve.removal_objective(net, res.frozen, tau, held, SIGMA).tolist()
    net.zero_grad()
    print(f"[removal] VE shift per step {['%.4f' % v for v in res.shift]}")
    print(f"[removal] VE clean per step {['%.5f' % v for v in res.clean]}")
    print(f"[removal] VE held-out total {before[0]:.5f} -> {after[0]:.5f} (ratio {after[0] / before[0]:.3f}); clean {before[1]:.5f} -> {after[1]:.5f}, "
          f"shift {before[2]:.5f} -> {after[2]:.5f}")
    assert after[0] <= 0.5 * before[0]
    # device noise: reproducible per seed; a mix of flags comes back as it was, also after an exception in a noise callable
    runs = []
    for seed in (11, 11, 12):
        n2 = fresh()
        r = defense_ve.remove_backdoor(n2, _sched(), tau, steps=2, batch=4, lr=lr, seed=seed)
        runs.append((r.total, n2.flat_param.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and runs[0][0] != runs[2][0]
    n3 = fresh()
    list(n3.parameters())[3].requires_grad_(False)
    flags = [p.requires_grad for p in n3.parameters()]

    def boom(i):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError, match="boom"):
        defense_ve.remove_backdoor(n3, _sched(), tau, steps=2, batch=4, lr=lr, noise=boom)
    assert [p.requires_grad for p in n3.parameters()] == flags


# ------------------------------------------------------------------------------------------------------------ 6. the detection features
def test_backdoor_features_on_a_small_model(small):
    ref, fresh, tau, noise = small
    net = fresh()
    n, batch, steps, seed = 10, 4, 3, 5
    sched = _sched()
    sched._rng_offset = 17                                                     # a scheduler with some history: put back afterwards
    pipe = P.ScoreSdeVePipeline(net, sched)
    f = defense_ve.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed)
    assert sched.device_rng_seed is None and sched._rng_offset == 17
    assert (f.n, f.batch, f.num_inference_steps, f.seed) == (n, batch, steps, seed) and f.clean.n == f.shifted.n == n
    sigma = f.sigma
    assert abs(sigma - SIGMA) <= 1e-4 * SIGMA
    # by hand: the same inits (chunks of 4, 4, 2 at disjoint Philox offsets) scaled by sigma_T, one pipeline call per chunk
    chw = 3 * 16 * 16
    eps = [ops.randn(torch.empty(m, 3, 16, 16, device=DEV), seed, k * ((batch * chw + 3) // 4)) for k, m in enumerate((4, 4, 2))]
    assert not torch.equal(eps[0], eps[1])
    sch2 = _sched()
    pipe2 = P.ScoreSdeVePipeline(net, sch2)
    sets = []
    for shift in (0.0, 1.0):
        sch2.device_rng_seed, sch2._rng_offset = seed + 1, 0
        outs = []
        for c in eps:
            x = ops.lincomb(torch.empty_like(c), [(c + shift * tau.to(DEV)).contiguous() if shift else c], [sigma])
            outs.append(pipe2(init=x, num_inference_steps=steps, return_tensor=True))
        sets.append(mitigation.image_set_stats(torch.cat(outs).clamp(0.0, 1.0), postprocess=False))
    for got, want in ((f.clean, sets[0]), (f.shifted, sets[1])):
        assert got.uniformity == want.uniformity and got.tv == want.tv and torch.equal(got.mean_image, want.mean_image)
        assert 0.0 <= float(got.mean_image.min()) and float(got.mean_image.max()) <= 1.0
    assert f.uniformity_ratio == mitigation._ratio(f.shifted.uniformity, f.clean.uniformity)
    print(f"[features] VE clean uniformity {f.clean.uniformity:.4f} tv {f.clean.tv:.2f}; shifted uniformity {f.shifted.uniformity:.4f} tv {f.shifted.tv:.2f}; "
          f"ratios {f.uniformity_ratio:.4f} / {f.tv_ratio:.4f}")
    again = defense_ve.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed)
    other = defense_ve.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed + 1)
    assert again.as_dict() == f.as_dict() and torch.equal(again.shifted.mean_image, f.shifted.mean_image)
    assert other.clean.uniformity != f.clean.uniformity or other.clean.tv != f.clean.tv


# ------------------------------------------------------------------------------------------------------------ 7. the tools
def test_tools_in_a_child_process(tmp_path):
    """tools/invert_trigger.py, detect_backdoor.py and remove_backdoor.py on a small NCSN++ checkpoint written by the project's own save_pretrained."""
    net = NCSNppModel(**SMALL)
    net.reset_parameters(seed=1)
    ckpt = str(tmp_path / "ckpt")
    P.ScoreSdeVePipeline(net, _sched()).save_pretrained(ckpt)
    out_i, out_d, out_r = str(tmp_path / "inv"), str(tmp_path / "detect"), str(tmp_path / "repaired")

    def tool(name, *args):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name), "--ckpt", ckpt, *args], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]

    tool("invert_trigger.py", "--steps", "3", "--batch", "4", "--seed", "2", "--out", out_i)
    info = json.load(open(os.path.join(out_i, "trigger_inv.json")))
    tau = torch.load(os.path.join(out_i, "trigger_inv.pt"))
    assert info["steps"] == 3 and info["batch"] == 4 and info["timestep"] == 1999 and abs(info["sigma"] - SIGMA) <= 1e-4 * SIGMA
    assert len(info["losses"]) == 3 and all(math.isfinite(x) for x in info["losses"]) and tuple(tau.shape) == (3, 16, 16)
    want = defense_ve.invert_trigger(net, _sched(), steps=3, batch=4, seed=2)
    assert info["losses"] == want.losses and torch.equal(tau, want.trigger.cpu())
    trig = os.path.join(out_i, "trigger_inv.pt")

    tool("detect_backdoor.py", "--trigger", trig, "--n", "6", "--batch", "4", "--steps", "2", "--seed", "2", "--threshold", "0.5", "--out", out_d)
    info = json.load(open(os.path.join(out_d, "detection.json")))
    mean = torch.load(os.path.join(out_d, "mean_shifted.pt"))
    assert (info["n"], info["batch"], info["num_inference_steps"], info["seed"], info["pipeline"]) == (6, 4, 2, 2, "ScoreSdeVePipeline")
    assert info["verdict"] == (info["uniformity_ratio"] < 0.5) and abs(info["sigma"] - SIGMA) <= 1e-4 * SIGMA
    assert tuple(mean.shape) == (3, 16, 16) and 0.0 <= float(mean.min()) <= float(mean.max()) <= 1.0
    wantf = defense_ve.backdoor_features(P.ScoreSdeVePipeline(net, _sched()), tau, n=6, batch=4, num_inference_steps=2, seed=2)
    assert info["clean"] == wantf.clean.as_dict() and info["shifted"] == wantf.shifted.as_dict()

    tool("remove_backdoor.py", "--trigger", trig, "--steps", "3", "--batch", "4", "--seed", "2", "--out", out_r)
    info = json.load(open(os.path.join(out_r, "removal.json")))
    assert (info["steps"], info["batch"], info["seed"], info["timestep"], info["lr"]) == (3, 4, 2, 1999, 2e-4)
    assert abs(info["sigma"] - SIGMA) <= 1e-4 * SIGMA
    assert all(len(info[k]) == 3 and all(math.isfinite(v) for v in info[k]) for k in ("total", "clean", "shift")) and info["clean"][0] <= 1e-6
    fixed = P.DiffusionPipeline.from_pretrained(out_r)
    assert type(fixed.unet).__name__ == "NCSNppModel" and not torch.equal(fixed.unet.flat_param, net.flat_param)
    assert torch.equal(fixed.unet.time_proj.weight, net.time_proj.weight)
