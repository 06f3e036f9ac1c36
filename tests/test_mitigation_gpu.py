"""Backdoor mitigation (villandiffusion_amd.mitigation): the removal-loss and image-set kernels against float64 torch, removal_objective against
the CPU oracle, remove_backdoor and backdoor_features end to end on a small model, and both tools in a child process."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import mitigation, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_defense_cpu.py::_model


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------------------ 1. the removal-loss kernel
def _loss(pred, ref, wc=1.0, ws=1.0, gscale=1.0):
    dpred = torch.full(pred.shape, float("nan"), device=DEV)
    terms = torch.full((3,), float("nan"), device=DEV)
    partial = torch.empty(2048, device=DEV)
    ops.removal_loss(pred, ref, wc, ws, dpred, terms, partial, gscale=gscale)
    torch.cuda.synchronize()
    return terms, dpred


@pytest.mark.parametrize("B", [1, 4, 64])
@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 64, 64), (5, 7, 9)])
def test_removal_loss_kernel_against_float64(B, shape):
    wc, ws = 0.75, 1.5
    pred = torch.randn((2 * B,) + shape, generator=g(B))
    ref = torch.randn((B,) + shape, generator=g(B + 1))
    p64 = pred.double().requires_grad_(True)
    r64 = ref.double()
    clean = ((p64[:B] - r64) ** 2).mean()
    shift = ((p64[B:] - r64) ** 2).mean()
    total = wc * clean + ws * shift
    total.backward()
    want = torch.stack([total, clean, shift]).detach()
    terms, dpred = _loss(pred.to(DEV), ref.to(DEV), wc, ws)
    e_t = float(((terms.double().cpu() - want).abs() / want.abs()).max())
    e_g = rel(dpred, p64.grad)
    print(f"[parity] removal loss B={B} {shape}: terms {e_t:.2e}, dpred {e_g:.2e}")
    assert e_t <= 1e-6 and e_g <= 1e-6
    again = _loss(pred.to(DEV), ref.to(DEV), wc, ws)
    assert torch.equal(again[0], terms) and torch.equal(again[1], dpred)                       # fixed summation order


@pytest.mark.parametrize("shape", [(3, 32, 32), (5, 7, 9)])
def test_removal_loss_kernel_views_weights_zero_and_scale(shape):
    B = 4
    Cc, H, W = shape
    buf = torch.randn(2 * B, Cc + 5, H, W, generator=g(2)).to(DEV)
    ref = torch.randn((B,) + shape, generator=g(3)).to(DEV)
    # pred as a channel slice of a wider buffer (batch stride > C*H*W; for (5, 7, 9) not even 16-byte aligned)
    a = _loss(buf[:, 2:2 + Cc], ref)
    b = _loss(buf[:, 2:2 + Cc].contiguous(), ref)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0][0]) > 0
    pred = buf[:, 2:2 + Cc].contiguous()
    # ... and from a pointer that is not 16-byte aligned (scalar accesses): the same elements in the same order
    flat = torch.empty(pred.numel() + 1, device=DEV)
    odd = flat[1:].view(pred.shape)
    odd.copy_(pred)
    assert odd.data_ptr() % 16 != 0
    c = _loss(odd, ref)
    assert torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])
    # a zero weight: exact zeros in that half of dpred, and the other half as before
    t0, d0 = _loss(pred, ref, wc=0.0, ws=1.0)
    assert float(d0[:B].abs().max()) == 0.0 and torch.equal(d0[B:], b[1][B:]) and float(t0[0]) == float(t0[2]) and float(t0[1]) == float(b[0][1])
    t1, d1 = _loss(pred, ref, wc=1.0, ws=0.0)
    assert float(d1[B:].abs().max()) == 0.0 and torch.equal(d1[:B], b[1][:B]) and float(t1[0]) == float(t1[1])
    # pred built from ref twice: nothing to learn, no NaN
    tz, dz = _loss(torch.cat([ref, ref]), ref)
    assert float(tz.abs().max()) == 0.0 and float(dz.abs().max()) == 0.0
    # a power-of-two gradient scale (loss scaling) scales dpred exactly and leaves the terms alone
    ts, ds = _loss(pred, ref, gscale=4096.0)
    assert torch.equal(ds, b[1] * 4096.0) and torch.equal(ts, b[0])
    # both weights 1: the total is twice the project's MSE of pred against [ref; ref]
    loss = torch.empty(1, device=DEV)
    ops.mse_fwd_bwd(pred, torch.cat([ref, ref]), torch.empty_like(pred), loss, torch.empty(1024, device=DEV))
    e = abs(float(b[0][0]) - 2.0 * float(loss)) / (2.0 * float(loss))
    print(f"[parity] removal loss total vs 2 * mse_fwd_bwd {shape}: {e:.2e}")
    assert e <= 1e-6


# ------------------------------------------------------------------------------------------------------------ 2. the image-set statistics
def _sets():
    """The six sets of the design check: gaussian N = 7 / 2 / 64, collapsed with spread 1e-3 and 1e-4, eight identical images."""
    gen = g(0)
    base = lambda s: (torch.rand(s, generator=gen, dtype=torch.float64) * 1.6 - 0.8)[None]
    rn = lambda N, s: torch.randn((N,) + s, generator=gen, dtype=torch.float64)
    return [("gauss", rn(7, (3, 32, 32))), ("gauss", rn(2, (5, 7, 9))), ("gauss", rn(64, (3, 32, 32)) * 0.5),
            ("collapsed 1e-3", base((3, 32, 32)) + 1e-3 * rn(64, (3, 32, 32))), ("collapsed 1e-4", base((3, 64, 64)) + 1e-4 * rn(32, (3, 64, 64))),
            ("identical", base((3, 32, 32)).repeat(8, 1, 1, 1))]


def _ref64(y):
    """Direct pairwise distances, mean TV and the mean image of f32 images, in float64."""
    y = y.double()
    N = y.shape[0]
    flat = y.reshape(N, -1)
    pair = torch.stack([((flat[i] - flat[j]) ** 2).sum() for i in range(N) for j in range(i + 1, N)]).mean()
    tv = (y[:, :, 1:] - y[:, :, :-1]).abs().sum((1, 2, 3)) + (y[:, :, :, 1:] - y[:, :, :, :-1]).abs().sum((1, 2, 3))
    return float(pair), float(tv.mean()), y.mean(0)


@pytest.mark.parametrize("idx", range(6))
def test_image_set_stats_against_float64(idx):
    name, x64 = _sets()[idx]
    x = x64.float()
    N = x.shape[0]
    y = ((x * 0.5) + 0.5).clamp(0.0, 1.0)                       # torch f32, op by op
    out = torch.empty_like(x, device=DEV)
    ops.postprocess(x.to(DEV), out, 0.5, 0.5, 0.0, 1.0, False)
    assert torch.equal(out.cpu(), y)                            # the values the statistics are defined on
    pair, tv, mean = _ref64(y)
    got = mitigation.image_set_stats(x.to(DEV))
    e_u = abs(got.uniformity - pair) / pair if pair else abs(got.uniformity)
    e_tv = abs(got.tv - tv) / tv
    e_m = float((got.mean_image.double().cpu() - mean).abs().max())
    print(f"[parity] image-set stats {name} N={N} {tuple(x.shape[1:])}: uniformity {got.uniformity:.6e} (pairwise f64 {pair:.6e}, rel {e_u:.2e}); "
          f"tv {got.tv:.6e} (rel {e_tv:.2e}); mean image abs {e_m:.2e}")
    assert got.n == N and e_tv <= 1e-6 and e_m <= 1e-7
    if name == "identical":
        assert got.uniformity == 0.0
    else:
        assert e_u <= 1e-6
    again = mitigation.image_set_stats(x.to(DEV))
    assert again.uniformity == got.uniformity and again.tv == got.tv and torch.equal(again.mean_image, got.mean_image)
    # a strided view (batch stride > C*H*W) gives the bits of its contiguous copy
    Cc = x.shape[1]
    wide = torch.randn(N, Cc + 3, x.shape[2], x.shape[3], generator=g(9)).to(DEV)
    wide[:, 1:1 + Cc] = x.to(DEV)
    st = mitigation.image_set_stats(wide[:, 1:1 + Cc])
    assert st.uniformity == got.uniformity and st.tv == got.tv and torch.equal(st.mean_image, got.mean_image)
    # ... and so does one whose pointer is not 16-byte aligned (scalar accesses)
    flat = torch.empty(x.numel() + 1, device=DEV)
    odd = flat[1:].view(x.shape)
    odd.copy_(x)
    assert odd.data_ptr() % 16 != 0
    st = mitigation.image_set_stats(odd)
    assert st.uniformity == got.uniformity and st.tv == got.tv and torch.equal(st.mean_image, got.mean_image)


def test_image_set_stats_without_postprocessing_and_refusals():
    x = torch.randn(5, 3, 16, 16, generator=g(4)) * 3
    pair, tv, mean = _ref64(x)
    got = mitigation.image_set_stats(x.to(DEV), postprocess=False)
    assert abs(got.uniformity - pair) <= 1e-6 * pair and abs(got.tv - tv) <= 1e-6 * tv
    assert float((got.mean_image.double().cpu() - mean).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        mitigation.image_set_stats(x[:1].to(DEV))


# ------------------------------------------------------------------------------------------------------------ 3. against the oracle
def _perturb_norms(ref):
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))


@pytest.mark.parametrize("math_mode", ["bf16x3", "f32"])
def test_removal_objective_matches_oracle(math_mode):
    torch.manual_seed(0)
    ref = UNet2DModelRef()
    _perturb_norms(ref)
    ref_frozen = copy.deepcopy(ref)
    _perturb_norms(ref_frozen)                                  # teacher != student: no term is near zero
    ref_frozen.requires_grad_(False)
    net, frozen = UNet2DModel(), UNet2DModel()
    net.load_state_dict(ref.state_dict())
    frozen.load_state_dict(ref_frozen.state_dict())
    net.conv_math = frozen.conv_math = math_mode
    B, wc, ws = 4, 1.0, 1.0
    eps = torch.randn(B, 3, 32, 32, generator=g(5))
    tau = torch.rand(3, 32, 32, generator=g(6))
    t = torch.full((2 * B,), 999)
    with torch.no_grad():
        y = ref_frozen(eps, t[:B])[0]
    e = ref(torch.cat([eps, eps + tau]), t)[0]
    clean, shift = ((e[:B] - y) ** 2).mean(), ((e[B:] - y) ** 2).mean()
    (clean + shift).backward()
    want = torch.stack([clean + shift, clean, shift]).detach().double()
    frozen_before = frozen.flat_param.clone()
    flags = [p.requires_grad for p in net.parameters()]
    net.zero_grad()
    terms = mitigation.removal_objective(net, frozen, tau.to(DEV), eps.to(DEV), 999, wc, ws)
    assert [p.requires_grad for p in net.parameters()] == flags and all(flags)
    assert torch.equal(frozen.flat_param, frozen_before)
    e_t = float(((terms.double().cpu() - want).abs() / want.abs()).max())
    gref = {n: p.grad for n, p in ref.named_parameters()}
    gmax = max(float(v.abs().max()) for v in gref.values())
    worst = (0.0, "")
    for n, p in net.named_parameters():
        a, b = p.grad.detach().double().cpu(), gref[n].double()
        err = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))          # relative to the parameter's own gradient scale (test_unet_gpu.py)
        if err > worst[0]:
            worst = (err, n)
    gn_ref = float(torch.sqrt(sum((v.double() ** 2).sum() for v in gref.values())))
    gn = float(torch.sqrt((net.flat_grad.double() ** 2).sum()))
    e_gn = abs(gn - gn_ref) / gn_ref
    print(f"[parity] removal_objective ({math_mode}): terms {[('%.5f' % v) for v in terms.tolist()]} (oracle {[('%.5f' % v) for v in want.tolist()]}, "
          f"rel {e_t:.2e}); grad norm {gn:.4f} (rel {e_gn:.2e}); worst param-grad rel_err {worst[0]:.2e} at {worst[1]}")
    net.zero_grad()
    assert e_t <= 1e-5 and e_gn <= 1e-4 and worst[0] <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**SMALL)
    gen = g(7)
    tau = torch.rand(3, 32, 32, generator=gen)
    noise = torch.randn(25, 4, 3, 32, 32, generator=gen)

    def fresh():
        net = UNet2DModel(**SMALL)
        net.load_state_dict(ref.state_dict())
        return net
    return ref, fresh, tau, noise


def _oracle_removal(ref, tau, noise, steps, lr):
    net = copy.deepcopy(ref)
    frozen = copy.deepcopy(ref).requires_grad_(False)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    B = noise.shape[1]
    t = torch.full((2 * B,), 999)
    rows = []
    for it in range(steps):
        with torch.no_grad():
            y = frozen(noise[it], t[:B])[0]
        e = net(torch.cat([noise[it], noise[it] + tau]), t)[0]
        c, s = ((e[:B] - y) ** 2).mean(), ((e[B:] - y) ** 2).mean()
        opt.zero_grad()
        (c + s).backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        rows.append((float(c.detach() + s.detach()), float(c.detach()), float(s.detach())))
    return net, rows


def test_remove_backdoor_end_to_end(small):
    """Held-out total after 24 steps at most 0.8 x its value before.  (The CPU oracle alone gives 0.51 for these weights.)"""
    ref, fresh, tau, noise = small
    steps, B, lr = 24, 4, 5e-5
    net = fresh()
    start = net.flat_param.clone()
    held = noise[24].to(DEV)
    flags = [p.requires_grad for p in net.parameters()]
    res = mitigation.remove_backdoor(net, S.DDPMScheduler(), tau, steps=steps, batch=B, lr=lr, max_grad_norm=1.0, w_clean=1.0, w_shift=1.0,
                                     noise=noise[:steps])
    assert [p.requires_grad for p in net.parameters()] == flags and all(flags)
    assert torch.equal(res.frozen.flat_param, start) and not any(p.requires_grad for p in res.frozen.parameters())     # the teacher: the state at entry
    assert not torch.equal(net.flat_param, start)
    assert len(res.total) == len(res.clean) == len(res.shift) == steps and all(math.isfinite(v) for v in res.total + res.clean + res.shift)
    # step 0: student == teacher, so `clean` is the squared difference between the training forward at 2B and the captured no-grad forward at B
    assert res.clean[0] <= 1e-6 and abs(res.total[0] - (res.clean[0] + res.shift[0])) <= 1e-6 * res.total[0] and res.timestep == 999
    before = mitigation.removal_objective(fresh(), res.frozen, tau, held, 999).tolist()
    after = mitigation.removal_objective(net, res.frozen, tau, held, 999).tolist()
    net.zero_grad()
    o_net, o_rows = _oracle_removal(ref, tau, noise, steps, lr)
    o_par, r_par = dict(o_net.named_parameters()), dict(ref.named_parameters())
    dist = math.sqrt(sum(float(((p.detach().cpu().double() - o_par[k].detach().double()) ** 2).sum()) for k, p in net.named_parameters()))
    moved = math.sqrt(sum(float(((o_par[k].detach().double() - r_par[k].detach().double()) ** 2).sum()) for k in o_par))
    print(f"[removal] shift per step {['%.4f' % v for v in res.shift]}")
    print(f"[removal] clean per step {['%.5f' % v for v in res.clean]}")
    print(f"[removal] oracle shift   {['%.4f' % r[2] for r in o_rows]}")
    print(f"[removal] held-out total {before[0]:.5f} -> {after[0]:.5f} (ratio {after[0] / before[0]:.3f}); clean {before[1]:.5f} -> {after[1]:.5f}, "
          f"shift {before[2]:.5f} -> {after[2]:.5f}")
    print(f"[removal] parameter distance to the oracle's {steps}-step result {dist:.3e} (the oracle moved {moved:.3e} from the start): recorded, not gated")
    assert after[0] <= 0.8 * before[0]


def test_remove_backdoor_is_reproducible_and_restores_flags(small):
    ref, fresh, tau, noise = small
    sched = S.DDPMScheduler()
    runs = []
    for seed in (11, 11, 12):
        net = fresh()
        res = mitigation.remove_backdoor(net, sched, tau, steps=3, batch=4, lr=5e-5, seed=seed)
        runs.append((res, net.flat_param.clone()))
    (a, wa), (b, wb), (c, wc) = runs
    assert (a.total, a.clean, a.shift) == (b.total, b.clean, b.shift) and torch.equal(wa, wb)     # device Philox noise, fixed summation orders
    assert a.shift != c.shift and not torch.equal(wa, wc)
    # a tensor and a callable give the same run
    n1, n2 = fresh(), fresh()
    r1 = mitigation.remove_backdoor(n1, sched, tau, steps=3, batch=4, lr=5e-5, noise=noise[:3])
    r2 = mitigation.remove_backdoor(n2, sched, tau, steps=3, batch=4, lr=5e-5, noise=lambda i: noise[i])
    assert r1.total == r2.total and torch.equal(n1.flat_param, n2.flat_param)
    # a mix of frozen and trainable parameters comes back as it was, also after an exception in a noise callable
    net = fresh()
    next(net.parameters()).requires_grad_(False)
    flags = [p.requires_grad for p in net.parameters()]
    mitigation.remove_backdoor(net, sched, tau, steps=1, batch=4, lr=5e-5)
    assert [p.requires_grad for p in net.parameters()] == flags and not flags[0]
    with pytest.raises(ValueError):
        mitigation.remove_backdoor(net, sched, tau, steps=2, batch=4, lr=5e-5, noise=lambda i: noise[i][:1])
    assert [p.requires_grad for p in net.parameters()] == flags

    def boom(i):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError, match="boom"):
        mitigation.remove_backdoor(net, sched, tau, steps=2, batch=4, lr=5e-5, noise=boom)
    assert [p.requires_grad for p in net.parameters()] == flags


def test_remove_backdoor_refuses_what_it_is_not_built_for(small):
    from villandiffusion_amd.ncsnpp import NCSNppModel
    ref, fresh, tau, noise = small
    pp = dict(sample_size=16, block_out_channels=(32, 64, 64), down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
              up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        mitigation.remove_backdoor(NCSNppModel(**pp), S.DDPMScheduler(), torch.zeros(3, 16, 16), steps=1, batch=1, lr=1e-4)
    net = fresh()
    with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
        mitigation.remove_backdoor(net, S.ScoreSdeVeScheduler(), tau, steps=1, batch=1, lr=1e-4)
    start = net.flat_param.clone()
    net.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16"):
        mitigation.remove_backdoor(net, S.DDPMScheduler(), tau, steps=1, batch=1, lr=1e-4)
    assert torch.equal(net.flat_param, start)


def test_remove_backdoor_bf16_mode_runs(small):
    ref, fresh, tau, noise = small
    net = fresh()
    net.conv_math = "bf16"
    res = mitigation.remove_backdoor(net, S.DDPMScheduler(), tau, steps=2, batch=4, lr=5e-5, noise=noise[:2])
    assert res.frozen.conv_math == "bf16" and all(math.isfinite(v) for v in res.total) and res.shift[0] > 0


# ------------------------------------------------------------------------------------------------------------ 5. the detection features
def test_backdoor_features_on_a_small_model(small):
    ref, fresh, tau, noise = small
    net = fresh()
    n, batch, steps, seed = 20, 8, 4, 5
    pipe = P.DDIMPipeline(net, S.DDIMScheduler())
    f = mitigation.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed)
    assert (f.n, f.batch, f.num_inference_steps, f.seed) == (n, batch, steps, seed) and f.clean.n == f.shifted.n == n
    # by hand: the same inits (chunks of 8, 8, 4 at disjoint Philox offsets), one pipeline call per chunk
    chw = 3 * 32 * 32
    inits = []
    for k, m in enumerate((8, 8, 4)):
        inits.append(ops.randn(torch.empty(m, 3, 32, 32, device=DEV), seed, k * ((batch * chw + 3) // 4)))
    assert not torch.equal(inits[0], inits[1]) and not torch.equal(inits[0][:4], inits[2])
    pipe2 = P.DDIMPipeline(net, S.DDIMScheduler())
    clean = torch.cat([pipe2(init=c, num_inference_steps=steps, return_tensor=True) for c in inits])
    shifted = torch.cat([pipe2(init=c + tau.to(DEV), num_inference_steps=steps, return_tensor=True) for c in inits])       # the SAME eps: paired sets
    for got, x in ((f.clean, clean), (f.shifted, shifted)):
        want = mitigation.image_set_stats(x)
        assert got.uniformity == want.uniformity and got.tv == want.tv and torch.equal(got.mean_image, want.mean_image)
    assert f.uniformity_ratio == f.shifted.uniformity / f.clean.uniformity and f.tv_ratio == f.shifted.tv / f.clean.tv
    print(f"[features] clean uniformity {f.clean.uniformity:.4f} tv {f.clean.tv:.2f}; shifted uniformity {f.shifted.uniformity:.4f} tv {f.shifted.tv:.2f}; "
          f"ratios {f.uniformity_ratio:.4f} / {f.tv_ratio:.4f}")
    again = mitigation.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed)
    other = mitigation.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed + 1)
    assert again.as_dict() == f.as_dict() and other.clean.uniformity != f.clean.uniformity
    with pytest.raises(TypeError):
        f.verdict()
    assert f.verdict(float("inf")) is True and f.verdict(0.0) is False
    # a stochastic sampler: the scheduler gets a device seed of its own for the call (seed + 1) and is left as it was found
    dd = P.DDPMPipeline(net, S.DDPMScheduler())
    a = mitigation.backdoor_features(dd, tau, n=6, batch=4, num_inference_steps=3, seed=2)
    b = mitigation.backdoor_features(dd, tau, n=6, batch=4, num_inference_steps=3, seed=2)
    assert a.as_dict() == b.as_dict() and dd.scheduler.device_rng_seed is None and getattr(dd.scheduler, "_rng_offset", 0) == 0


def test_backdoor_features_refuses_latent_and_ve_pipelines(small):
    from villandiffusion_amd.ncsnpp import NCSNppModel
    ref, fresh, tau, noise = small
    with pytest.raises(NotImplementedError, match="LDMPipeline"):
        mitigation.backdoor_features(P.LDMPipeline(vqvae=object(), unet=fresh(), scheduler=S.DDIMScheduler()), tau, n=4, batch=2)
    pp = NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                     up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)
    with pytest.raises(NotImplementedError, match="ScoreSdeVePipeline"):
        mitigation.backdoor_features(P.ScoreSdeVePipeline(pp, S.ScoreSdeVeScheduler()), torch.zeros(3, 16, 16), n=4, batch=2)


# ------------------------------------------------------------------------------------------------------------ 6. the tools
def test_tools_detect_and_remove_in_a_child_process(tmp_path):
    """tools/detect_backdoor.py and tools/remove_backdoor.py on a (small) diffusers-format checkpoint written by the project's own save_pretrained."""
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=1)
    ckpt, out_d, out_r = str(tmp_path / "ckpt"), str(tmp_path / "detect"), str(tmp_path / "repaired")
    P.DDIMPipeline(net, S.DDIMScheduler()).save_pretrained(ckpt)
    trig = str(tmp_path / "trigger_inv.pt")
    tau = torch.rand(3, 32, 32, generator=g(8))
    torch.save(tau, trig)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "detect_backdoor.py"), "--ckpt", ckpt, "--trigger", trig, "--n", "10", "--batch", "4",
                          "--steps", "3", "--seed", "2", "--threshold", "0.5", "--out", out_d], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    info = json.load(open(os.path.join(out_d, "detection.json")))
    mean = torch.load(os.path.join(out_d, "mean_shifted.pt"))
    assert (info["n"], info["batch"], info["num_inference_steps"], info["seed"], info["threshold"]) == (10, 4, 3, 2, 0.5)
    assert info["verdict"] == (info["uniformity_ratio"] < 0.5) and tuple(mean.shape) == (3, 32, 32) and 0.0 <= float(mean.min()) <= float(mean.max()) <= 1.0
    want = mitigation.backdoor_features(P.DiffusionPipeline.from_pretrained(ckpt), tau, n=10, batch=4, num_inference_steps=3, seed=2)
    assert info["clean"] == want.clean.as_dict() and info["shifted"] == want.shifted.as_dict() and info["uniformity_ratio"] == want.uniformity_ratio
    assert torch.equal(mean, want.shifted.mean_image.cpu())
    # no --threshold: no verdict
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "detect_backdoor.py"), "--ckpt", ckpt, "--trigger", trig, "--n", "4", "--batch", "4",
                          "--steps", "2", "--out", out_d], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "verdict" not in json.load(open(os.path.join(out_d, "detection.json")))

    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "remove_backdoor.py"), "--ckpt", ckpt, "--trigger", trig, "--steps", "3", "--batch", "4",
                          "--seed", "2", "--out", out_r], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    info = json.load(open(os.path.join(out_r, "removal.json")))
    assert (info["steps"], info["batch"], info["seed"], info["timestep"], info["lr"]) == (3, 4, 2, 999, 2e-4)
    assert all(len(info[k]) == 3 and all(math.isfinite(v) for v in info[k]) for k in ("total", "clean", "shift")) and info["clean"][0] <= 1e-6
    fixed = P.DiffusionPipeline.from_pretrained(out_r)
    assert not torch.equal(fixed.unet.flat_param, net.flat_param)
    twin = UNet2DModel(**SMALL)
    twin.flat_param.data.copy_(net.flat_param)
    twin.weights_changed()
    res = mitigation.remove_backdoor(twin, S.DDIMScheduler(), tau, steps=3, batch=4, lr=2e-4, seed=2)
    assert info["shift"] == res.shift and torch.equal(fixed.unet.flat_param, twin.flat_param)      # the JSON and the checkpoint match the tensors
