"""villandiffusion_amd.defense_ldm on the GPU: the streaming image-set statistics (`vd_image_set_merge`) against float64 torch, the pixel-space
objective and one iteration against the oracle pair (oracle/unet_ref.py after oracle/vqmodel_ref.py), inversion in both spaces, the detection
features, removal, and the three tools on a saved LDM checkpoint in child processes."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from oracle.vqmodel_ref import VQModelRef  # noqa: E402
from villandiffusion_amd import defense, defense_ldm, mitigation, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402
from villandiffusion_amd.vqmodel import VQModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNET = dict(sample_size=8, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # the defence tests' small model, at 3x8x8
VQ = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3)
VQ_NET = dict(VQ, down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2, sample_size=16)
Z, PX = (3, 8, 8), (3, 16, 16)


def g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ 1. the merge kernel
SHAPES = [(3, 32, 32), (5, 7, 9), (3, 64, 64)]
CHUNKINGS = [(5, 2), (64, 16), (7, 7)]                     # (N, chunk): a lone last image; three merges; one chunk
KINDS = ["random", "collapsed 1e-3", "saturating"]


def _set(kind, N, shape):
    gen = g(N + shape[1])
    rn = torch.randn((N,) + shape, generator=gen, dtype=torch.float64)
    if kind == "random":
        return rn * 0.5
    if kind == "collapsed 1e-3":
        return (torch.rand(shape, generator=gen, dtype=torch.float64) * 1.6 - 0.8)[None] + 1e-3 * rn
    return rn * 3.0                                        # most values beyond the clamp of the post-processing


def _ref64(y):
    """tests/test_mitigation_gpu.py's reference: direct pairwise distances, mean TV and the mean image of f32 images, in float64."""
    y = y.double()
    N = y.shape[0]
    flat = y.reshape(N, -1)
    pair = torch.stack([((flat[i] - flat[j]) ** 2).sum() for i in range(N) for j in range(i + 1, N)]).mean()
    tv = (y[:, :, 1:] - y[:, :, :-1]).abs().sum((1, 2, 3)) + (y[:, :, :, 1:] - y[:, :, :, :-1]).abs().sum((1, 2, 3))
    return float(pair), float(tv.mean()), y.mean(0)


def _errors(got, pair, tv, mean):
    return (abs(got.uniformity - pair) / pair, abs(got.tv - tv) / tv, float((got.mean_image.double().cpu() - mean).abs().max()))


def _streamed(x, chunk, **kw):
    acc = defense_ldm.ImageSetAccumulator(x.shape[1:], x.device, **kw)
    for i in range(0, x.shape[0], chunk):
        acc.add(x[i:i + chunk])
    return acc.result()


def _same(a, b):
    return a.n == b.n and a.uniformity == b.uniformity and a.tv == b.tv and torch.equal(a.mean_image, b.mean_image)


@pytest.mark.parametrize("N,chunk", CHUNKINGS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_streamed_image_set_stats_against_float64(kind, shape, N, chunk):
    """The bound of tests/test_mitigation_gpu.py::test_image_set_stats_against_float64 for the resident kernel: uniformity and TV 1e-6 relative,
    the mean image 1e-7 absolute.  The resident kernel's own error on the same set is printed next to the streamed one."""
    x = _set(kind, N, shape).float()
    y = ((x * 0.5) + 0.5).clamp(0.0, 1.0)
    pair, tv, mean = _ref64(y)
    xd = x.to(DEV)
    resident = mitigation.image_set_stats(xd)
    got = _streamed(xd, chunk)
    r_u, r_tv, r_m = _errors(resident, pair, tv, mean)
    e_u, e_tv, e_m = _errors(got, pair, tv, mean)
    print(f"[parity] streamed image-set stats {kind} N={N} in chunks of {chunk} {shape}: uniformity rel {e_u:.2e} (resident {r_u:.2e}); "
          f"tv rel {e_tv:.2e} (resident {r_tv:.2e}); mean image abs {e_m:.2e} (resident {r_m:.2e})")
    assert got.n == N and e_tv <= 1e-6 and e_m <= 1e-7 and e_u <= 1e-6
    if chunk >= N:
        assert _same(got, resident)                         # one chunk through the accumulator: the resident call, bit for bit
    assert _same(_streamed(xd, chunk), got)                 # two runs are bit-identical
    # a strided chunk view (batch stride > C*H*W) gives the bits of its contiguous copy
    Cc = shape[0]
    wide = torch.randn(N, Cc + 3, shape[1], shape[2], generator=g(9)).to(DEV)
    wide[:, 1:1 + Cc] = xd
    assert _same(_streamed(wide[:, 1:1 + Cc], chunk), got)
    # without post-processing: the set as it is
    pair, tv, mean = _ref64(x)
    raw = _streamed(xd, chunk, postprocess=False)
    e_u, e_tv, e_m = _errors(raw, pair, tv, mean)
    scale = float(mean.abs().max())                         # (the 1e-7 of the [0, 1] images, for a mean image of this size)
    assert e_u <= 1e-6 and e_tv <= 1e-6 and e_m <= 1e-7 * max(1.0, 2.0 * scale)


def test_merge_kernel_contract():
    """n_a == 0 copies b into a; unaligned means (scalar accesses) give the bits of aligned ones; the update is Chan et al.'s."""
    shape = (5, 7, 9)
    n = 5 * 7 * 9
    gen = g(3)
    ma, mb = torch.rand(n, generator=gen), torch.rand(n, generator=gen)
    sa, sb = torch.tensor([3.0, 7.0]), torch.tensor([2.0, 5.0])
    partial = torch.empty(2048, device=DEV)
    a, s = torch.full((n,), float("nan"), device=DEV), torch.full((2,), float("nan"), device=DEV)
    ops.image_set_merge(a, s, 0, mb.to(DEV), sb.to(DEV), 4, partial)
    assert torch.equal(a.cpu(), mb) and torch.equal(s.cpu(), sb)
    a, s = ma.to(DEV), sa.to(DEV)
    ops.image_set_merge(a, s, 6, mb.to(DEV), sb.to(DEV), 2, partial)
    d = mb.double() - ma.double()
    want_mean = (ma.double() + d * (2 / 8)).float()
    want0 = float(torch.tensor(3.0 + 2.0 + 6 * 2 / 8 * float((d * d).sum())).float())
    assert torch.equal(a.cpu(), want_mean) and abs(float(s[0]) - want0) <= 2e-7 * want0 and float(s[1]) == 12.0
    # 4-divisible size: aligned (16-byte accesses) against a misaligned copy (scalar accesses)
    m4a, m4b = torch.rand(3 * 32 * 32, generator=gen).to(DEV), torch.rand(3 * 32 * 32, generator=gen).to(DEV)
    a1, s1 = m4a.clone(), sa.to(DEV)
    ops.image_set_merge(a1, s1, 6, m4b, sb.to(DEV), 2, partial)
    flat = torch.empty(m4a.numel() + 1, device=DEV)
    a2 = flat[1:]
    a2.copy_(m4a)
    s2 = sa.to(DEV)
    assert a2.data_ptr() % 16 != 0
    ops.image_set_merge(a2, s2, 6, m4b, sb.to(DEV), 2, partial)
    assert torch.equal(a1, a2) and torch.equal(s1, s2)
    with pytest.raises(ValueError):
        defense_ldm.ImageSetAccumulator(shape, DEV).add(torch.zeros(1, *shape, device=DEV)).result()       # one image is no set
    with pytest.raises(ValueError):
        defense_ldm.ImageSetAccumulator(shape, DEV).add(torch.zeros(2, 3, 7, 9, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 2. the tiny pipeline and its oracle
@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    uref, vref = UNet2DModelRef(**UNET), VQModelRef(**VQ)
    with torch.no_grad():
        for ref in (uref, vref):
            for n, p in ref.named_parameters():
                if "norm" in n:
                    p.add_(0.1 * torch.randn_like(p))
        vref.quantize.embedding.weight.normal_(0, 0.5)

    def fresh(sched=None):
        unet, vq = UNet2DModel(**UNET), VQModel(**VQ_NET)
        unet.load_state_dict(uref.state_dict())
        vq.load_state_dict(vref.state_dict())
        return P.LDMPipeline(vqvae=vq, unet=unet, scheduler=sched if sched is not None else S.DDIMScheduler())
    return uref, vref, fresh, fresh()


def _oracle_objective(uref, vref, p, eps, t, lam):
    pr = p.clone().requires_grad_(True)
    z = vref.encode(pr[None]).latents[0]
    e = uref(eps + z, t)[0]
    L = (e.mean(0) - lam * z).norm()
    L.backward()
    uref.zero_grad()
    vref.zero_grad()
    return L.item(), pr.grad, z.detach()


def test_pixel_objective_matches_the_oracle_pair(tiny):
    """The bounds of tests/test_trigger_inversion_gpu.py::test_inversion_objective_matches_oracle: loss 1e-5, gradient 1e-3 of its maximum."""
    uref, vref, _, pipe = tiny
    B, lam = 4, 0.5
    eps = torch.randn((B,) + Z, generator=g(5))
    p = torch.rand(PX, generator=g(6)) * 2 - 1
    t = torch.full((B,), 999)
    L_ref, dp_ref, _ = _oracle_objective(uref, vref, p, eps, t, lam)
    flags = [q.requires_grad for q in pipe.unet.parameters()]
    loss, dp = defense_ldm.inversion_objective(pipe, p.to(DEV), eps.to(DEV), t.to(DEV), lam)
    assert [q.requires_grad for q in pipe.unet.parameters()] == flags and all(flags) and pipe.vqvae._input_grad is False
    assert all(q.grad is None for q in pipe.vqvae.parameters())
    e_loss = abs(float(loss) - L_ref) / L_ref
    e_g = float((dp.double().cpu() - dp_ref.double()).abs().max() / dp_ref.double().abs().max())
    print(f"[parity] pixel inversion_objective: L={float(loss):.4f} (oracle {L_ref:.4f}, rel {e_loss:.2e}); dp rel_err {e_g:.2e} "
          f"(max|dp_ref| {float(dp_ref.abs().max()):.3e})")
    assert tuple(dp.shape) == PX and e_loss <= 1e-5 and e_g <= 1e-3


def test_one_pixel_iteration_matches_torch_adam_then_clamp(tiny):
    uref, vref, _, pipe = tiny
    B, lam, lr = 4, 0.5, 0.1
    eps = torch.randn((B,) + Z, generator=g(5))
    p0 = torch.rand(PX, generator=g(6)) * 2.2 - 1.1                 # some pixels leave [-1, 1] with the step, some start outside
    _, dp_ref, _ = _oracle_objective(uref, vref, p0, eps, torch.full((B,), 999), lam)       # the oracle's gradient: sign flips are not the subject
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr)
    pt.grad = dp_ref.clone()
    opt.step()
    want = pt.detach().clamp(-1.0, 1.0)
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    defense.adam_update(p, dp_ref.to(DEV), m, v, 1, lr)
    q = defense_ldm._clamp_into(p, torch.empty_like(p), -1.0, 1.0)
    err = float((q.cpu() - want).abs().max())
    print(f"[parity] Adam step + clamp on the pixel trigger vs torch: max abs err {err:.2e}")
    assert err <= 1e-6 and float(q.max()) == 1.0 and float(q.min()) == -1.0 and float((pt.detach().abs() > 1.0).float().mean()) > 0.01


# ------------------------------------------------------------------------------------------------------------ 3. inversion
def test_latent_space_is_defense_invert_trigger(tiny):
    _, _, _, pipe = tiny
    noise = torch.randn(3, 4, *Z, generator=g(7))
    a = defense_ldm.invert_trigger(pipe, space="latent", steps=3, batch=4, seed=3, noise=noise, lr=0.05, lam=0.4, timestep=500)
    b = defense.invert_trigger(pipe.unet, pipe.scheduler, steps=3, batch=4, seed=3, noise=noise, lr=0.05, lam=0.4, timestep=500)
    assert torch.equal(a.trigger, b.trigger) and a.losses == b.losses and a.extra == {"space": "latent"} and b.extra == {}
    assert (a.lam, a.lr, a.steps, a.batch, a.timestep, a.seed) == (b.lam, b.lr, b.steps, b.batch, b.timestep, b.seed)
    c = defense_ldm.invert_trigger(pipe, steps=2, batch=4, seed=11)                        # the default space, device noise
    d = defense.invert_trigger(pipe.unet, pipe.scheduler, steps=2, batch=4, seed=11)
    assert torch.equal(c.trigger, d.trigger) and c.losses == d.losses and tuple(c.trigger.shape) == Z


def test_pixel_space_inversion_against_the_oracle_loop(tiny):
    """Three iterations with the caller's noise against torch.optim.Adam + clamp on the oracle pair.  No existing end-to-end test carries an
    oracle-loop bound, so this one is derived from the project's own gradient bound.  An Adam step is lr * m / (sqrt(v) + eps): in the first
    steps close to lr * sign(g), so a pixel whose gradient lies inside the gradient error (1e-3 of the largest, the test above) may move the other
    way, and any pixel's step may be off by lr times its gradient's relative error: p is not comparable pixel by pixel.  The objective is.
    Iteration 0 sees the same p on both sides: the objective's own bound, 1e-5.  Before iteration k every pixel is off by at most 2 lr k and
    dL = sum_i g_i dp_i with the error-carrying part of each g_i dp_i at most 1e-3 max|g| * 2 lr, so |dL| <= k * n * 1e-3 * max|g| * 2 lr: the gate
    of iteration k, from the oracle's max|g| and L alone (a worst case over all n pixels; what is measured is printed)."""
    uref, vref, _, pipe = tiny
    steps, batch, lam, lr = 3, 4, 0.5, 0.1
    noise = torch.randn(steps, batch, *Z, generator=g(8))
    init = torch.rand(PX, generator=g(9)) * 2.2 - 1.1
    pt = init.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr)
    o_losses, gmax = [], 0.0
    for it in range(steps):
        L, grad, _ = _oracle_objective(uref, vref, pt.detach(), noise[it], torch.full((batch,), 999), lam)
        o_losses.append(L)
        gmax = max(gmax, float(grad.abs().max()))
        pt.grad = grad
        opt.step()
        with torch.no_grad():
            pt.clamp_(-1.0, 1.0)
    flags = [q.requires_grad for q in pipe.unet.parameters()]
    res = defense_ldm.invert_trigger(pipe, space="pixel", steps=steps, batch=batch, lam=lam, lr=lr, init=init, noise=noise)
    assert [q.requires_grad for q in pipe.unet.parameters()] == flags and all(flags) and pipe.vqvae._input_grad is False
    assert not any(q.requires_grad for q in pipe.vqvae.parameters()) and all(q.grad is None for q in pipe.vqvae.parameters())
    errs = [abs(a - b) / b for a, b in zip(res.losses, o_losses)]
    moved = float((res.trigger.cpu() - pt.detach()).abs().mean())
    print(f"[inversion] pixel losses {['%.5f' % x for x in res.losses]} oracle {['%.5f' % x for x in o_losses]} rel {['%.1e' % e for e in errs]}; "
          f"max|g| {gmax:.3e}; mean |p - p_oracle| {moved:.2e}")
    n_px = PX[0] * PX[1] * PX[2]
    gates = [1e-5 + k * n_px * 1e-3 * gmax * 2 * lr / o_losses[k] for k in range(steps)]
    print(f"[inversion] gates {['%.1e' % x for x in gates]}")
    assert all(e <= gt for e, gt in zip(errs, gates)), (errs, gates)
    assert tuple(res.trigger.shape) == PX and float(res.trigger.min()) >= -1.0 and float(res.trigger.max()) <= 1.0
    assert float((init.abs() > 1.0).float().mean()) > 0.01                                  # (the clamp had something to do)
    assert res.extra["space"] == "pixel" and torch.equal(res.extra["latent"], defense_ldm.encode_trigger(pipe, res.trigger))
    assert torch.equal(res.extra["latent"], pipe.encode(res.trigger[None])[0]) and res.timestep == 999
    # reproducible; no clamp when asked; the default init is the VP rule at pixel shape
    again = defense_ldm.invert_trigger(pipe, space="pixel", steps=steps, batch=batch, lam=lam, lr=lr, init=init, noise=lambda i: noise[i])
    assert torch.equal(again.trigger, res.trigger) and again.losses == res.losses
    free = defense_ldm.invert_trigger(pipe, space="pixel", steps=1, batch=batch, init=init, noise=noise[:1], clamp=None)
    assert float(free.trigger.abs().max()) > 1.0
    dflt = defense_ldm.invert_trigger(pipe, space="pixel", steps=1, batch=batch, seed=5, lr=1e-9, noise=noise[:1])
    assert torch.allclose(dflt.trigger.cpu(), torch.rand(PX, generator=g(5)), atol=1e-6)
    # the flags and the switch come back after an exception inside the loop too
    with pytest.raises(ValueError):
        defense_ldm.invert_trigger(pipe, space="pixel", steps=2, batch=batch, noise=lambda i: noise[i][:1])
    assert [q.requires_grad for q in pipe.unet.parameters()] == flags and pipe.vqvae._input_grad is False


def test_render_and_encode_trigger(tiny):
    _, vref, _, pipe = tiny
    z = torch.randn(Z, generator=g(10))
    img = defense_ldm.render_trigger(pipe, z)
    assert tuple(img.shape) == PX and torch.equal(img, pipe.vqvae.decode(z[None].to(DEV)).sample[0])
    p = torch.rand(PX, generator=g(11)) * 2 - 1
    lat = defense_ldm.encode_trigger(pipe, p)
    with torch.no_grad():
        want = vref.encode(p[None]).latents[0]
    assert tuple(lat.shape) == Z and float((lat.cpu() - want).abs().max() / want.abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------ 4. the detection features
def test_backdoor_features_on_the_tiny_pipeline(tiny):
    _, _, fresh, pipe = tiny
    n, batch, steps, seed = 5, 2, 4, 5
    tau = torch.rand(Z, generator=g(12))
    f = defense_ldm.backdoor_features(pipe, tau, n=n, batch=batch, num_inference_steps=steps, seed=seed)
    assert isinstance(f, defense_ldm.LDMBackdoorFeatures) and (f.n, f.batch, f.num_inference_steps, f.seed, f.space) == (n, batch, steps, seed, "latent")
    # by hand: the same inits (chunks of 2, 2, 1 at disjoint Philox offsets), one pipeline call per chunk, everything resident
    chw = Z[0] * Z[1] * Z[2]
    inits = [ops.randn(torch.empty((m,) + Z, device=DEV), seed, k * ((batch * chw + 3) // 4)) for k, m in enumerate((2, 2, 1))]
    pipe2 = fresh()
    for got_px, got_lat, shift in ((f.clean, f.latent_clean, 0.0), (f.shifted, f.latent_shifted, 1.0)):
        starts = [c + shift * tau.to(DEV) for c in inits]
        imgs = torch.cat([pipe2(init=c, num_inference_steps=steps, return_tensor=True) for c in starts])
        lats = torch.cat([P.DiffusionPipeline.__call__(pipe2, init=c, num_inference_steps=steps, return_tensor=True) for c in starts])
        assert tuple(imgs.shape) == (n,) + PX and tuple(lats.shape) == (n,) + Z
        for got, y in ((got_px, ((imgs.cpu() * 0.5) + 0.5).clamp(0.0, 1.0)), (got_lat, lats.cpu())):        # the merge bound, against float64
            pair, tv, mean = _ref64(y)
            e_u, e_tv, e_m = _errors(got, pair, tv, mean)
            assert got.n == n and e_u <= 1e-6 and e_tv <= 1e-6 and e_m <= 1e-7 * max(1.0, 2.0 * float(mean.abs().max())), (e_u, e_tv, e_m)
    assert f.uniformity_ratio == f.shifted.uniformity / f.clean.uniformity and f.tv_ratio == f.shifted.tv / f.clean.tv
    assert f.latent_uniformity_ratio == f.latent_shifted.uniformity / f.latent_clean.uniformity
    print(f"[features] LDM pixel ratios {f.uniformity_ratio:.4f} / {f.tv_ratio:.4f}; latent uniformity ratio {f.latent_uniformity_ratio:.4f}")
    d = f.as_dict()
    assert d["space"] == "latent" and d["latent"]["clean"] == f.latent_clean.as_dict() and json.dumps(d)
    # a zero trigger: both sets are the same set
    zero = defense_ldm.backdoor_features(pipe, torch.zeros(Z), n=n, batch=batch, num_inference_steps=steps, seed=seed)
    assert zero.uniformity_ratio == 1.0 and zero.tv_ratio == 1.0 and zero.latent_uniformity_ratio == 1.0
    # a pixel trigger and its encode_trigger give identical records (but for the space they name)
    p = torch.rand(PX, generator=g(13)) * 2 - 1
    a = defense_ldm.backdoor_features(pipe, p, n=n, batch=batch, num_inference_steps=steps, seed=seed).as_dict()
    b = defense_ldm.backdoor_features(pipe, defense_ldm.encode_trigger(pipe, p), n=n, batch=batch, num_inference_steps=steps, seed=seed).as_dict()
    assert a.pop("space") == "pixel" and b.pop("space") == "latent" and a == b
    # a stochastic sampler: the scheduler gets a device seed of its own for the call (seed + 1) and is left as it was found
    dd = fresh(S.DDPMScheduler())
    r1 = defense_ldm.backdoor_features(dd, tau, n=3, batch=2, num_inference_steps=3, seed=2)
    r2 = defense_ldm.backdoor_features(dd, tau, n=3, batch=2, num_inference_steps=3, seed=2)
    assert r1.as_dict() == r2.as_dict() and dd.scheduler.device_rng_seed is None and getattr(dd.scheduler, "_rng_offset", 0) == 0
    with pytest.raises(NotImplementedError, match="LDMPipeline"):                          # the VP module keeps its refusal
        mitigation.backdoor_features(pipe, tau, n=4, batch=2)


# ------------------------------------------------------------------------------------------------------------ 5. removal
def test_remove_backdoor_is_mitigation_on_the_latent_unet(tiny):
    _, _, fresh, _ = tiny
    tau = torch.rand(Z, generator=g(14))
    a, b = fresh(), fresh()
    vq0 = a.vqvae.flat_param.clone()
    ra = defense_ldm.remove_backdoor(a, tau, steps=3, batch=2, lr=2e-4, seed=4)
    rb = mitigation.remove_backdoor(b.unet, b.scheduler, tau, steps=3, batch=2, lr=2e-4, seed=4)
    assert (ra.total, ra.clean, ra.shift) == (rb.total, rb.clean, rb.shift) and torch.equal(a.unet.flat_param, b.unet.flat_param)
    assert torch.equal(a.vqvae.flat_param, vq0) and not torch.equal(a.unet.flat_param, fresh().unet.flat_param)
    # a pixel trigger is encoded once
    p = torch.rand(PX, generator=g(15)) * 2 - 1
    c, d = fresh(), fresh()
    rc = defense_ldm.remove_backdoor(c, p, steps=2, batch=2, lr=2e-4, seed=4)
    rd = mitigation.remove_backdoor(d.unet, d.scheduler, defense_ldm.encode_trigger(d, p), steps=2, batch=2, lr=2e-4, seed=4)
    assert rc.shift == rd.shift and torch.equal(c.unet.flat_param, d.unet.flat_param)


# ------------------------------------------------------------------------------------------------------------ 6. the tools
def test_tools_on_a_saved_ldm_checkpoint(tmp_path):
    """The three tools on the tiny LDM pipeline written by save_pretrained, each in a child process with a time limit."""
    from PIL import Image
    unet, vq = UNet2DModel(**UNET), VQModel(**VQ_NET)
    unet.reset_parameters(seed=1)
    vq.reset_parameters(seed=2)
    ckpt = str(tmp_path / "ldm")
    P.LDMPipeline(vqvae=vq, unet=unet, scheduler=S.DDIMScheduler()).save_pretrained(ckpt)

    def tool(name, *args):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name), "--ckpt", ckpt, *args], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]

    pipe = P.DiffusionPipeline.from_pretrained(ckpt)
    out = str(tmp_path / "inv")
    tool("invert_trigger.py", "--steps", "3", "--batch", "4", "--seed", "2", "--space", "pixel", "--out", out)
    info = json.load(open(os.path.join(out, "trigger_inv.json")))
    tf = os.path.join(out, "trigger_inv.pt")
    trig = torch.load(tf)
    png = np.asarray(Image.open(os.path.join(out, "trigger_inv.png")))
    assert info["space"] == "pixel" and info["steps"] == 3 and len(info["losses"]) == 3 and all(math.isfinite(x) for x in info["losses"])
    assert tuple(trig.shape) == PX and png.shape == (16, 16, 3) and png.dtype == np.uint8
    want = defense_ldm.invert_trigger(pipe, space="pixel", steps=3, batch=4, seed=2)
    assert torch.equal(trig, want.trigger.cpu()) and info["losses"] == want.losses
    assert np.array_equal(png, (P._post(trig[None].to(DEV))[0] * 255).round().astype("uint8"))
    od = str(tmp_path / "det")
    tool("detect_backdoor.py", "--trigger", tf, "--n", "5", "--batch", "2", "--steps", "3", "--seed", "2", "--out", od)
    det = json.load(open(os.path.join(od, "detection.json")))
    wantf = defense_ldm.backdoor_features(pipe, trig, n=5, batch=2, num_inference_steps=3, seed=2)
    assert det["space"] == "pixel" and det["pipeline"] == "LDMPipeline" and det["latent"] == wantf.as_dict()["latent"]
    assert det["clean"] == wantf.clean.as_dict() and det["uniformity_ratio"] == wantf.uniformity_ratio and "verdict" not in det
    assert tuple(torch.load(os.path.join(od, "mean_shifted.pt")).shape) == PX
    fixed = str(tmp_path / "fixed")
    tool("remove_backdoor.py", "--trigger", tf, "--steps", "3", "--batch", "2", "--seed", "2", "--out", fixed)
    rem = json.load(open(os.path.join(fixed, "removal.json")))
    assert rem["space"] == "pixel" and rem["steps"] == 3 and rem["lr"] == 2e-4 and all(len(rem[k]) == 3 for k in ("total", "clean", "shift"))
    after = P.DiffusionPipeline.from_pretrained(fixed)
    assert isinstance(after, P.LDMPipeline) and torch.equal(after.vqvae.flat_param, vq.flat_param) and not torch.equal(after.unet.flat_param, unet.flat_param)
    twin = P.DiffusionPipeline.from_pretrained(ckpt)
    res = defense_ldm.remove_backdoor(twin, torch.load(tf), steps=3, batch=2, lr=2e-4, seed=2)
    assert rem["shift"] == res.shift and torch.equal(after.unet.flat_param, twin.unet.flat_param)
