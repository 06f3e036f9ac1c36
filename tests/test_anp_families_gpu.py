"""Adversarial Neuron Pruning on NCSN++ (villandiffusion_amd.anp_ve) and latent diffusion (villandiffusion_amd.anp_ldm) on the GPU: the neuron
kernels at the row lengths the two families bring (3 floats; 16128 floats), anp_objective of both against the CPU oracle
(tests/anp_families_ref.py), the ascent step's signs, the mask trajectory, "the model is left alone", pruning_curve of all three modules, and
tools/anp_defense.py on an NCSN++ and an LDM checkpoint in child processes."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_families_ref as fam  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import anp, anp_ldm, anp_ve, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402
from villandiffusion_amd.vqmodel import VQModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP1 = dict(fam.SMALL_PP, layers_per_block=1)
VP_SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_anp_gpu.py's
VQ_NET = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3,
              down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2, sample_size=16)   # test_defense_ldm_gpu.py's


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ve_sched():
    return S.ScoreSdeVeScheduler(**fam.VE_SCHED)


# ------------------------------------------------------------------------------------------------------------ 1. the kernels at the new row lengths
SHAPES = ((5, 3), (6, 64), (3, 9216), (2, 16128))       # NCSN++'s down skip_conv rows; one item per lane; 1024 x 9; the LDM UNet's 1792 x 9


def synthetic_table():
    """Eight jobs, built like tests/test_anp_gpu.py's: every (rows, row length) with and without a bias.  Weight offsets alternate between
    multiples of four floats and 1 / 2 / 3 past one, so rows start aligned and unaligned whatever the row length (rows of 3 floats start
    unaligned three times in four anyway); five to eight unused floats lie between the pieces and 64 after the last."""
    jobs, cursor, neuron, block = [], 3, 0, 0
    for k, (rows, ln) in enumerate(s for s in SHAPES for _ in range(2)):
        off = (cursor + 3) // 4 * 4 + (k % 4 if k % 2 else 0)
        cursor = off + rows * ln + 5
        boff = -1
        if k % 2 == 0:
            boff, cursor = cursor, cursor + rows + 5
        jobs.append((off, rows, ln, boff, neuron, block))
        neuron += rows
        block += (rows + 3) // 4
    tab = anp.NeuronTable(jobs, neuron, {f"job{k}": slice(j[4], j[4] + j[1]) for k, j in enumerate(jobs)})
    assert tab.extent == cursor - 5 and any(j[0] % 4 for j in jobs) and any(j[0] % 4 == 0 for j in jobs)
    return tab, cursor + 64


def on_device(host, shift):
    """A device copy of `host` whose base pointer is `shift` floats past 16-byte alignment."""
    buf = torch.empty(host.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + host.numel()]
    v.copy_(host)
    return v


def scale_ref(w0, w_init, tab, mask, delta, xi):
    w = w_init.clone()
    for off, rows, ln, boff, n0, _ in tab.jobs:
        s = mask[n0:n0 + rows] if delta is None else mask[n0:n0 + rows] + delta[n0:n0 + rows]
        w[off:off + rows * ln] = (s[:, None] * w0[off:off + rows * ln].view(rows, ln)).reshape(-1)
        if boff >= 0:
            b = w0[boff:boff + rows]
            w[boff:boff + rows] = b if xi is None else (1.0 + xi[n0:n0 + rows]) * b
    return w


@pytest.mark.parametrize("shifts", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "both+4B", "w+4B"])
def test_neuron_scale_at_the_new_row_lengths(shifts):
    tab, numel = synthetic_table()
    n = tab.n_neurons
    gen = g(1)
    w0 = torch.randn(numel, generator=gen)
    mask, delta, xi = torch.rand(n, generator=gen), (torch.rand(n, generator=gen) * 2 - 1) * 0.4, (torch.rand(n, generator=gen) * 2 - 1) * 0.4
    hard = (torch.rand(n, generator=gen) < 0.5).float()                        # pruning_curve's masks: zeros and ones, no xi
    sentinel = torch.full((numel,), float("nan"))
    w0_d = on_device(w0, shifts[0])
    for m, d, x in ((mask, delta, xi), (mask, None, xi), (mask, delta, None), (mask, None, None), (hard, None, None)):
        w_d = on_device(sentinel, shifts[1])
        assert w_d.data_ptr() % 16 == 4 * shifts[1]
        up = lambda v: None if v is None else v.to(DEV)
        ops.neuron_scale(w0_d, w_d, tab, m.to(DEV), up(d), up(x))
        want = scale_ref(w0, sentinel, tab, m, d, x)
        assert torch.equal(bits(w_d), bits(want))                 # bit for bit, the NaN sentinel in the gaps and the tail included
        assert int(torch.isnan(want).sum()) == numel - tab.weight_floats - tab.n_bias
    assert torch.equal(bits(w0_d), bits(w0))
    # a mask of ones leaves every selected float its bits, and the biases too
    w_d = on_device(sentinel, shifts[1])
    ops.neuron_scale(w0_d, w_d, tab, torch.ones(n, device=DEV), None, None)
    keep = ~torch.isnan(w_d.cpu())
    assert torch.equal(bits(w_d)[keep], bits(w0)[keep]) and int(keep.sum()) == tab.weight_floats + tab.n_bias


def _grad(tab, gv, w0, shift, **kw):
    n = tab.n_neurons
    gm, gx = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    ops.neuron_grad(on_device(gv, shift), on_device(w0, shift), tab, gm, gx, **kw)
    return gm.cpu(), gx.cpu()


def test_neuron_grad_is_exact_on_integers_at_the_new_row_lengths():
    tab, numel = synthetic_table()
    gen = g(2)
    gv = torch.randint(-4, 5, (numel,), generator=gen).float()
    w0 = torch.randint(-4, 5, (numel,), generator=gen).float()               # |row sum| <= 16128 * 16 < 2^24: exact in f32 in any order
    want_m = torch.zeros(tab.n_neurons, dtype=torch.int64)
    want_x = torch.zeros(tab.n_neurons, dtype=torch.int64)
    has_bias = torch.zeros(tab.n_neurons, dtype=torch.bool)
    for off, rows, ln, boff, n0, _ in tab.jobs:
        want_m[n0:n0 + rows] = (gv[off:off + rows * ln].long() * w0[off:off + rows * ln].long()).view(rows, ln).sum(1)
        if boff >= 0:
            want_x[n0:n0 + rows] = gv[boff:boff + rows].long() * w0[boff:boff + rows].long()
            has_bias[n0:n0 + rows] = True
    assert int(want_m.abs().max()) > 200                                      # the long rows do add up to something
    for shift in (0, 1):
        gm, gx = _grad(tab, gv, w0, shift)
        assert torch.equal(gm, want_m.float())
        assert torch.equal(gx[has_bias], want_x[has_bias].float()) and bool(torch.isnan(gx[~has_bias]).all())      # bias-less jobs: untouched
    assert 0 < int(has_bias.sum()) < tab.n_neurons


def test_neuron_grad_accuracy_at_the_new_row_lengths():
    """The existing gate, anp_ref.grad_bound = min(n, 128) 2^-24 sum|g w0|: the kernel's longest addition chain at 16128 floats is 63 products
    per lane and position, then 2 + 6 additions -- 71 < 128 -- so the gate that held at 4608 is the right one here."""
    tab, numel = synthetic_table()
    gen = g(3)
    gv, w0 = torch.randn(numel, generator=gen), torch.randn(numel, generator=gen)
    gm, gx = _grad(tab, gv, w0, 0)
    worst = 0.0
    for off, rows, ln, boff, n0, _ in tab.jobs:
        a, b = gv[off:off + rows * ln].double().view(rows, ln), w0[off:off + rows * ln].double().view(rows, ln)
        err = (gm[n0:n0 + rows].double() - (a * b).sum(1)).abs()
        bound = fam.grad_bound(ln, a, b)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"[parity] neuron_grad rows of {ln}: worst error / (min(n, 128) 2^-24 sum|g w0|) = {ratio:.3f}")
        assert bool((err <= bound).all())
        if boff >= 0:
            assert torch.equal(gx[n0:n0 + rows], gv[boff:boff + rows] * w0[boff:boff + rows])
    print(f"[parity] neuron_grad worst ratio at the new row lengths {worst:.3f}")
    again = _grad(tab, gv, w0, 0)                                             # fixed order: a repeat and a shifted base pointer give equal bits
    odd = _grad(tab, gv, w0, 1)
    for other in (again, odd):
        assert torch.equal(bits(other[0]), bits(gm)) and torch.equal(bits(other[1]), bits(gx))


# ------------------------------------------------------------------------------------------------------------ 2. anp_ve against the oracle
@pytest.fixture(scope="module")
def ve():
    ref = fam.small_ncsnpp(1)                                                 # the CPU test's exact set-up
    tab = anp_ve.neuron_table(NCSNppModel(**PP1, device="cpu"), "all")
    assert (tab.n_jobs, tab.n_neurons) == (73, 4256)
    data = fam.ve_inputs(tab.n_neurons)
    cache = {}

    def fresh(math_mode="bf16x3"):
        net = NCSNppModel(**PP1)
        net.load_state_dict(ref.state_dict())
        net.conv_math = math_mode
        return net

    def oracle(case):
        if case not in cache:
            cache[case] = fam.objective("ve", ref, tab.slices, tab.n_neurons, data["clean"][:4], data["timesteps"][0], data["noise"][0],
                                        *fam.case_args(data, tab.n_neurons, case))
        return cache[case]
    return ref, fresh, tab, data, oracle


def _check_objective(label, got, want, tab):
    loss, gmask, gxi = got
    want_l, want_m, want_x = want
    e_l = abs(float(loss) - float(want_l)) / abs(float(want_l))
    e_m, e_x = fam.layer_errors(gmask.cpu(), want_m, tab.slices), fam.layer_errors(gxi.cpu(), want_x, tab.slices)
    print(f"[parity] {label}: loss {float(loss):.6f} (oracle {float(want_l):.6f}, rel {e_l:.2e}); worst layer gmask {e_m[0]:.2e} at {e_m[1]}, "
          f"gxi {e_x[0]:.2e} at {e_x[1]}")
    assert e_l <= 1e-5 and e_m[0] <= 1e-3 and e_x[0] <= 1e-3


@pytest.mark.parametrize("case", ["ones", "random"])
@pytest.mark.parametrize("math_mode", ["bf16x3", "f32"])
def test_ve_objective_matches_oracle(ve, math_mode, case):
    """Gates: the project's -- loss 1e-5 relative; gmask and gxi per layer 1e-3 of the layer's largest entry, floored at 1e-4 of the vector's."""
    ref, fresh, tab, d, oracle = ve
    net = fresh(math_mode)
    before = net.flat_param.clone()
    flags = [p.requires_grad for p in net.parameters()]
    fourier = net.time_proj.weight.detach().clone()
    got = anp_ve.anp_objective(net, ve_sched(), d["clean"][:4], d["timesteps"][0], d["noise"][0], *fam.case_args(d, tab.n_neurons, case))
    assert torch.equal(bits(net.flat_param), bits(before)) and [p.requires_grad for p in net.parameters()] == flags
    assert not net.time_proj.weight.requires_grad and sum(flags) == len(flags) - 1 and torch.equal(bits(net.time_proj.weight), bits(fourier))
    _check_objective(f"anp_ve.anp_objective ({math_mode}, {case})", got, oracle(case), tab)


# ------------------------------------------------------------------------------------------------------------ 3. signs and trajectory
def _check_signs(label, res, want, tab):
    share, firm = fam.near_zero_share(want["gd"], tab.slices)
    mismatch = int((res.last_delta[firm] != want["delta"][firm]).sum())
    print(f"[parity] {label} ascent signs: {share:.1%} of {tab.n_neurons} neurons excluded (oracle gradient within 1e-2 of zero on its layer's "
          f"scale); {mismatch} mismatches on the rest, {int((res.last_delta != want['delta']).sum())} in all")
    assert share <= 0.10
    assert mismatch == 0
    lim = float(torch.tensor(0.4, dtype=torch.float32))
    assert float(res.last_delta.abs().max()) <= lim and float(res.last_xi.abs().max()) <= lim
    assert len(res.natural) == len(res.robust) == 1 and abs(res.natural[0] - want["natural"][0]) <= 1e-5 * want["natural"][0]


def _check_trajectory(label, res, want, tab, lr):
    got = res.flat()
    worst = (0.0, "")
    for name, sl in tab.slices.items():
        assert torch.equal(res.masks[name], got[sl])
        bound = 2 * lr * sum(1e-3 * float(gm[sl].abs().max()) for gm in want["gm"])
        ratio = float((got[sl] - want["mask"][sl]).abs().max()) / bound
        if ratio > worst[0]:
            worst = (ratio, name)
    moved = float((want["mask"] - 1.0).abs().max())
    print(f"[parity] {label} mask trajectory: worst |m - m_ref| / bound {worst[0]:.3f} at {worst[1]}; the oracle's mask moved up to {moved:.3e} from 1")
    assert worst[0] <= 1.0 and moved > 0.0
    assert res.robust == [] and len(res.natural) == 3
    assert abs(res.natural[0] - want["natural"][0]) <= 1e-5 * want["natural"][0]          # step 0: the same mask, the loss gate


SIGNS = dict(steps=1, batch=4, anp_eps=0.4, anp_steps=1, anp_alpha=0.2, lr=0.2, momentum=0.9)
TRAJECTORY = dict(steps=3, batch=4, anp_eps=0.0, anp_steps=1, anp_alpha=0.2, lr=2.0, momentum=0.0)


def test_ve_ascent_step_signs_match_the_oracle(ve):
    """tests/test_anp_gpu.py's sign test on the small NCSN++: delta after one step's ascent equals the oracle's wherever the oracle's gradient
    exceeds 1e-2 of its layer's largest; at most 10 % of the neurons are excluded."""
    ref, fresh, tab, d, _ = ve
    want = fam.learn("ve", ref, tab.slices, tab.n_neurons, d["clean"], timesteps=d["timesteps"], noise=d["noise"], perturbation=d["pert"], **SIGNS)
    res = anp_ve.learn_neuron_mask(fresh(), ve_sched(), d["clean"], layers="all", timesteps=d["timesteps"][:1], noise=d["noise"][:1],
                                   perturbation=d["pert"][:1], **SIGNS)
    _check_signs("VE", res, want, tab)


def test_ve_mask_trajectory_follows_the_restated_loop(ve):
    """tests/test_anp_gpu.py's trajectory test on the small NCSN++: anp_eps = 0, momentum = 0, lr = 2, three steps; per layer
    |m - m_ref| <= 2 * lr * sum_s 1e-3 * max_j |g_s,j| (first order from the gradient gate, doubled for the feedback into later steps)."""
    ref, fresh, tab, d, _ = ve
    want = fam.learn("ve", ref, tab.slices, tab.n_neurons, d["clean"], timesteps=d["timesteps"], noise=d["noise"], **TRAJECTORY)
    res = anp_ve.learn_neuron_mask(fresh(), ve_sched(), d["clean"], layers="all", timesteps=d["timesteps"], noise=d["noise"], **TRAJECTORY)
    _check_trajectory("VE", res, want, tab, TRAJECTORY["lr"])


# ------------------------------------------------------------------------------------------------------------ 4. anp_ldm on the tiny pipeline
@pytest.fixture(scope="module")
def ldm():
    torch.manual_seed(0)
    uref = UNet2DModelRef(**fam.SMALL_LDM)
    fam.perturb_norms(uref)
    tab = anp.neuron_table(UNet2DModel(**fam.SMALL_LDM, device="cpu"), "all")
    assert (tab.n_jobs, tab.n_neurons) == (50, 2912)
    data = fam.ldm_inputs(tab.n_neurons)
    data["pixels"] = torch.rand(8, 3, 16, 16, generator=g(11)) * 2 - 1
    vq0 = VQModel(**VQ_NET)
    vq0.reset_parameters(seed=2)
    cache = {}

    def fresh(math_mode="bf16x3"):
        unet, vq = UNet2DModel(**fam.SMALL_LDM), VQModel(**VQ_NET)
        unet.load_state_dict(uref.state_dict())
        with torch.no_grad():
            vq.flat_param.copy_(vq0.flat_param)
        unet.conv_math = math_mode
        return P.LDMPipeline(vqvae=vq, unet=unet, scheduler=S.DDIMScheduler())

    def oracle(case):
        if case not in cache:
            cache[case] = fam.objective("ldm", uref, tab.slices, tab.n_neurons, data["clean"][:4], data["timesteps"][0], data["noise"][0],
                                        *fam.case_args(data, tab.n_neurons, case))
        return cache[case]
    return uref, fresh, tab, data, oracle


@pytest.mark.parametrize("case", ["ones", "random"])
@pytest.mark.parametrize("math_mode", ["bf16x3", "f32"])
def test_ldm_objective_matches_oracle(ldm, math_mode, case):
    uref, fresh, tab, d, oracle = ldm
    pipe = fresh(math_mode)
    before, vq_before = pipe.unet.flat_param.clone(), pipe.vqvae.flat_param.clone()
    flags = [p.requires_grad for p in pipe.unet.parameters()]
    got = anp_ldm.anp_objective(pipe, d["clean"][:4], d["timesteps"][0], d["noise"][0], *fam.case_args(d, tab.n_neurons, case))
    assert torch.equal(bits(pipe.unet.flat_param), bits(before)) and [p.requires_grad for p in pipe.unet.parameters()] == flags
    assert torch.equal(bits(pipe.vqvae.flat_param), bits(vq_before))
    _check_objective(f"anp_ldm.anp_objective ({math_mode}, {case}, latent clean)", got, oracle(case), tab)


def test_ldm_pixel_clean_is_encoded_in_chunks_of_batch(ldm):
    """Pixel-shaped clean images give the bits of passing `pipeline.encode` of the same chunks; the VQ-VAE is never written."""
    uref, fresh, tab, d, _ = ldm
    pipe = fresh()
    vq_before = pipe.vqvae.flat_param.clone()
    vq_flags = [p.requires_grad for p in pipe.vqvae.parameters()]
    kw = dict(steps=3, batch=3, anp_eps=0.4, layers="conv", seed=5)              # 8 images in chunks of 3, 3, 2; the batch wraps in step 2
    px = anp_ldm.learn_neuron_mask(pipe, d["pixels"], **kw)
    with torch.no_grad():
        z = torch.cat([pipe.encode(d["pixels"][i:i + 3].to(DEV)) for i in range(0, 8, 3)])
    assert tuple(z.shape) == (8, 3, 8, 8) and anp_ldm.clean_space(pipe, z) == "latent"
    lat = anp_ldm.learn_neuron_mask(fresh(), z, **kw)
    assert torch.equal(bits(px.flat()), bits(lat.flat())) and px.natural == lat.natural and px.robust == lat.robust
    assert float(px.flat().min()) < 1.0 and all(math.isfinite(v) for v in px.natural + px.robust)
    assert torch.equal(bits(pipe.vqvae.flat_param), bits(vq_before)) and [p.requires_grad for p in pipe.vqvae.parameters()] == vq_flags
    t, eps, m = d["timesteps"][0], d["noise"][0], torch.ones(tab.n_neurons)
    a = anp_ldm.anp_objective(pipe, d["pixels"][:4], t, eps, m)                  # one evaluation: the images are one chunk
    with torch.no_grad():
        z4 = pipe.encode(d["pixels"][:4].to(DEV))
    b = anp_ldm.anp_objective(pipe, z4, t, eps, m)
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b)) and math.isfinite(float(a[0]))
    assert torch.equal(bits(pipe.vqvae.flat_param), bits(vq_before))


def test_ldm_mask_trajectory_follows_the_restated_loop(ldm):
    uref, fresh, tab, d, _ = ldm
    want = fam.learn("ldm", uref, tab.slices, tab.n_neurons, d["clean"], timesteps=d["timesteps"], noise=d["noise"], **TRAJECTORY)
    res = anp_ldm.learn_neuron_mask(fresh(), d["clean"], layers="all", timesteps=d["timesteps"], noise=d["noise"], **TRAJECTORY)
    _check_trajectory("LDM", res, want, tab, TRAJECTORY["lr"])


# ------------------------------------------------------------------------------------------------------------ 5. the model is left alone
def _families(ve, ldm):
    """(label, fresh() -> (target tuple, network), learn, data) for the two new modules."""
    _, fresh_ve, _, d_ve, _ = ve
    _, fresh_ldm, _, d_ldm, _ = ldm

    def make_ve():
        net = fresh_ve()
        return (net, ve_sched()), net

    def make_ldm():
        pipe = fresh_ldm()
        return (pipe,), pipe.unet
    return (("VE", make_ve, anp_ve, d_ve, lambda net, x, t: net(x, t.float() + 1.0)[0]),             # (a positive noise level per image)
            ("LDM", make_ldm, anp_ldm, d_ldm, lambda net, x, t: net(x, t)[0]))


@pytest.mark.parametrize("which", [0, 1], ids=["ve", "ldm"])
def test_learning_a_mask_leaves_the_model_alone(ve, ldm, which):
    label, make, mod, d, call = _families(ve, ldm)[which]
    target, net = make()
    list(net.parameters())[3].requires_grad_(False)                            # a mix of frozen and trainable parameters comes back as it was
    flags = [p.requires_grad for p in net.parameters()]
    x, t = d["noise"][0].to(DEV), d["timesteps"][0].to(DEV)
    with torch.no_grad():
        out_before = call(net, x, t).clone()
    before = net.flat_param.clone()
    kw = dict(steps=3, batch=4, anp_eps=0.4, layers="all")
    res = mod.learn_neuron_mask(*target, d["clean"], **kw)
    assert float(res.flat().min()) < 1.0                                       # the loop did run on scaled weights
    assert torch.equal(bits(net.flat_param), bits(before)) and [p.requires_grad for p in net.parameters()] == flags and not flags[3]
    with torch.no_grad():
        assert torch.equal(bits(call(net, x, t)), bits(out_before))            # caches were invalidated and rebuilt from the restored weights

    def boom(i):
        if i == 1:
            raise RuntimeError("boom")                                         # the second step: the weights are scaled at that moment
        return d["noise"][i]
    with pytest.raises(RuntimeError, match="boom"):
        mod.learn_neuron_mask(*target, d["clean"], noise=boom, **kw)
    assert torch.equal(bits(net.flat_param), bits(before)) and [p.requires_grad for p in net.parameters()] == flags
    with torch.no_grad():
        assert torch.equal(bits(call(net, x, t)), bits(out_before))
    assert float(net.flat_grad.abs().max()) == 0.0


@pytest.mark.parametrize("which", [0, 1], ids=["ve", "ldm"])
def test_learning_is_deterministic(ve, ldm, which):
    label, make, mod, d, _ = _families(ve, ldm)[which]
    kw = dict(steps=3, batch=4, anp_eps=0.4, anp_steps=2, lr=0.2, momentum=0.9, layers="conv", seed=3)
    a, b = (mod.learn_neuron_mask(*make()[0], d["clean"], **kw) for _ in range(2))
    m = a.flat()
    assert 0.0 <= float(m.min()) and float(m.max()) <= 1.0 and float(m.min()) < 1.0 and a.settings()["anp_steps"] == 2
    assert len(a.natural) == len(a.robust) == 3 and all(math.isfinite(v) and v > 0 for v in a.natural + a.robust)
    assert torch.equal(bits(m), bits(b.flat())) and a.natural == b.natural and a.robust == b.robust     # Philox noise, fixed summation orders
    c = mod.learn_neuron_mask(*make()[0], d["clean"], **(kw | dict(seed=4)))
    assert c.natural != a.natural
    curves = [mod.pruning_curve(*make()[0], d["clean"][:4], r, fractions=(0.02, 0.05), seed=3) for r in (a, b)]
    assert curves[0] == curves[1] and len(curves[0]) == 3
    # a tensor and a callable give the same run
    t1 = mod.learn_neuron_mask(*make()[0], d["clean"], timesteps=d["timesteps"], noise=d["noise"], perturbation=d["pert"], **(kw | dict(layers="all")))
    t2 = mod.learn_neuron_mask(*make()[0], d["clean"], timesteps=lambda i: d["timesteps"][i], noise=lambda i: d["noise"][i],
                               perturbation=lambda i: d["pert"][i], **(kw | dict(layers="all")))
    assert torch.equal(bits(t1.flat()), bits(t2.flat())) and t1.robust == t2.robust


# ------------------------------------------------------------------------------------------------------------ 6. pruning_curve
def _vp_family():
    net0 = UNet2DModel(**VP_SMALL, device="cpu")
    net0.reset_parameters(1)
    gen = g(9)
    d = dict(clean=torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1, noise=torch.randn(1, 4, 3, 32, 32, generator=gen),
             timesteps=torch.tensor([[10, 300, 600, 950]]))

    def make():
        net = UNet2DModel(**VP_SMALL)
        with torch.no_grad():
            net.flat_param.copy_(net0.flat_param)
        return (net, S.DDPMScheduler()), net
    return "VP", make, anp, d


@pytest.mark.parametrize("which", [0, 1, 2], ids=["ve", "ldm", "vp"])
def test_pruning_curve(ve, ldm, which):
    """Record 0 is the loss of anp_objective at mask = 1 on the same inputs; every later record is record 0's computation on a twin network
    pruned by prune_neurons with the same selection -- both to the loss gate 1e-5 (the training forward and the no-grad forward may take
    different kernels: a gate, not bits); `pruned` is prune_neurons' total; the model keeps its bits."""
    label, make, mod, d = (_families(ve, ldm) + (_vp_family(),))[which][:4]
    target, net = make()
    tab = anp.neuron_table(net, "conv")
    flat = torch.rand(tab.n_neurons, generator=g(21)) * 0.9 + 0.1
    masks = {name: flat[sl].clone() for name, sl in tab.slices.items()}
    x0, t, eps = d["clean"][:4], d["timesteps"][0], d["noise"][0]
    before = net.flat_param.clone()
    fractions = (0.02, 0.05)
    curve = mod.pruning_curve(*target, x0, masks, fractions=fractions, timesteps=t, noise=eps)
    assert torch.equal(bits(net.flat_param), bits(before))
    assert [r["fraction"] for r in curve] == [None, 0.02, 0.05] and curve[0]["pruned"] == 0 and all(math.isfinite(r["loss"]) for r in curve)
    full = anp.neuron_table(net, "all")
    want0 = float(mod.anp_objective(*target, x0, t, eps, torch.ones(full.n_neurons))[0])
    e0 = abs(curve[0]["loss"] - want0) / want0
    errs = []
    for f, rec in zip(fractions, curve[1:]):
        twin_target, twin = make()
        counts = mod.prune_neurons(twin_target[0], masks, fraction=f)
        assert rec["pruned"] == sum(counts.values()) == int(math.floor(f * tab.n_neurons))
        want = mod.pruning_curve(*twin_target, x0, masks, fractions=(), timesteps=t, noise=eps)
        assert len(want) == 1
        errs.append(abs(rec["loss"] - want[0]["loss"]) / want[0]["loss"])
        assert rec["loss"] != curve[0]["loss"]                                 # zeroing 2 % of the rows does move the loss
    print(f"[parity] {label} pruning_curve: losses {[round(r['loss'], 6) for r in curve]}; record 0 vs anp_objective at mask 1 rel {e0:.2e}; "
          f"records vs a pruned twin rel {[f'{e:.2e}' for e in errs]}")
    assert e0 <= 1e-5 and all(e <= 1e-5 for e in errs)
    # thresholds are read as prune_neurons reads them
    by_t = mod.pruning_curve(*target, x0, masks, thresholds=(0.15,), timesteps=t, noise=eps)
    assert by_t[1]["threshold"] == 0.15 and by_t[1]["pruned"] == int((flat < 0.15).sum()) and by_t[0]["loss"] == curve[0]["loss"]
    # a candidate that empties a layer raises before anything is written; the model has its bits after an exception inside the loop too
    victim = list(tab.slices)[2]
    rows = masks[victim].numel()
    bad = masks | {victim: torch.zeros(rows)}
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        mod.pruning_curve(*target, x0, bad, fractions=(0.001, (rows + 0.5) / tab.n_neurons), timesteps=t, noise=eps)
    assert torch.equal(bits(net.flat_param), bits(before))
    calls = []
    real = net.weights_changed

    def changed():
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("boom")                                         # the second candidate's weights have just been written
        real()
    net.weights_changed = changed
    try:
        with pytest.raises(RuntimeError, match="boom"):
            mod.pruning_curve(*target, x0, masks, fractions=fractions, timesteps=t, noise=eps)
    finally:
        del net.weights_changed
    assert torch.equal(bits(net.flat_param), bits(before))
    again = mod.pruning_curve(*target, x0, masks, fractions=fractions, timesteps=t, noise=eps)
    assert again == curve


# ------------------------------------------------------------------------------------------------------------ 7. the tool
def _run_tool(ckpt, out):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "anp_defense.py"), "--ckpt", ckpt, "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "16",
                          "--steps", "2", "--batch", "4", "--fraction", "0.05", "--sweep", "0.02,0.05", "--out", out],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1]), json.load(open(os.path.join(out, "anp.json"))), torch.load(os.path.join(out, "anp_mask.pt"))


def _check_tool_record(info, line, counts, tab, family):
    k = int(math.floor(0.05 * tab.n_neurons))
    assert info["family"] == family and len(info["natural"]) == len(info["robust"]) == 2
    assert all(math.isfinite(v) for v in info["natural"] + info["robust"])
    assert sum(info["pruned"].values()) == info["pruned_total"] == k == line["pruned_total"] and info["pruned"] == counts
    assert (info["steps"], info["batch"], info["layers"], info["fraction"], info["n_clean"], info["n_neurons"]) == (2, 4, "conv", 0.05, 16, tab.n_neurons)
    curve = info["curve"]
    assert len(curve) == 3 and [r["fraction"] for r in curve] == [None, 0.02, 0.05] and all(math.isfinite(r["loss"]) and r["loss"] > 0 for r in curve)
    assert [r["pruned"] for r in curve] == [0, int(math.floor(0.02 * tab.n_neurons)), k]


def test_tool_on_an_ncsnpp_checkpoint(tmp_path):
    net = NCSNppModel(**PP1)
    net.reset_parameters(seed=1)
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "pruned")
    P.ScoreSdeVePipeline(net, ve_sched()).save_pretrained(ckpt)
    line, info, masks = _run_tool(ckpt, out)
    pruned = P.DiffusionPipeline.from_pretrained(out).unet
    tab = anp_ve.neuron_table(net, "conv")
    assert type(pruned).__name__ == "NCSNppModel" and list(masks) == list(tab.slices)
    twin = NCSNppModel(**PP1, device="cpu")
    twin.flat_param.data.copy_(net.flat_param.cpu())
    counts = anp_ve.prune_neurons(twin, masks, fraction=0.05)                  # the selection the masks imply, applied to the input checkpoint
    assert torch.equal(bits(pruned.flat_param), bits(twin.flat_param))         # the pruned rows are zero, every other parameter has its bits
    assert torch.equal(bits(pruned.time_proj.weight), bits(net.time_proj.weight))
    _check_tool_record(info, line, counts, tab, "ve")
    assert "space" not in info


def test_tool_on_an_ldm_checkpoint(tmp_path):
    unet, vq = UNet2DModel(**fam.SMALL_LDM), VQModel(**VQ_NET)
    unet.reset_parameters(seed=1)
    vq.reset_parameters(seed=2)
    ckpt, out = str(tmp_path / "ldm"), str(tmp_path / "pruned")
    P.LDMPipeline(vqvae=vq, unet=unet, scheduler=S.DDIMScheduler()).save_pretrained(ckpt)
    line, info, masks = _run_tool(ckpt, out)
    pruned = P.DiffusionPipeline.from_pretrained(out)
    tab = anp.neuron_table(unet, "conv")
    assert type(pruned).__name__ == "LDMPipeline" and list(masks) == list(tab.slices)
    twin = UNet2DModel(**fam.SMALL_LDM, device="cpu")
    twin.flat_param.data.copy_(unet.flat_param.cpu())
    counts = anp.prune_neurons(twin, masks, fraction=0.05)
    assert torch.equal(bits(pruned.unet.flat_param), bits(twin.flat_param))
    assert torch.equal(bits(pruned.vqvae.flat_param), bits(vq.flat_param))     # the VQ-VAE went through untouched
    _check_tool_record(info, line, counts, tab, "ldm")
    assert info["space"] == "pixel"
