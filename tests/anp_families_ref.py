"""CPU restatement of villandiffusion_amd.anp_ve and villandiffusion_amd.anp_ldm for the tests (a helper module, not a test file; no GPU needed).

As tests/anp_ref.py does for the VP family: the neuron scales are applied to `oracle.ncsnpp_ref.NCSNppRef` / `oracle.unet_ref.UNet2DModelRef`
through `torch.func.functional_call` -- weight rows times (mask + delta), biases times (1 + xi) --, the loss is `oracle.loss_ref.LossFnRef`'s
(`SDE_VE, psi=0` / `SDE_LDM, psi=1`, a zero poison image) and autograd gives the gradients; nothing here uses the identity dL/dm_j = <g_j, w_j>
the HIP path rests on.  The element formulas of the kernels (`step`, `sign`, `grad_bound`) and `layer_max` are tests/anp_ref.py's, imported.

`oracle/ncsnpp_ref.py` does not run in float64 as it stands: its FIR kernel is built in f32 and `F.conv2d` refuses a double input beside it.
`upfirdn2d_native` is therefore wrapped from outside, here, casting the kernel to the input's dtype (a no-op in f32); oracle/ is not edited."""
import functools

import torch
from torch.func import functional_call

import oracle.ncsnpp_ref as _pp
from anp_ref import bias_of, grad_bound, layer_max, scaled_parameters, sign, step  # noqa: F401
from oracle.loss_ref import SDE_LDM, SDE_VE, LossFnRef
from oracle.schedulers_ref import DDIMSchedulerRef, ScoreSdeVeSchedulerRef

if not getattr(_pp.upfirdn2d_native, "_casts_kernel", False):
    _native = _pp.upfirdn2d_native

    @functools.wraps(_native)
    def _upfirdn2d_any_dtype(x, kernel, *args, **kwargs):
        return _native(x, kernel.to(x.dtype), *args, **kwargs)
    _upfirdn2d_any_dtype._casts_kernel = True
    _pp.upfirdn2d_native = _upfirdn2d_any_dtype

SMALL_PP = dict(sample_size=16, block_out_channels=(32, 64, 64), down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))        # + layers_per_block; test_defense_ve_gpu.py's
VE_SCHED = dict(num_train_timesteps=2000, sigma_min=0.01, sigma_max=380.0, snr=0.075)
VE_T = (0, 700, 1400, 1999)                                                                    # sigma = 0.01 ... 380
SMALL_LDM = dict(sample_size=8, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                 down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_defense_ldm_gpu.py's
LDM_T = (10, 300, 600, 950)
HEADS = ("conv_out.weight", "up_blocks.0.skip_conv.weight", "up_blocks.1.skip_conv.weight")    # NCSN++: rows are the image channels


def perturb_norms(ref):
    """test_defense_ve_gpu.py's: GroupNorm affines off their 1 / 0 initialisation, so that no gradient is degenerate."""
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))


def small_ncsnpp(layers_per_block=1):
    """The issue's small NCSN++ oracle: torch.manual_seed(1), norms perturbed by 0.1 * randn."""
    torch.manual_seed(1)
    ref = _pp.NCSNppRef(**SMALL_PP, layers_per_block=layers_per_block)
    perturb_norms(ref)
    return ref


def selected(ref, layers):
    """Names of the selected weights by the rule of the issue, from the oracle's parameters: anp_ref.selected with every weight whose rows are
    the output channels left out."""
    out = []
    for name, p in ref.named_parameters():
        if name == "conv_out.weight" or (name.startswith("up_blocks.") and name.endswith(".skip_conv.weight")):
            continue
        if (layers == "all" and p.dim() >= 2) or (layers == "conv" and p.dim() == 4 and name.endswith(".weight")):
            out.append(name)
    return out


def _loss(family, sched):
    if family == "ve":
        return LossFnRef(sched or ScoreSdeVeSchedulerRef(**VE_SCHED), SDE_VE, psi=0)
    return LossFnRef(sched or DDIMSchedulerRef(), SDE_LDM, psi=1)


def objective(family, ref, slices, n, clean, t, eps, mask, delta=None, xi=None, sched=None):
    """(loss, gmask, gxi): the family's clean loss at (mask + delta, 1 + xi) and its gradients by autograd, in the dtype of `ref`.
    family: "ve" (ref an NCSNppRef; t indexes the ascending training sigma table) or "ldm" (ref a UNet2DModelRef, clean latents)."""
    dtype = next(ref.parameters()).dtype
    s = (mask.to(dtype) + (delta.to(dtype) if delta is not None else 0)).detach().requires_grad_(True)
    sb = (1 + (xi.to(dtype) if xi is not None else torch.zeros(n, dtype=dtype))).detach().requires_grad_(True)
    scaled = scaled_parameters(ref, slices, s, sb)
    model = lambda x, tt, return_dict=False: functional_call(ref, scaled, (x, tt))
    loss = _loss(family, sched).p_loss(model, clean.to(dtype), torch.zeros_like(clean, dtype=dtype), t, noise=eps.to(dtype))
    gs, gb = torch.autograd.grad(loss, (s, sb), allow_unused=True)
    return loss.detach(), gs, gb if gb is not None else torch.zeros(n, dtype=dtype)


def learn(family, ref, slices, n, clean, *, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, timesteps, noise, perturbation=None,
          sched=None):
    """anp_ref.learn with this module's objective.  -> dict(mask, natural, robust, delta, xi, gm: the mask gradient of every step, gd: the last
    ascent gradient of delta)."""
    obj = lambda *a: objective(family, ref, slices, n, *a, sched=sched)
    mask, buf = torch.ones(n), torch.zeros(n)
    N = clean.shape[0]
    natural, robust, gms = [], [], []
    delta = xi = gd = None
    a = anp_eps / anp_steps
    for it in range(steps):
        idx = [(it * batch + k) % N for k in range(batch)]
        x0, t, eps = clean[idx], timesteps[it], noise[it]
        if anp_eps > 0:
            delta, xi = perturbation[it, 0].clone(), perturbation[it, 1].clone()
            for _ in range(anp_steps):
                _, gd, gx = obj(x0, t, eps, mask, delta, xi)
                delta, _ = step(delta, gd, None, -a, 0.0, -anp_eps, anp_eps, True)
                xi, _ = step(xi, gx, None, -a, 0.0, -anp_eps, anp_eps, True)
            l_rob, g_rob, _ = obj(x0, t, eps, mask, delta, xi)
            l_nat, g_nat, _ = obj(x0, t, eps, mask)
            gm = torch.tensor(1.0 - anp_alpha, dtype=torch.float32) * g_rob + torch.tensor(anp_alpha, dtype=torch.float32) * g_nat
            robust.append(float(l_rob))
        else:
            l_nat, gm, _ = obj(x0, t, eps, mask)
        natural.append(float(l_nat))
        gms.append(gm)
        mask, buf = step(mask, gm, buf, lr, momentum, 0.0, 1.0, False)
    return dict(mask=mask, natural=natural, robust=robust, delta=delta, xi=xi, gm=gms, gd=gd)


def ve_inputs(n, seed=7, steps=3, batch=4, images=8, size=16):
    """One set of inputs for the VE tests, CPU and GPU alike: clean images in [0, 1], unit noise, timesteps (step 0: VE_T), the uniform draws
    of the perturbation and a mask in [0.5, 1)."""
    gen = torch.Generator().manual_seed(seed)
    return dict(clean=torch.rand(images, 3, size, size, generator=gen), noise=torch.randn(steps, batch, 3, size, size, generator=gen),
                timesteps=torch.stack([torch.tensor(VE_T)] + [torch.randint(0, VE_SCHED["num_train_timesteps"], (batch,), generator=gen)
                                                              for _ in range(steps - 1)]),
                pert=(torch.rand(steps, 2, n, generator=gen) * 2 - 1) * 0.4, mask=torch.rand(n, generator=gen) * 0.5 + 0.5)


def ldm_inputs(n, seed=7, steps=3, batch=4, images=8):
    """The same for the latent UNet at 3 x 8 x 8: latents of unit scale, timesteps of 1000 (step 0: LDM_T)."""
    gen = torch.Generator().manual_seed(seed)
    return dict(clean=torch.randn(images, 3, 8, 8, generator=gen), noise=torch.randn(steps, batch, 3, 8, 8, generator=gen),
                timesteps=torch.stack([torch.tensor(LDM_T)] + [torch.randint(0, 1000, (batch,), generator=gen) for _ in range(steps - 1)]),
                pert=(torch.rand(steps, 2, n, generator=gen) * 2 - 1) * 0.4, mask=torch.rand(n, generator=gen) * 0.5 + 0.5)


def case_args(d, n, case):
    """(mask[, delta, xi]) of the two objective cases: "ones" and "random"."""
    return (d["mask"], d["pert"][0, 0], d["pert"][0, 1]) if case == "random" else (torch.ones(n),)


def layer_errors(got, want, slices):
    """(worst error, its layer): per layer max |got - want| relative to the layer's largest |want|, floored at 1e-4 of the whole vector's (the
    gate of tests/test_anp_gpu.py, for its reason: a layer whose gradient is analytically zero holds rounding noise alone)."""
    got, want = got.double(), want.double()
    floor = 1e-4 * float(want.abs().max())
    worst = (0.0, "")
    for name, sl in slices.items():
        err = float((got[sl] - want[sl]).abs().max() / (want[sl].abs().max() + floor))
        if err > worst[0]:
            worst = (err, name)
    return worst


def near_zero_share(g, slices, rel=1e-2):
    """(share, firm): the share of neurons whose gradient is within `rel` of zero on its layer's scale, and the bool vector of the others."""
    firm = torch.zeros(g.numel(), dtype=torch.bool)
    for name, sl in slices.items():
        firm[sl] = g[sl].abs() > rel * g[sl].abs().max()
    return 1.0 - float(firm.float().mean()), firm
