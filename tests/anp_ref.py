"""CPU restatement of villandiffusion_amd.anp for the tests (a helper module, not a test file; no GPU needed).

The neuron scales are applied to `oracle.unet_ref.UNet2DModelRef` through `torch.func.functional_call` -- weight rows times (mask + delta), biases
times (1 + xi) -- and autograd gives the mask gradients; nothing here uses the identity dL/dm_j = <g_j, w_j> the HIP path rests on.  The learning
loop and the three kernels' element formulas are restated in plain torch, op by op.

Per-neuron vectors are laid out by `slices` (weight name -> slice), which the tests take from `anp.neuron_table`; `selected` restates the
selection rule on the oracle's own parameters so that the table can be checked against it."""
import math

import torch
from torch.func import functional_call

from oracle.loss_ref import SDE_VP, LossFnRef
from oracle.schedulers_ref import DDPMSchedulerRef


def selected(ref, layers):
    """Names of the selected weights, by the rule of the issue, from the oracle's parameters (order: the oracle's, not the table's)."""
    out = []
    for name, p in ref.named_parameters():
        if name == "conv_out.weight":
            continue
        if (layers == "all" and p.dim() >= 2) or (layers == "conv" and p.dim() == 4 and name.endswith(".weight")):
            out.append(name)
    return out


def bias_of(ref, name):
    b = name[:-len("weight")] + "bias"
    return b if b in dict(ref.named_parameters()) else None


def scaled_parameters(ref, slices, s, sb):
    """name -> tensor for functional_call: rows of every selected weight times s[slice], its bias times sb[slice]."""
    params = dict(ref.named_parameters())
    out = {}
    for name, sl in slices.items():
        w = params[name]
        out[name] = w * s[sl].to(w.dtype).reshape((-1,) + (1,) * (w.dim() - 1))
        b = bias_of(ref, name)
        if b is not None:
            out[b] = params[b] * sb[sl].to(w.dtype)
    return out


def objective(ref, slices, n, clean, t, eps, mask, delta=None, xi=None, sched=None):
    """(loss, gmask, gxi): the clean noise-prediction loss at (mask + delta, 1 + xi) and its gradients by autograd, in the dtype of `ref`."""
    dtype = next(ref.parameters()).dtype
    sched = sched or DDPMSchedulerRef()
    s = (mask.to(dtype) + (delta.to(dtype) if delta is not None else 0)).detach().requires_grad_(True)
    sb = (1 + (xi.to(dtype) if xi is not None else torch.zeros(n, dtype=dtype))).detach().requires_grad_(True)
    scaled = scaled_parameters(ref, slices, s, sb)
    model = lambda x, tt, return_dict=False: functional_call(ref, scaled, (x, tt))
    loss = LossFnRef(sched, SDE_VP, psi=1).p_loss(model, clean.to(dtype), torch.zeros_like(clean, dtype=dtype), t, noise=eps.to(dtype))
    gs, gb = torch.autograd.grad(loss, (s, sb), allow_unused=True)
    return loss.detach(), gs, gb if gb is not None else torch.zeros(n, dtype=dtype)


def sign(g):
    return (g > 0).to(g.dtype) - (g < 0).to(g.dtype)               # torch.sign: 0 for +-0 (and NaN)


def step(x, g, buf, lr, momentum, lo, hi, use_sign):
    """vd_neuron_step in f32 torch ops, one rounding each, in the documented order.  -> (x, buf)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    if buf is not None:
        d = buf = buf * f(momentum) + g
    else:
        d = sign(g) if use_sign else g
    return torch.minimum(torch.maximum(x - f(lr) * d, f(lo)), f(hi)), buf


def learn(ref, slices, n, clean, *, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, timesteps, noise, perturbation=None):
    """The loop of `learn_neuron_mask` with oracle gradients.  -> dict(mask, natural, robust, delta, xi, gm: the mask gradient of every step,
    gd: the last ascent gradient of delta)."""
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
                _, gd, gx = objective(ref, slices, n, x0, t, eps, mask, delta, xi)
                delta, _ = step(delta, gd, None, -a, 0.0, -anp_eps, anp_eps, True)
                xi, _ = step(xi, gx, None, -a, 0.0, -anp_eps, anp_eps, True)
            l_rob, g_rob, _ = objective(ref, slices, n, x0, t, eps, mask, delta, xi)
            l_nat, g_nat, _ = objective(ref, slices, n, x0, t, eps, mask)
            gm = torch.tensor(1.0 - anp_alpha, dtype=torch.float32) * g_rob + torch.tensor(anp_alpha, dtype=torch.float32) * g_nat
            robust.append(float(l_rob))
        else:
            l_nat, gm, _ = objective(ref, slices, n, x0, t, eps, mask)
        natural.append(float(l_nat))
        gms.append(gm)
        mask, buf = step(mask, gm, buf, lr, momentum, 0.0, 1.0, False)
    return dict(mask=mask, natural=natural, robust=robust, delta=delta, xi=xi, gm=gms, gd=gd)


def layer_max(v, slices):
    """name -> max |v| over the layer's neurons."""
    return {name: float(v[sl].abs().max()) for name, sl in slices.items()}


def grad_bound(n_row, g, w0):
    """The accuracy gate of vd_neuron_grad: min(n, 128) * 2^-24 * sum_k |g_k * w0_k| per row (g, w0: [rows, n] float64)."""
    return min(n_row, 128) * 2.0 ** -24 * (g * w0).abs().sum(1)
