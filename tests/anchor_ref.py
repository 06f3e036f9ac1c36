"""The anchored optimiser step restated in torch on the oracle (UNet2DModelRef, LossFnRef, torch.optim.Adam, clip_grad_norm_): what
`Trainer(anchor=AnchorConfig(...))` is held to, plus the inputs and bounds the anchor tests share.

One optimiser step: loss = mean over the micro-batches of the step of the oracle's loss, plus the penalty WRITTEN IN TORCH,
    lam / 2 * sum_i F_i (w_i - w0_i)^2          (F = 1: L2-SP),
once per optimiser step; autograd; clip_grad_norm_(1.0), Adam, cosine schedule.  lam = 0 (mode None) is the plain step.

The trajectory tests use LAM, `fisher_of` (non-uniform, seeded) and `anchor_of` (the start plus a seeded perturbation, so the penalty acts from
step one); tests/test_anchor_cpu.py checks on the CPU that with them the anchored trajectory lies at least 0.1 away from the plain one."""
import numpy as np
import torch

import oracle.schedulers_ref as R
import sam_ref
from oracle.loss_ref import SDE_VP, LossFnRef

SMALL = sam_ref.SMALL
batch_of = sam_ref.batch_of
update_l2_error = sam_ref.update_l2_error
sum_bound = sam_ref.sum_bound

LAM = 0.1                  # the lambda of the trajectory tests
W0_SIGMA = 0.005           # w0 = start + W0_SIGMA * N(0, 1)
MODES = ("l2sp", "ewc")


def g(seed):
    return torch.Generator().manual_seed(seed)


def fisher_of(numel, seed=11):
    """A non-uniform stand-in for a normalised Fisher: log-normal, mean about 1, spread over three decades."""
    return torch.exp(1.5 * torch.randn(numel, generator=g(seed)) - 1.125).float()


def anchor_of(flat_start, seed=12):
    return (flat_start + W0_SIGMA * torch.randn(flat_start.numel(), generator=g(seed))).float()


def named(flat, offs):
    """name -> tensor views of a flat host tensor, by the network's offsets (name -> (offset, numel, shape))."""
    return {k: flat[off:off + n].view(shape) for k, (off, n, shape) in offs.items()}


def penalty(params, w0, F, lam):
    """lam / 2 * sum F (w - w0)^2 in torch, differentiable.  params / w0 / F: name -> tensor (F None: L2-SP)."""
    tot = 0.0
    for k, p in params.items():
        d = p - w0[k]
        tot = tot + ((d * d) if F is None else (F[k] * d * d)).sum()
    return 0.5 * lam * tot


def closed_form_grad(params, w0, F, lam):
    """lam * F * (w - w0), name -> tensor."""
    return {k: lam * (p.detach() - w0[k]) * (1.0 if F is None else F[k]) for k, p in params.items()}


class AnchorOnOracle:
    """mode None: the plain step.  step(micro_batches) returns (mean loss without the penalty, the penalty at the weights the step started from)."""

    def __init__(self, ref, mode, lam=LAM, w0=None, F=None, lr=1e-3, total_steps=20, warmup_steps=0, max_grad_norm=1.0):
        self.ref, self.mode, self.lam, self.w0, self.F, self.max_grad_norm = ref, mode, lam, w0, (F if mode == "ewc" else None), max_grad_norm
        self.named = dict(ref.named_parameters())
        self.opt = torch.optim.Adam(ref.parameters(), lr=lr)
        self.sch = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda k: R.cosine_with_warmup_lambda(k, warmup_steps, total_steps))
        self.lf = LossFnRef(R.DDPMSchedulerRef(), SDE_VP, psi=1)

    def step(self, micro_batches):
        self.opt.zero_grad()
        loss = sum(self.lf.p_loss(self.ref, x0, Rr, t, noise=eps) for x0, Rr, t, eps in micro_batches) / len(micro_batches)
        pen = None
        if self.mode is not None:
            pen = penalty(self.named, self.w0, self.F, self.lam)
            (loss + pen).backward()
        else:
            loss.backward()
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.ref.parameters(), self.max_grad_norm)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad()
        return float(loss.detach()), (None if pen is None else float(pen.detach()))


# ---- the kernels' numpy float32 op sequences ----------------------------------------------------------------------------------------------------
f32 = np.float32


def fisher_accum_ref(F, gr, s):
    """q = g * g; F = F + s * q."""
    q = gr * gr
    return F + f32(s) * q


def anchor_grad_ref(gr, w, w0, F, coef):
    """d = w - w0; t = F * d (F None: d); g = g + coef * t.  -> (g, t, d)"""
    d = w - w0
    t = d if F is None else F * d
    return gr + f32(coef) * t, t, d


def pen_chain(n, grid, block):
    """vd_anchor_grad's penalty sum: ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18 (include/villan_hip.h)."""
    items = (n + 3) // 4
    return -(-items // (grid * block)) + -(-grid // 256) + 18


# ---- the trajectory cases, computed once and shared read-only -----------------------------------------------------------------------------------
_SETUP, _ORACLE = {}, {}


def setup():
    """The start of the trajectory tests (the small UNet at seed 3) with its w0 and F: flat host tensors, the layout, and name -> tensor views."""
    if not _SETUP:
        from villandiffusion_amd.unet import UNet2DModel
        twin = UNet2DModel(**SMALL, device="cpu")
        twin.reset_parameters(seed=3)
        flat = twin.flat_param.detach().clone()
        w0, F = anchor_of(flat), fisher_of(flat.numel())
        inside = torch.zeros(flat.numel(), dtype=torch.bool)   # the alignment gaps of the flat layout belong to no parameter: w0 = w and F = 0 there
        for off, n, _ in twin._offs.values():
            inside[off:off + n] = True
        w0[~inside] = flat[~inside]
        F[~inside] = 0.0
        _SETUP.update(offs=dict(twin._offs), flat=flat, w0=w0, F=F, start={k: v.clone() for k, v in named(flat, twin._offs).items()})
    return _SETUP


def oracle_run(mode, accum=1, steps=4):
    """`steps` optimiser steps of AnchorOnOracle from `setup()`; step i takes the micro-batches batch_of(i * accum) ... -> losses, penalties, end."""
    key = (mode, accum, steps)
    if key not in _ORACLE:
        from oracle.unet_ref import UNet2DModelRef
        s = setup()
        ref = UNet2DModelRef(**SMALL)
        ref.load_state_dict(s["start"])
        o = AnchorOnOracle(ref, mode, LAM, named(s["w0"], s["offs"]), named(s["F"], s["offs"]))
        out = [o.step([batch_of(i * accum + j) for j in range(accum)]) for i in range(steps)]
        _ORACLE[key] = dict(losses=[a for a, _ in out], penalties=[b for _, b in out], end={k: v.detach().clone() for k, v in ref.named_parameters()})
    return _ORACLE[key]
