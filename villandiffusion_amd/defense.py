"""Trigger inversion for backdoored diffusion models: the distribution-shift objective of Elijah (An et al., AAAI 2024) on the HIP path.

    tau* = argmin_tau || mean_b model(eps_b + tau, T) - lam * tau ||_2

A clean model maps a shifted input to a shifted output only through `lam`; a backdoored one (BadDiffusion, TrojDiff, VillanDiffusion)
preserves the shift, so the minimiser recovers (a multiple of) its trigger.  One iteration is the network's no-weight-gradient backward
(`UNet2DModel`'s input-gradient pass: frozen weights, dL/dsample only), one fused objective launch (`vd_trigger_inv_objective`), one column sum
over the batch and the project's Adam kernel on `tau`.  Nothing here syncs with the host inside the loop.

VP-type `UNet2DModel`s only (the latent UNet of the LDM configuration included: it is inverted in latent space, no VAE involved).  What the
inverted trigger is then used for -- Elijah's uniformity / total-variation features and the data-free removal fine-tune -- is in `mitigation`.
The same for the score network of SDE-VE (`NCSNppModel` with `ScoreSdeVeScheduler`) is `defense_ve`, a module of its own.

This is the lowest of the three modules (`defense` <- `mitigation` <- `defense_ve`), so what they share lives here, once: the argument checks
(`_check_count`, `_check_loop_args`, `_check_pair`, `_check_trigger`), the per-iteration noise (`_noise_of`), the `requires_grad` contexts
(`_frozen`, `_trainable`), the objective's launch sequence (`_objective_into`, which takes SDE-VE's sigma) and the inversion loop
(`_run_inversion`).  The A/B tools under tools/ time these very functions.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Union

import torch

from . import ops

__all__ = ["TriggerInversion", "inversion_objective", "invert_trigger"]


@dataclass
class TriggerInversion:
    trigger: torch.Tensor                  # [C, H, W] on the model's device
    losses: List[float]                    # the objective at the START of every iteration (read from the device once, after the loop)
    lam: float
    lr: float
    steps: int
    batch: int
    timestep: int
    seed: int
    extra: dict = field(default_factory=dict)

    @property
    def trigger_norm(self) -> float:
        return float(torch.linalg.vector_norm(self.trigger.double()).item())


def _check_model(model, noise_sched=None):
    """NotImplementedError for what the objective is not defined / built for, saying which."""
    from .unet import UNet2DModel
    if not isinstance(model, UNet2DModel):
        raise TypeError(f"trigger inversion needs a villandiffusion_amd UNet2DModel, got {type(model).__name__}")
    if not getattr(model, "_input_grad", False):
        raise NotImplementedError(f"trigger inversion: {type(model).__name__} has no input-gradient pass (NCSN++ / score-SDE models are out of scope; "
                                  f"VP-type UNet2DModel only)")
    if noise_sched is not None:
        from .schedulers import KarrasVeScheduler, ScoreSdeVeScheduler
        if isinstance(noise_sched, (ScoreSdeVeScheduler, KarrasVeScheduler)) or not hasattr(noise_sched, "alphas_cumprod"):
            raise NotImplementedError(f"trigger inversion: {type(noise_sched).__name__} is a VE-type scheduler; the distribution-shift objective is "
                                      f"built for VP-type (DDPM-style) noise schedules only")


def _shape(model):
    S = int(model.sample_size)
    return (int(model.in_channels), S, S)


def _check_count(what, name, v):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f"{what}: {name} must be a positive int, got {v!r}")


def _check_loop_args(what, model, steps, batch, lr, noise, shape):
    _check_count(what, "steps", steps)
    _check_count(what, "batch", batch)
    if not (lr > 0.0 and lr != float("inf")):
        raise ValueError(f"{what}: lr must be positive and finite, got {lr!r}")
    if int(model.out_channels) != shape[0]:
        raise ValueError(f"{what}: the objective compares the model's output with its input: out_channels {model.out_channels} != in_channels "
                         f"{model.in_channels}")
    if torch.is_tensor(noise) and tuple(noise.shape) != (steps, batch) + shape:
        raise ValueError(f"{what}: noise must be [steps, batch, C, H, W] = {(steps, batch) + shape}, got {tuple(noise.shape)}")
    if noise is not None and not torch.is_tensor(noise) and not callable(noise):
        raise TypeError(f"{what}: noise is None, a tensor or a callable iteration -> [batch, C, H, W]")


def _check_pair(what, tau, eps):
    if eps.dim() != 4 or tuple(tau.shape) != tuple(eps.shape[1:]):
        raise ValueError(f"{what}: eps must be [B, C, H, W] and tau [C, H, W] (got {tuple(eps.shape)}, {tuple(tau.shape)})")


def _check_trigger(what, trigger, shape):
    if not torch.is_tensor(trigger) or tuple(trigger.shape) != shape:
        raise ValueError(f"{what}: trigger must be {shape}, got {tuple(trigger.shape) if torch.is_tensor(trigger) else type(trigger).__name__}")


def _noise_of(what, noise, it, eps_buf, seed, per_iter, dev):
    """Iteration `it`'s unit noise: the Philox draw at counter (it + 1) * per_iter into eps_buf, or the caller's tensor / callable."""
    if noise is None:
        return ops.randn(eps_buf, int(seed), (it + 1) * per_iter)
    eps = noise[it] if torch.is_tensor(noise) else noise(it)
    if tuple(eps.shape) != tuple(eps_buf.shape):
        raise ValueError(f"{what}: noise({it}) must be {tuple(eps_buf.shape)}, got {tuple(eps.shape)}")
    return eps.detach().to(dev, torch.float32).contiguous()


@contextlib.contextmanager
def _flags_set(model, value, skip=()):
    """Every parameter's requires_grad set to `value` for the duration, except those in `skip`; the caller's flags come back on exit, also
    after an exception."""
    flags = [(p, p.requires_grad) for p in model.parameters()]
    keep = {id(p) for p in skip}
    try:
        for p, _ in flags:
            if id(p) not in keep:
                p.requires_grad_(value)
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)


def _frozen(model):
    """Every parameter's requires_grad off for the duration; the flags come back on exit, also after an exception."""
    return _flags_set(model, False)


def _trainable(model, skip=()):
    """The mirror of `_frozen`: every parameter's requires_grad on for the duration, except those in `skip`, which stay as they are."""
    return _flags_set(model, True, skip)


def _objective_into(model, tau, eps, t, lam, loss, dtau, partial, sigma=None):
    """One evaluation with caller-owned outputs: loss ([1] view) and dtau ([C, H, W]) are written in place.  The model must be frozen.
    sigma=None: the VP objective at timesteps t.  A sigma: the SDE-VE one (`defense_ve`) -- the input is sigma * (eps + tau), t holds sigma, the
    model's input gradients must be switched on and the score is read as the noise prediction -sigma * s."""
    B = eps.shape[0]
    x = eps.clone()
    ops.add_strided(x, tau.unsqueeze(0).expand_as(x), accumulate=True)          # x[b] = eps[b] + tau
    if sigma is not None:
        ops.scale_(x, sigma)                                                    # x[b] = sigma * (eps[b] + tau)
    x.requires_grad_(True)
    with torch.enable_grad():
        e = model(x, t)[0]
    if e.grad_fn is None:
        raise RuntimeError("trigger inversion: the model did not take its input-gradient pass (are its parameters frozen?)")
    dout = torch.empty_like(e)
    if sigma is None:
        ops.trigger_inv_objective(e.detach(), tau, lam, loss, dout, dtau, partial)          # loss, dL/de (every image), the direct term of dL/dtau
    else:
        ops.score_inv_objective(e.detach(), tau, sigma, lam, loss, dout, dtau, partial)     # ... with sigma * dL/ds: dx/dtau = sigma is in dout
    dx, = torch.autograd.grad(e, x, dout)
    chw = tau.numel()
    ops.colsum(dx.view(B, chw), dtau, B, chw, accumulate=True)                   # dtau = direct term + sum_b dL/dx[b]
    return loss, dtau


def inversion_objective(model, tau: torch.Tensor, eps: torch.Tensor, t, lam: float = 0.5):
    """(loss, dtau) of L(tau) = || mean_b model(eps[b] + tau, t) - lam * tau ||_2 at frozen weights: loss a [1] device tensor, dtau like tau.
    For tests and for callers with an optimiser of their own; the parameters' requires_grad flags are restored on exit."""
    _check_model(model)
    _check_pair("inversion_objective", tau, eps)
    dev = model.device
    tau = tau.detach().to(dev, torch.float32).contiguous()
    eps = eps.detach().to(dev, torch.float32).contiguous()
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    dtau = torch.empty_like(tau)
    partial = torch.empty(1024, device=dev, dtype=torch.float32)
    with _frozen(model):
        _objective_into(model, tau, eps, t, float(lam), loss, dtau, partial)
    return loss, dtau


def adam_update(tau, dtau, m, v, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """torch.optim.Adam's update of `tau` in place (the project's one Adam kernel: no clip, no overflow skip; no weight cache is invalidated)."""
    ops.adam_step(tau, dtau, m, v, None, 0.0, 1.0, lr, beta1, beta2, eps, step, weights=False)
    return tau


def _check_inversion_args(what, model, steps, batch, lam, lr, noise, init):
    """The checks both `invert_trigger`s share, after the family's own check of the model.  -> (shape, lam, lr)"""
    lam, lr = float(lam), float(lr)
    if not (lam == lam and abs(lam) != float("inf")):
        raise ValueError(f"{what}: lam must be finite, got {lam!r}")
    shape = _shape(model)
    _check_loop_args(what, model, steps, batch, lr, noise, shape)
    if init is not None and tuple(init.shape) != shape:
        raise ValueError(f"{what}: init must be {shape}, got {tuple(init.shape)}")
    return shape, lam, lr


def _run_inversion(what, model, shape, t, lam, lr, steps, batch, seed, init, noise, sigma=None):
    """The inversion loop of both families: Adam(lr) on tau for `steps` iterations at the noise level `t` (a VP timestep; for SDE-VE the sigma,
    passed as `sigma` too).  The caller holds the model frozen (and, for SDE-VE, its input gradients on) around the call.
    -> (tau, the objective at the START of every iteration)"""
    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = model.device
    if init is not None:
        tau = init.detach().to(dev, torch.float32).contiguous().clone()
    else:
        tau = torch.rand(shape, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32).to(dev)
    m, v = torch.zeros_like(tau), torch.zeros_like(tau)
    dtau = torch.empty_like(tau)
    losses = torch.zeros(steps, device=dev, dtype=torch.float32)
    partial = torch.empty(1024, device=dev, dtype=torch.float32)
    t = torch.full((batch,), t, device=dev, dtype=torch.int64 if sigma is None else torch.float32)
    eps_buf = torch.empty((batch,) + shape, device=dev, dtype=torch.float32)
    per_iter = (eps_buf.numel() + 3) // 4                  # Philox counters one iteration's noise consumes (four normals each)
    for it in range(steps):
        eps = _noise_of(what, noise, it, eps_buf, seed, per_iter, dev)
        _objective_into(model, tau, eps, t, lam, losses[it:it + 1], dtau, partial, sigma)
        adam_update(tau, dtau, m, v, it + 1, lr)
    return tau, [float(x) for x in losses.cpu().tolist()]   # the one read of the loop's results


def _vp_timestep(what, noise_sched, timestep):
    T_train = int(noise_sched.config.num_train_timesteps)
    T = T_train - 1 if timestep is None else int(timestep)
    if not 0 <= T < T_train:
        raise ValueError(f"{what}: timestep {T} outside the scheduler's [0, {T_train})")
    return T


def invert_trigger(model, noise_sched, *, steps: int, batch: int, lam: float = 0.5, lr: float = 0.1, seed: int = 0, timestep: Optional[int] = None,
                   init: Optional[torch.Tensor] = None,
                   noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None) -> TriggerInversion:
    """Minimise the distribution-shift objective over the trigger `tau` with Adam(lr).

    timestep: defaults to the scheduler's last training timestep.  noise: None -- fresh per iteration from the device Philox stream (seed, disjoint
    counter ranges per iteration and image); a [steps, batch, C, H, W] tensor or a callable iteration -> [batch, C, H, W] makes a run reproducible
    against another implementation.  init: the starting trigger (default U[0, 1) from `seed`)."""
    # everything that can be checked is checked before the device is touched (in _run_inversion)
    _check_model(model, noise_sched)
    shape, lam, lr = _check_inversion_args("invert_trigger", model, steps, batch, lam, lr, noise, init)
    T = _vp_timestep("invert_trigger", noise_sched, timestep)
    with _frozen(model):
        tau, losses = _run_inversion("invert_trigger", model, shape, T, lam, lr, steps, batch, seed, init, noise)
    return TriggerInversion(trigger=tau, losses=losses, lam=lam, lr=lr, steps=steps, batch=batch, timestep=T, seed=int(seed))
