"""Trigger inversion for backdoored diffusion models: the distribution-shift objective of Elijah (An et al., AAAI 2024) on the HIP path.

    tau* = argmin_tau || mean_b model(eps_b + tau, T) - lam * tau ||_2

A clean model maps a shifted input to a shifted output only through `lam`; a backdoored one (BadDiffusion, TrojDiff, VillanDiffusion)
preserves the shift, so the minimiser recovers (a multiple of) its trigger.  One iteration is the network's no-weight-gradient backward
(`UNet2DModel`'s input-gradient pass: frozen weights, dL/dsample only), one fused objective launch (`vd_trigger_inv_objective`), one column sum
over the batch and the project's Adam kernel on `tau`.  Nothing here syncs with the host inside the loop.

VP-type `UNet2DModel`s only (the latent UNet of the LDM configuration included: it is inverted in latent space, no VAE involved).  What the
inverted trigger is then used for -- Elijah's uniformity / total-variation features and the data-free removal fine-tune -- is in `mitigation`.
The same for the score network of SDE-VE (`NCSNppModel` with `ScoreSdeVeScheduler`) is `defense_ve`, a module of its own.
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


@contextlib.contextmanager
def _frozen(model):
    """Every parameter's requires_grad off for the duration; the flags come back on exit, also after an exception."""
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)


def _objective_into(model, tau, eps, t, lam, loss, dtau, partial):
    """One evaluation with caller-owned outputs: loss ([1] view) and dtau ([C, H, W]) are written in place.  The model must be frozen."""
    B = eps.shape[0]
    x = eps.clone()
    ops.add_strided(x, tau.unsqueeze(0).expand_as(x), accumulate=True)          # x[b] = eps[b] + tau
    x.requires_grad_(True)
    with torch.enable_grad():
        e = model(x, t)[0]
    if e.grad_fn is None:
        raise RuntimeError("trigger inversion: the model did not take its input-gradient pass (are its parameters frozen?)")
    dout = torch.empty_like(e)
    ops.trigger_inv_objective(e.detach(), tau, lam, loss, dout, dtau, partial)  # loss, dL/de (every image), the direct term of dL/dtau
    dx, = torch.autograd.grad(e, x, dout)
    chw = tau.numel()
    ops.colsum(dx.view(B, chw), dtau, B, chw, accumulate=True)                   # dtau = direct term + sum_b dL/dx[b]
    return loss, dtau


def inversion_objective(model, tau: torch.Tensor, eps: torch.Tensor, t, lam: float = 0.5):
    """(loss, dtau) of L(tau) = || mean_b model(eps[b] + tau, t) - lam * tau ||_2 at frozen weights: loss a [1] device tensor, dtau like tau.
    For tests and for callers with an optimiser of their own; the parameters' requires_grad flags are restored on exit."""
    _check_model(model)
    if eps.dim() != 4 or tuple(tau.shape) != tuple(eps.shape[1:]):
        raise ValueError(f"inversion_objective: eps must be [B, C, H, W] and tau [C, H, W] (got {tuple(eps.shape)}, {tuple(tau.shape)})")
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


def invert_trigger(model, noise_sched, *, steps: int, batch: int, lam: float = 0.5, lr: float = 0.1, seed: int = 0, timestep: Optional[int] = None,
                   init: Optional[torch.Tensor] = None,
                   noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None) -> TriggerInversion:
    """Minimise the distribution-shift objective over the trigger `tau` with Adam(lr).

    timestep: defaults to the scheduler's last training timestep.  noise: None -- fresh per iteration from the device Philox stream (seed, disjoint
    counter ranges per iteration and image); a [steps, batch, C, H, W] tensor or a callable iteration -> [batch, C, H, W] makes a run reproducible
    against another implementation.  init: the starting trigger (default U[0, 1) from `seed`)."""
    # ---- everything that can be checked without the device ----
    if not isinstance(steps, int) or isinstance(steps, bool) or steps < 1:
        raise ValueError(f"invert_trigger: steps must be a positive int, got {steps!r}")
    if not isinstance(batch, int) or isinstance(batch, bool) or batch < 1:
        raise ValueError(f"invert_trigger: batch must be a positive int, got {batch!r}")
    lam, lr = float(lam), float(lr)
    if not (lam == lam and abs(lam) != float("inf")):
        raise ValueError(f"invert_trigger: lam must be finite, got {lam!r}")
    if not (lr > 0.0 and lr != float("inf")):
        raise ValueError(f"invert_trigger: lr must be positive and finite, got {lr!r}")
    _check_model(model, noise_sched)
    T_train = int(noise_sched.config.num_train_timesteps)
    T = T_train - 1 if timestep is None else int(timestep)
    if not 0 <= T < T_train:
        raise ValueError(f"invert_trigger: timestep {T} outside the scheduler's [0, {T_train})")
    S = int(model.sample_size)
    shape = (int(model.in_channels), S, S)
    if int(model.out_channels) != shape[0]:
        raise ValueError(f"invert_trigger: the objective compares the model's output with its input: out_channels {model.out_channels} != "
                         f"in_channels {model.in_channels}")
    if torch.is_tensor(noise) and tuple(noise.shape) != (steps, batch) + shape:
        raise ValueError(f"invert_trigger: noise must be [steps, batch, C, H, W] = {(steps, batch) + shape}, got {tuple(noise.shape)}")
    if noise is not None and not torch.is_tensor(noise) and not callable(noise):
        raise TypeError("invert_trigger: noise is None, a tensor or a callable iteration -> [batch, C, H, W]")
    if init is not None and tuple(init.shape) != shape:
        raise ValueError(f"invert_trigger: init must be {shape}, got {tuple(init.shape)}")

    # ---- device state ----
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
    t = torch.full((batch,), T, device=dev, dtype=torch.int64)
    eps_buf = torch.empty((batch,) + shape, device=dev, dtype=torch.float32)
    per_iter = (eps_buf.numel() + 3) // 4                  # Philox counters one iteration's noise consumes (four normals each)
    with _frozen(model):
        for it in range(steps):
            if noise is None:
                ops.randn(eps_buf, int(seed), (it + 1) * per_iter)
                eps = eps_buf
            else:
                eps = noise[it] if torch.is_tensor(noise) else noise(it)
                if tuple(eps.shape) != (batch,) + shape:
                    raise ValueError(f"invert_trigger: noise({it}) must be {(batch,) + shape}, got {tuple(eps.shape)}")
                eps = eps.detach().to(dev, torch.float32).contiguous()
            _objective_into(model, tau, eps, t, lam, losses[it:it + 1], dtau, partial)
            adam_update(tau, dtau, m, v, it + 1, lr)
    host = [float(x) for x in losses.cpu().tolist()]        # the one read of the loop's results
    return TriggerInversion(trigger=tau, losses=host, lam=lam, lr=lr, steps=steps, batch=batch, timestep=T, seed=int(seed))
