"""What to do with an inverted trigger (villandiffusion_amd.defense): the other two thirds of Elijah (An et al., AAAI 2024) on the HIP path.

* Detection features.  Sample a set of images from x_T = eps + tau and the paired set from x_T = eps.  A backdoored model collapses the shifted
  set onto its target: the images become alike (low uniformity = mean pairwise squared distance) and, for most targets, smooth (low total
  variation).  `image_set_stats` computes both in two launches over the final sampler states (`vd_image_set_stats`: the mean image first, then
  deviations and TV; the pairwise mean is 2/(N-1) * sum_i ||y_i - mean||^2, never an N^2 walk and never the one-pass form that cancels on exactly
  the collapsed sets detection is for).  `backdoor_features` samples both sets through the pipeline's chunked entry and returns the ratios.
  Elijah trains a classifier over many models on these features; this project has no such model zoo and therefore no default threshold.

* Removal.  Fine-tune on pure noise so that a shifted input no longer gives a shifted output, with a frozen copy of the same model as teacher:

      L = w_clean * mse(model(eps), frozen(eps)) + w_shift * mse(model(eps + tau), frozen(eps))

  No data and no true trigger are needed.  One step is the frozen model's no-grad forward at B (the sampler's captured forward), the model's
  training forward and backward at 2B, one `vd_removal_loss` launch pair (loss terms and dL/dpred in one read of pred) and the project's clip +
  Adam.  Nothing syncs with the host inside the loop.

Pixel-space VP-type `UNet2DModel`s, single process.  (`NCSNppModel` / SDE-VE: `defense_ve`, which imports from here what the two families
share: `_check_feature_args`, `_features`, `_check_removal_args`, `_removal_step` and the removal loop `_run_removal`.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import torch

from . import ops
from .defense import (_check_count, _check_loop_args, _check_model, _check_pair, _check_trigger, _frozen, _noise_of, _shape, _trainable,
                      _vp_timestep)

__all__ = ["ImageSetStats", "image_set_stats", "BackdoorFeatures", "backdoor_features", "removal_objective", "BackdoorRemoval", "remove_backdoor"]


# ------------------------------------------------------------------------------------------------------------------------ detection features
@dataclass
class ImageSetStats:
    n: int
    uniformity: float                      # mean over pairs i < j of ||y_i - y_j||^2
    tv: float                              # mean over images of the anisotropic total variation
    mean_image: torch.Tensor               # [C, H, W] on the set's device: the mean post-processed image (a collapsed set's target)

    def as_dict(self) -> dict:
        return {"n": self.n, "uniformity": self.uniformity, "tv": self.tv}


def image_set_stats(x: torch.Tensor, *, postprocess: bool = True) -> ImageSetStats:
    """Uniformity and total variation of an [N, C, H, W] device tensor of final sampler states.  postprocess: measure the images the pipelines
    return, clamp(x/2 + 1/2, 0, 1) (pipelines._post); False: x as it is.  One host read (two floats)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"image_set_stats: x must be an [N, C, H, W] tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    N, Cc, H, W = (int(s) for s in x.shape)
    if N < 2:
        raise ValueError(f"image_set_stats: a pairwise statistic needs N >= 2 images, got {N}")
    from . import lib
    lib.require_device()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride()[1:] != (H * W, W, 1):
        x = x.contiguous()
    mean = torch.empty((Cc, H, W), device=x.device, dtype=torch.float32)
    stats = torch.empty(2, device=x.device, dtype=torch.float32)
    partial = torch.empty(2048, device=x.device, dtype=torch.float32)
    mul, add, lo, hi = (0.5, 0.5, 0.0, 1.0) if postprocess else (1.0, 0.0, float("-inf"), float("inf"))
    ops.image_set_stats(x, mean, stats, partial, mul, add, lo, hi)
    dev_sq, tv_sum = stats.cpu().tolist()                   # the one host read
    return ImageSetStats(n=N, uniformity=2.0 / (N - 1) * dev_sq, tv=tv_sum / N, mean_image=mean)


@dataclass
class BackdoorFeatures:
    clean: ImageSetStats                   # the set sampled from eps
    shifted: ImageSetStats                 # the set sampled from eps + trigger (the same eps)
    uniformity_ratio: float                # shifted / clean
    tv_ratio: float
    n: int
    batch: int
    num_inference_steps: int
    seed: int
    sigma: Optional[float] = None          # SDE-VE (`defense_ve`) only: the noise level the sets start from

    def verdict(self, threshold: float) -> bool:
        """True (backdoored) when the shifted set is more than 1/threshold times as alike as the clean one.  The threshold is the caller's:
        it depends on the sampler, the step count and the model family, and nothing here has been calibrated."""
        return self.uniformity_ratio < float(threshold)

    def as_dict(self) -> dict:
        return {"clean": self.clean.as_dict(), "shifted": self.shifted.as_dict(), "uniformity_ratio": self.uniformity_ratio,
                "tv_ratio": self.tv_ratio, "n": self.n, "batch": self.batch, "num_inference_steps": self.num_inference_steps, "seed": self.seed}


def _check_pipeline(pipeline):
    from .pipelines import DiffusionPipeline
    from .unet import UNet2DModel
    name = type(pipeline).__name__
    if not isinstance(pipeline, DiffusionPipeline):
        raise TypeError(f"backdoor_features needs a villandiffusion_amd pipeline, got {name}")
    if type(pipeline).__call__ is not DiffusionPipeline.__call__ or getattr(pipeline, "vqvae", None) is not None:
        raise NotImplementedError(f"backdoor_features: {name} is out of scope (latent and VE pipelines have sampling loops of their own); "
                                  f"pixel-space UNet2DModel pipelines only")
    if not isinstance(pipeline.unet, UNet2DModel) or not getattr(pipeline.unet, "_input_grad", False):
        raise NotImplementedError(f"backdoor_features: {name} with a {type(pipeline.unet).__name__} is out of scope; pixel-space UNet2DModel "
                                  f"pipelines only")


def _check_feature_args(what, pipeline, trigger, n, batch, num_inference_steps) -> int:
    """The checks both `backdoor_features` share, after the family's own check of the pipeline.  -> the resolved step count"""
    _check_count(what, "n", n)
    _check_count(what, "batch", batch)
    if n < 2:
        raise ValueError(f"{what}: a pairwise statistic needs n >= 2 images, got {n}")
    _check_trigger(what, trigger, _shape(pipeline.unet))
    steps = int(num_inference_steps) if num_inference_steps is not None else int(pipeline.default_steps)
    if steps < 1:
        raise ValueError(f"{what}: num_inference_steps must be positive, got {steps}")
    return steps


def _features(clean: ImageSetStats, shifted: ImageSetStats, n, batch, steps, seed, sigma=None) -> BackdoorFeatures:
    return BackdoorFeatures(clean=clean, shifted=shifted, uniformity_ratio=_ratio(shifted.uniformity, clean.uniformity),
                            tv_ratio=_ratio(shifted.tv, clean.tv), n=n, batch=batch, num_inference_steps=steps, seed=int(seed), sigma=sigma)


def _feature_inits(pipeline, n: int, batch: int, seed: int) -> List[torch.Tensor]:
    """The n noise images of `backdoor_features` as chunks of at most `batch`: chunk k is drawn from the device Philox stream of `seed` at
    counter offset k * ceil(batch*C*H*W / 4), so the chunks are disjoint and a chunk does not depend on n."""
    shape = _shape(pipeline.unet)
    per_chunk = (batch * shape[0] * shape[1] * shape[2] + 3) // 4
    out = []
    for k, first in enumerate(range(0, n, batch)):
        c = torch.empty((min(batch, n - first),) + shape, device=pipeline.device, dtype=torch.float32)
        out.append(ops.randn(c, int(seed), k * per_chunk))
    return out


def _sample_set(pipeline, inits, n_steps):
    """Final states of the chunks through the pipeline's chunked entry: concurrent chunks where the measure loop would use them."""
    from .sampling_io import _concurrent_ok, sampler_streams
    if _concurrent_ok(pipeline, [(c, len(c)) for c in inits], None):
        outs = pipeline.sample_concurrent(list(inits), num_inference_steps=n_steps, n_streams=sampler_streams())
    else:
        outs = pipeline.sample_sequential(list(inits), num_inference_steps=n_steps)
    return torch.cat(outs)


def backdoor_features(pipeline, trigger: torch.Tensor, *, n: int, batch: int, num_inference_steps: Optional[int] = None,
                      seed: int = 0) -> BackdoorFeatures:
    """Sample n images from eps and n from eps + trigger (the same eps, in chunks of `batch`; the last may be short) and compare the two sets.
    The inits come from the Philox stream of `seed`; a scheduler that draws its step noise on the device and has no `device_rng_seed` gets
    `seed + 1` for the call, so the two never share counters.  Both sets are sampled from the same scheduler offset: they differ in the trigger
    alone."""
    _check_pipeline(pipeline)
    steps = _check_feature_args("backdoor_features", pipeline, trigger, n, batch, num_inference_steps)
    sch = pipeline.scheduler

    from . import lib
    lib.require_device()
    dev = pipeline.device
    tau = trigger.detach().to(dev, torch.float32).contiguous()
    own_seed = hasattr(sch, "device_rng_seed") and sch.device_rng_seed is None
    off0 = getattr(sch, "_rng_offset", None)
    if own_seed:
        sch.device_rng_seed = int(seed) + 1
    try:
        inits = _feature_inits(pipeline, n, batch, seed)
        clean = image_set_stats(_sample_set(pipeline, inits, steps))
        if off0 is not None:
            sch._rng_offset = off0                        # the shifted set draws the step noise the clean one drew
        for c in inits:
            ops.add_strided(c, tau.unsqueeze(0).expand_as(c), accumulate=True)     # eps + tau, in place: the same eps
        shifted = image_set_stats(_sample_set(pipeline, inits, steps))
    finally:
        if own_seed:
            sch.device_rng_seed = None
            if off0 is not None:
                sch._rng_offset = off0
    return _features(clean, shifted, n, batch, steps, seed)


def _ratio(a: float, b: float) -> float:
    return a / b if b != 0.0 else (float("nan") if a == 0.0 else float("inf"))


# ------------------------------------------------------------------------------------------------------------------------------------ removal
@dataclass
class BackdoorRemoval:
    total: List[float]                     # per step, at the START of the step: w_clean*clean + w_shift*shift
    clean: List[float]                     # mse(model(eps), frozen(eps))
    shift: List[float]                     # mse(model(eps + tau), frozen(eps))
    frozen: object                         # the teacher: the model's state at entry, untouched
    lr: float
    steps: int
    batch: int
    w_clean: float
    w_shift: float
    max_grad_norm: Optional[float]
    timestep: int
    seed: int
    sigma: Optional[float] = None          # SDE-VE (`defense_ve`) only: the noise level of the fine-tune
    anchor_penalty: Optional[List[float]] = None      # with anchor_lambda only: per step, at its START, lambda / 2 * sum F (w - w0)^2 (0 at step one)
    anchor_lambda: Optional[float] = None


def _frozen_copy(model):
    """A second network with the model's configuration, arithmetic and current weights, every parameter frozen."""
    twin = type(model)(**vars(model.config), device=model.device)
    for attr in ("conv_math", "fused_attention", "sampler_graph"):
        if hasattr(model, attr):
            setattr(twin, attr, getattr(model, attr))
    with torch.no_grad():
        twin.flat_param.copy_(model.flat_param)
    twin.weights_changed()
    for p in twin.parameters():
        p.requires_grad_(False)
    return twin


def _removal_into(model, teacher, tau, eps, t2, w_clean, w_shift, terms, partial):
    """One evaluation with a caller-owned `terms` ([3] view): the gradient of terms[0] is ADDED to model.flat_grad (as loss.backward() does).
    teacher: x, t -> the frozen model's output (pipelines.sampler_forward of the frozen copy)."""
    B = eps.shape[0]
    x = torch.empty((2 * B,) + tuple(eps.shape[1:]), device=eps.device, dtype=torch.float32)
    x[:B].copy_(eps)
    x[B:].copy_(eps)
    ops.add_strided(x[B:], tau.unsqueeze(0).expand_as(eps), accumulate=True)           # x = [eps; eps + tau]
    with torch.no_grad():
        ref = teacher(eps, t2[:B])
    with torch.enable_grad():
        pred = model(x, t2)[0]
    if pred.grad_fn is None:
        raise RuntimeError("backdoor removal: the model did not take its training forward (are all of its parameters frozen?)")
    dpred = torch.empty_like(pred)
    ops.removal_loss(pred.detach(), ref, w_clean, w_shift, dpred, terms, partial)
    pred.backward(dpred)
    return terms


def _removal_step(model, teacher, opt, tau, eps, t2, w_clean, w_shift, terms, partial, anchor=None):
    """One step of `remove_backdoor`'s loop: the evaluation into `terms`, clip + Adam, the gradient reset.  anchor: None, or (w0, F or None,
    lambda, a 1024-float scratch, the device word of this step's unscaled penalty) -- one launch adds lambda * F * (w - w0) to the gradient before
    the clip (anchor.py)."""
    _removal_into(model, teacher, tau, eps, t2, w_clean, w_shift, terms, partial)
    if anchor is not None:
        w0, F, lam, scratch, pen = anchor
        ops.anchor_grad(model.flat_grad, model.flat_param, w0, F, lam, scratch, pen)
    opt.step()
    model.zero_grad()


def _check_removal_args(what, w_clean, w_shift, max_grad_norm):
    for name, w in (("w_clean", w_clean), ("w_shift", w_shift)):
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError(f"{what}: {name} must be finite and non-negative, got {w!r}")
    if max_grad_norm is not None and not (float(max_grad_norm) > 0.0 and math.isfinite(float(max_grad_norm))):
        raise ValueError(f"{what}: max_grad_norm must be positive and finite (or None: no clipping), got {max_grad_norm!r}")


def _check_f16(what, model):
    if getattr(model, "conv_math", None) == "f16":
        raise NotImplementedError(f"{what}: conv_math 'f16' needs loss scaling, which the removal loop does not have; use 'bf16x3', 'f32' or 'bf16'")


def _anchor_args(what, model, anchor_lambda, fisher):
    """The AnchorConfig of a removal loop's anchor_lambda / fisher (None, None: no anchor); every refusal before the device is touched."""
    if anchor_lambda is None:
        if fisher is not None:
            raise ValueError(f"{what}: fisher needs anchor_lambda")
        return None
    from .anchor import AnchorConfig
    cfg = AnchorConfig(lam=anchor_lambda, mode="l2sp" if fisher is None else "ewc", fisher=fisher)
    if fisher is not None and fisher.numel() != model.flat_numel:
        raise ValueError(f"{what}: the Fisher holds {fisher.numel()} entries; the model's flat_param has {model.flat_numel} floats")
    return cfg


def _run_removal(what, model, make_teacher, trigger, shape, t, w_clean, w_shift, lr, max_grad_norm, steps, batch, seed, noise,
                 prepare=lambda x: x, skip=(), anchor_lambda=None, fisher=None):
    """The removal loop of both families: `steps` iterations of clip + FusedAdam(lr) on `model`, in place, at the noise level `t`, against a
    frozen copy of its state at entry.  make_teacher: frozen copy -> (x, t -> its output), called once before the loop with the model's
    parameters already trainable.  prepare: what turns the trigger and each iteration's unit noise into network input units (SDE-VE scales by
    sigma).  skip: parameters that are never unfrozen.  -> (the frozen copy, the [total, clean, shift] rows of every step, on the host)
    anchor_lambda (with fisher: EWC, else L2-SP): every step's gradient gains lambda * F * (w - w0), w0 the frozen copy's flat_param, and a third
    value is returned: the penalty lambda / 2 * sum F (w - w0)^2 at the start of every step.  At the defaults nothing changes."""
    acfg = _anchor_args(what, model, anchor_lambda, fisher)
    from . import lib
    from .trainer import FusedAdam
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = model.device
    tau = prepare(trigger.detach().to(dev, torch.float32).contiguous())
    frozen = _frozen_copy(model)
    opt = FusedAdam(model, lr, max_grad_norm=None if max_grad_norm is None else float(max_grad_norm))
    curves = torch.zeros((steps, 3), device=dev, dtype=torch.float32)
    partial = torch.empty(2048, device=dev, dtype=torch.float32)
    t2 = torch.full((2 * batch,), float(t), device=dev, dtype=torch.float32)
    eps_buf = torch.empty((batch,) + shape, device=dev, dtype=torch.float32)
    per_iter = (eps_buf.numel() + 3) // 4                  # Philox counters one iteration's noise consumes (four normals each)
    pens = anchor_of = None
    if acfg is not None:
        pens = torch.zeros(steps, device=dev, dtype=torch.float32)
        F = None if acfg.fisher is None else acfg.fisher.detach().to(dev, torch.float32).contiguous()
        scratch = torch.empty(1024, device=dev, dtype=torch.float32)
        anchor_of = lambda it: (frozen.flat_param, F, float(acfg.lam), scratch, pens[it:it + 1])
    with _trainable(model, skip):                          # the fine-tune trains every parameter (but `skip`); the caller's flags come back on exit
        teacher = make_teacher(frozen)                     # before the loop: a captured forward synchronises
        model.zero_grad()
        for it in range(steps):
            eps = prepare(_noise_of(what, noise, it, eps_buf, seed, per_iter, dev))
            _removal_step(model, teacher, opt, tau, eps, t2, w_clean, w_shift, curves[it], partial,
                          **({} if anchor_of is None else {"anchor": anchor_of(it)}))
    if pens is not None:
        return frozen, curves.cpu().tolist(), [0.5 * float(acfg.lam) * v for v in pens.cpu().tolist()]
    return frozen, curves.cpu().tolist()                   # the one read of the loop's results


def _timesteps(t, B2, dev):
    if torch.is_tensor(t):
        t = t.to(dev).reshape(-1)
        if t.numel() == 1:
            return t.to(torch.float32).expand(B2).contiguous()
        if t.numel() == B2 // 2:
            return torch.cat([t, t]).to(torch.float32)                # the same timestep for an image and its shifted twin
        raise ValueError(f"removal_objective: t must hold 1 or B timesteps, got {t.numel()} for B = {B2 // 2}")
    return torch.full((B2,), float(t), device=dev, dtype=torch.float32)


def removal_objective(model, frozen, tau: torch.Tensor, eps: torch.Tensor, t, w_clean: float = 1.0, w_shift: float = 1.0) -> torch.Tensor:
    """terms = [w_clean*clean + w_shift*shift, clean, shift] (a [3] device tensor) of the removal loss at `model`'s current weights, `frozen` the
    teacher; the gradient of terms[0] with respect to the parameters is accumulated into `model.flat_grad` (call `model.zero_grad()` first for the
    gradient of this evaluation alone).  For tests and for callers with an optimiser of their own."""
    _check_model(model)
    _check_model(frozen)
    _check_pair("removal_objective", tau, eps)
    _check_f16("removal_objective", model)
    from . import lib
    from .pipelines import sampler_forward
    lib.require_device()
    dev = model.device
    tau = tau.detach().to(dev, torch.float32).contiguous()
    eps = eps.detach().to(dev, torch.float32).contiguous()
    B = eps.shape[0]
    t2 = _timesteps(t, 2 * B, dev)
    terms = torch.empty(3, device=dev, dtype=torch.float32)
    partial = torch.empty(2048, device=dev, dtype=torch.float32)
    with _frozen(frozen):
        teacher = sampler_forward(frozen, B)
        _removal_into(model, teacher, tau, eps, t2, float(w_clean), float(w_shift), terms, partial)
    return terms


def remove_backdoor(model, noise_sched, trigger: torch.Tensor, *, steps: int, batch: int, lr: float, w_clean: float = 1.0, w_shift: float = 1.0,
                    max_grad_norm: Optional[float] = 1.0, seed: int = 0, timestep: Optional[int] = None,
                    noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None, anchor_lambda: Optional[float] = None,
                    fisher: Optional[torch.Tensor] = None) -> BackdoorRemoval:
    """Fine-tune `model` IN PLACE for `steps` Adam(lr, constant) iterations of the removal loss on `batch` noise images each, against a frozen copy
    of its state at entry (returned as `.frozen`, never written).  anchor_lambda: the weights are held to that state by the L2-SP penalty, or with
    `fisher` (a flat Fisher, anchor.estimate_fisher) the EWC penalty; the record gains `anchor_penalty`, its value at the start of every step.

    timestep: defaults to the scheduler's last training timestep.  noise: None -- fresh per iteration from the device Philox stream (seed, disjoint
    counter ranges per iteration); a [steps, batch, C, H, W] tensor or a callable iteration -> [batch, C, H, W] makes a run reproducible against
    another implementation.  The three loss terms of every step stay on the device until the loop is over."""
    # everything that can be checked is checked before the device is touched (in _run_removal)
    lr, w_clean, w_shift = float(lr), float(w_clean), float(w_shift)
    _check_removal_args("remove_backdoor", w_clean, w_shift, max_grad_norm)
    _check_model(model, noise_sched)
    _check_f16("remove_backdoor", model)
    shape = _shape(model)
    _check_loop_args("remove_backdoor", model, steps, batch, lr, noise, shape)
    T = _vp_timestep("remove_backdoor", noise_sched, timestep)
    _check_trigger("remove_backdoor", trigger, shape)
    from .pipelines import sampler_forward
    _anchor_args("remove_backdoor", model, anchor_lambda, fisher)
    akw = {} if anchor_lambda is None else dict(anchor_lambda=anchor_lambda, fisher=fisher)
    frozen, host, *pen = _run_removal("remove_backdoor", model, lambda twin: sampler_forward(twin, batch), trigger, shape, T, w_clean, w_shift, lr,
                                      max_grad_norm, steps, batch, seed, noise, **akw)
    return BackdoorRemoval(total=[r[0] for r in host], clean=[r[1] for r in host], shift=[r[2] for r in host], frozen=frozen, lr=lr, steps=steps,
                           batch=batch, w_clean=w_clean, w_shift=w_shift, max_grad_norm=max_grad_norm, timestep=T, seed=int(seed),
                           **({} if not pen else dict(anchor_penalty=pen[0], anchor_lambda=float(anchor_lambda))))
