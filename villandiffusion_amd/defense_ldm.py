"""Trigger inversion, detection features and data-free removal (Elijah, An et al., AAAI 2024) for the latent-diffusion pipeline: `LDMPipeline`
with a `VQModel`, a VP-type latent `UNet2DModel` and a VP-type scheduler.  The same function names and result types as `defense` / `mitigation`
(pixel-space VP models) and `defense_ve` (NCSN++), which stay as they are; every function here takes the pipeline.

The LDM attack is a pixel-space attack: the trigger image is encoded with the VQ-VAE and the sampler starts from noise + encode(trigger).  So a
trigger lives in one of two spaces, told apart by its shape:

* latent `[C, h, w]` (the UNet's input shape): what is added to the noise.  `encode_trigger` maps a pixel trigger to it, `render_trigger`
  decodes one for looking at.
* pixel `[3, S, S]` (the VQ-VAE's input shape): what the attacker stamped.  `invert_trigger(space="pixel")` searches there, i.e. only over
  latent triggers a pixel image can produce (the encoder's range): each iteration encodes p at batch 1 inside `VQModel.input_gradients()`,
  evaluates the latent objective at tau = encode(p) (`defense._objective_into`: `vd_trigger_inv_objective` plus the UNet's input-gradient pass at
  `batch`), pulls dL/dz back through the encoder, takes one `vd_adam_step` on p and clamps p (`vd_postprocess`).  Nothing syncs with the host
  inside the loop.

Detection samples both sets through the latent loop `LDMPipeline.__call__` runs and measures them twice: the final latents as they are and the
decoded images as the pipeline returns them.  A decoded 256 x 256 set does not fit next to the decoder's activations, so a chunk is decoded,
measured (`vd_image_set_stats`), merged into a running result (`vd_image_set_merge`, the pairwise update of Chan et al.) and freed:
`ImageSetAccumulator`.  Removal fine-tunes the latent UNet alone (`mitigation.remove_backdoor` at the encoded trigger); the VQ-VAE is untouched.

No detection quality is claimed, and nothing about which space inverts better: no genuinely backdoored LDM checkpoint exists to calibrate
anything on.  Single process; the VQ-VAE runs in f32, the UNet in its own arithmetic.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Union

import torch

from . import defense, mitigation, ops
from .defense import (TriggerInversion, _check_count, _check_inversion_args, _check_loop_args, _check_pair, _frozen, _noise_of, _objective_into,
                      _shape, _vp_timestep, adam_update)
from .mitigation import (BackdoorFeatures, BackdoorRemoval, ImageSetStats, _check_f16, _check_removal_args, _feature_inits, _ratio)

__all__ = ["ImageSetAccumulator", "LDMBackdoorFeatures", "trigger_space", "encode_trigger", "render_trigger", "inversion_objective",
           "invert_trigger", "backdoor_features", "remove_backdoor"]


# ------------------------------------------------------------------------------------------------------------------- what is accepted
def _check_pipeline(pipeline, what: str):
    """NotImplementedError for what this module is not built for, saying which and where to go instead.  Touches no device."""
    from .ncsnpp import NCSNppModel
    from .pipelines import DiffusionPipeline, LDMPipeline
    from .unet import UNet2DModel
    from .vqmodel import VQModel
    name = type(pipeline).__name__
    if not isinstance(pipeline, DiffusionPipeline):
        raise TypeError(f"{what} needs a villandiffusion_amd LDMPipeline, got {name}")
    unet, sched = pipeline.unet, pipeline.scheduler
    if isinstance(unet, NCSNppModel):
        raise NotImplementedError(f"{what}: {name} with an NCSNppModel is a score-SDE (VE) pipeline; use villandiffusion_amd.defense_ve "
                                  f"(defense_ldm is for LDMPipeline: VQModel + latent UNet2DModel)")
    if not isinstance(pipeline, LDMPipeline) or getattr(pipeline, "vqvae", None) is None:
        raise NotImplementedError(f"{what}: {name} is a pixel-space pipeline; use villandiffusion_amd.defense / villandiffusion_amd.mitigation "
                                  f"(defense_ldm is for LDMPipeline: VQModel + latent UNet2DModel)")
    if not isinstance(pipeline.vqvae, VQModel):
        raise NotImplementedError(f"{what}: {name} with a {type(pipeline.vqvae).__name__} as its VAE is out of scope; the project's VQModel only")
    if not isinstance(unet, UNet2DModel) or not getattr(unet, "_input_grad", False):
        raise NotImplementedError(f"{what}: {name} with a {type(unet).__name__} is out of scope; a UNet2DModel with the input-gradient pass only")
    from .schedulers import KarrasVeScheduler, ScoreSdeVeScheduler
    if isinstance(sched, (ScoreSdeVeScheduler, KarrasVeScheduler)) or not hasattr(sched, "alphas_cumprod"):
        raise NotImplementedError(f"{what}: {name} with a {type(sched).__name__} is out of scope: a VE-type scheduler; the LDM defences are built "
                                  f"for VP-type (DDPM-style) noise schedules only")
    if int(pipeline.vqvae.config.latent_channels) != int(unet.in_channels):
        raise ValueError(f"{what}: the VQModel has {pipeline.vqvae.config.latent_channels} latent channels, the UNet takes {unet.in_channels}")


def _shapes(pipeline):
    """(latent shape, pixel shape): the UNet's input and the image the encoder maps onto it (one stride-2 convolution per level but the last)."""
    z = _shape(pipeline.unet)
    cfg = pipeline.vqvae.config
    f = 2 ** (len(cfg.block_out_channels) - 1)
    return z, (int(cfg.in_channels), z[1] * f, z[2] * f)


def _space_of(what, pipeline, trigger) -> str:
    z, p = _shapes(pipeline)
    shape = tuple(trigger.shape) if torch.is_tensor(trigger) else None
    if shape == z:                                         # (a pipeline whose two shapes coincide has no downsampling: latent it is)
        return "latent"
    if shape == p:
        return "pixel"
    raise ValueError(f"{what}: trigger must be latent-shaped {z} or pixel-shaped {p}, got {shape if shape is not None else type(trigger).__name__}")


def trigger_space(pipeline, trigger: torch.Tensor) -> str:
    """"latent" or "pixel", by the trigger's shape; ValueError for neither."""
    _check_pipeline(pipeline, "trigger_space")
    return _space_of("trigger_space", pipeline, trigger)


def _encode(pipeline, p):
    return pipeline.encode(p.detach().unsqueeze(0))[0]


def _latent(pipeline, trigger, space):
    """The trigger in latent space on the pipeline's device: a pixel trigger is encoded, once."""
    tau = trigger.detach().to(pipeline.device, torch.float32).contiguous()
    return _encode(pipeline, tau) if space == "pixel" else tau


def encode_trigger(pipeline, pixel_trigger: torch.Tensor) -> torch.Tensor:
    """The latent trigger [C, h, w] a pixel trigger [3, S, S] stands for: `pipeline.encode(trigger[None])[0]`, what the attack adds to the noise."""
    _check_pipeline(pipeline, "encode_trigger")
    _, pshape = _shapes(pipeline)
    if not torch.is_tensor(pixel_trigger) or tuple(pixel_trigger.shape) != pshape:
        raise ValueError(f"encode_trigger: the pixel trigger must be {pshape}, got "
                         f"{tuple(pixel_trigger.shape) if torch.is_tensor(pixel_trigger) else type(pixel_trigger).__name__}")
    from . import lib
    lib.require_device()
    return _encode(pipeline, pixel_trigger.to(pipeline.device, torch.float32))


def render_trigger(pipeline, latent_trigger: torch.Tensor) -> torch.Tensor:
    """A latent trigger [C, h, w] as a pixel image [3, S, S] in the model's range: the pipeline's own decode, quantised as `LDMPipeline.__call__`
    does it (clamp(x / 2 + 1 / 2, 0, 1) of it is what a picture shows).  For looking at; the decoder is not an inverse of the encoder."""
    _check_pipeline(pipeline, "render_trigger")
    zshape, _ = _shapes(pipeline)
    if not torch.is_tensor(latent_trigger) or tuple(latent_trigger.shape) != zshape:
        raise ValueError(f"render_trigger: the latent trigger must be {zshape}, got "
                         f"{tuple(latent_trigger.shape) if torch.is_tensor(latent_trigger) else type(latent_trigger).__name__}")
    from . import lib
    lib.require_device()
    return pipeline.vqvae.decode(latent_trigger.detach().to(pipeline.device, torch.float32).unsqueeze(0)).sample[0]


# ------------------------------------------------------------------------------------------------------------------------- inversion
def _pixel_objective_into(pipeline, p, eps, t, lam, loss, dz, partial):
    """One pixel-space evaluation: z = encode(p) at batch 1, the latent objective at tau = z into loss / dz (dz with its direct term), and dL/dz
    pulled back through the encoder.  -> dL/dp, [3, S, S].  Both networks frozen and the VQModel's input gradients on, by the caller."""
    x = p.detach().unsqueeze(0).requires_grad_(True)
    with torch.enable_grad():
        z4 = pipeline.vqvae.encode(x).latents
    if z4.grad_fn is None:
        raise RuntimeError("trigger inversion: the VQModel did not keep a tape (is this inside vqvae.input_gradients()?)")
    _objective_into(pipeline.unet, z4.detach()[0], eps, t, lam, loss, dz, partial)
    dx, = torch.autograd.grad(z4, x, dz.unsqueeze(0))
    return dx[0]


def inversion_objective(pipeline, p: torch.Tensor, eps: torch.Tensor, t, lam: float = 0.5):
    """(loss, dp) of L(p) = || mean_b unet(eps[b] + encode(p), t) - lam * encode(p) ||_2 at frozen weights: loss a [1] device tensor, dp like the
    pixel image p.  eps: [B, C, h, w] latent noise.  For tests and for callers with an optimiser of their own; the parameters' requires_grad
    flags and the VQModel's input-gradient switch are restored on exit."""
    _check_pipeline(pipeline, "inversion_objective")
    zshape, pshape = _shapes(pipeline)
    if not torch.is_tensor(p) or tuple(p.shape) != pshape:
        raise ValueError(f"inversion_objective: p must be a pixel image {pshape}, got {tuple(p.shape) if torch.is_tensor(p) else type(p).__name__}")
    _check_pair("inversion_objective", torch.empty(zshape, device="meta"), eps)
    from . import lib
    lib.require_device()
    dev = pipeline.device
    p = p.detach().to(dev, torch.float32).contiguous()
    eps = eps.detach().to(dev, torch.float32).contiguous()
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    dz = torch.empty(zshape, device=dev, dtype=torch.float32)
    partial = torch.empty(1024, device=dev, dtype=torch.float32)
    vq = pipeline.vqvae
    with _frozen(pipeline.unet), _frozen(vq), vq.input_gradients():
        dp = _pixel_objective_into(pipeline, p, eps, t, float(lam), loss, dz, partial)
    return loss, dp


def _clamp_into(p, out, lo, hi):
    """out = clamp(p, lo, hi) (vd_postprocess with the identity map)."""
    ops.postprocess(p.unsqueeze(0), out.unsqueeze(0), 1.0, 0.0, lo, hi, False)
    return out


def _run_pixel_inversion(pipeline, zshape, pshape, T, lam, lr, steps, batch, seed, init, noise, clamp):
    """Adam(lr) on the pixel image p for `steps` iterations, clamped after every step.  -> (p, the objective at the START of every iteration)"""
    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = pipeline.device
    if init is not None:
        p = init.detach().to(dev, torch.float32).contiguous().clone()
    else:
        p = torch.rand(pshape, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32).to(dev)
    q = torch.empty_like(p)                                # the clamp's output: p and q swap roles every iteration
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    dz = torch.empty(zshape, device=dev, dtype=torch.float32)
    losses = torch.zeros(steps, device=dev, dtype=torch.float32)
    partial = torch.empty(1024, device=dev, dtype=torch.float32)
    t = torch.full((batch,), T, device=dev, dtype=torch.int64)
    eps_buf = torch.empty((batch,) + zshape, device=dev, dtype=torch.float32)
    per_iter = (eps_buf.numel() + 3) // 4                  # Philox counters one iteration's noise consumes (four normals each)
    for it in range(steps):
        eps = _noise_of("invert_trigger", noise, it, eps_buf, seed, per_iter, dev)
        dp = _pixel_objective_into(pipeline, p, eps, t, lam, losses[it:it + 1], dz, partial)
        adam_update(p, dp, m, v, it + 1, lr)
        if clamp is not None:
            p, q = _clamp_into(p, q, clamp[0], clamp[1]), p
    return p, [float(x) for x in losses.cpu().tolist()]    # the one read of the loop's results


def invert_trigger(pipeline, *, space: str = "latent", steps: int, batch: int, lam: float = 0.5, lr: float = 0.1, seed: int = 0,
                   timestep: Optional[int] = None, init: Optional[torch.Tensor] = None,
                   noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                   clamp: Optional[tuple] = (-1.0, 1.0)) -> TriggerInversion:
    """Minimise the distribution-shift objective of the latent UNet over a trigger.

    space="latent": `defense.invert_trigger(pipeline.unet, pipeline.scheduler, ...)`, the same result (`clamp` does not apply: a latent has no
    range), with extra = {"space": "latent"}.  space="pixel": the variable is a pixel image p, the objective is evaluated at tau = encode(p) (see
    the module docstring); `init` is pixel-shaped (default U[0, 1) from `seed`), `noise` stays latent-shaped ([steps, batch, C, h, w] or a
    callable), `clamp` = (lo, hi) is applied to p after every Adam step (None: no clamp).  The result's trigger is p and extra =
    {"space": "pixel", "latent": encode(p)}."""
    # everything that can be checked is checked before the device is touched
    _check_pipeline(pipeline, "invert_trigger")
    if space not in ("latent", "pixel"):
        raise ValueError(f"invert_trigger: space must be 'latent' or 'pixel', got {space!r}")
    unet, sched, vq = pipeline.unet, pipeline.scheduler, pipeline.vqvae
    if space == "latent":
        res = defense.invert_trigger(unet, sched, steps=steps, batch=batch, lam=lam, lr=lr, seed=seed, timestep=timestep, init=init, noise=noise)
        res.extra = {"space": "latent"}
        return res
    zshape, pshape = _shapes(pipeline)
    _, lam, lr = _check_inversion_args("invert_trigger", unet, steps, batch, lam, lr, noise, None)
    if init is not None and (not torch.is_tensor(init) or tuple(init.shape) != pshape):
        raise ValueError(f"invert_trigger: in pixel space init must be {pshape}, got {tuple(init.shape) if torch.is_tensor(init) else type(init).__name__}")
    if clamp is not None:
        if len(clamp) != 2 or not float(clamp[0]) < float(clamp[1]):
            raise ValueError(f"invert_trigger: clamp must be (lo, hi) with lo < hi, or None, got {clamp!r}")
        clamp = (float(clamp[0]), float(clamp[1]))
    T = _vp_timestep("invert_trigger", sched, timestep)
    with _frozen(unet), _frozen(vq), vq.input_gradients():
        p, losses = _run_pixel_inversion(pipeline, zshape, pshape, T, lam, lr, steps, batch, seed, init, noise, clamp)
    return TriggerInversion(trigger=p, losses=losses, lam=lam, lr=lr, steps=steps, batch=batch, timestep=T, seed=int(seed),
                            extra={"space": "pixel", "latent": _encode(pipeline, p)})


# ------------------------------------------------------------------------------------------------------------------ detection features
class ImageSetAccumulator:
    """`mitigation.image_set_stats` of a set that arrives in chunks: `.add(x_chunk)` makes the two-pass call on the chunk and merges its result
    into the running one (`vd_image_set_merge`); nothing of the chunk is kept.  `.result()` reads the two sums back (the one host read).  A chunk
    of one image is fine: the two-pass kernel takes N = 1 (mean = the image, no deviation).  One chunk gives the resident call's bits."""

    def __init__(self, shape, device, postprocess: bool = True):
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3:
            raise ValueError(f"ImageSetAccumulator: shape is one image's (C, H, W), got {shape!r}")
        from . import lib
        lib.require_device()
        self.n = 0
        self._post = (0.5, 0.5, 0.0, 1.0) if postprocess else (1.0, 0.0, float("-inf"), float("inf"))
        f32 = dict(device=device, dtype=torch.float32)
        self._mean, self._mean_b = torch.empty(self.shape, **f32), torch.empty(self.shape, **f32)
        self._stats, self._stats_b = torch.zeros(2, **f32), torch.empty(2, **f32)
        self._partial = torch.empty(2048, **f32)

    def add(self, x: torch.Tensor) -> "ImageSetAccumulator":
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != self.shape or x.shape[0] < 1:
            raise ValueError(f"ImageSetAccumulator.add: a chunk is [N >= 1, {', '.join(map(str, self.shape))}], got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        N, _, H, W = (int(s) for s in x.shape)
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride()[1:] != (H * W, W, 1):
            x = x.contiguous()
        ops.image_set_stats(x, self._mean_b, self._stats_b, self._partial, *self._post)
        ops.image_set_merge(self._mean, self._stats, self.n, self._mean_b, self._stats_b, N, self._partial)
        self.n += N
        return self

    def result(self) -> ImageSetStats:
        if self.n < 2:
            raise ValueError(f"ImageSetAccumulator: a pairwise statistic needs N >= 2 images, got {self.n}")
        dev_sq, tv_sum = self._stats.cpu().tolist()          # the one host read
        return ImageSetStats(n=self.n, uniformity=2.0 / (self.n - 1) * dev_sq, tv=tv_sum / self.n, mean_image=self._mean.clone())


@dataclass
class LDMBackdoorFeatures(BackdoorFeatures):
    """The inherited fields hold the statistics of the decoded images (what the pipeline returns); the latent_* ones those of the final latents."""
    latent_clean: Optional[ImageSetStats] = None
    latent_shifted: Optional[ImageSetStats] = None
    latent_uniformity_ratio: float = float("nan")
    space: str = "latent"                  # the space the caller's trigger came in

    def as_dict(self) -> dict:
        return super().as_dict() | {"latent": {"clean": self.latent_clean.as_dict(), "shifted": self.latent_shifted.as_dict(),
                                               "uniformity_ratio": self.latent_uniformity_ratio}, "space": self.space}


def backdoor_features(pipeline, trigger: torch.Tensor, *, n: int, batch: int, num_inference_steps: Optional[int] = None,
                      seed: int = 0) -> LDMBackdoorFeatures:
    """Sample n latents from eps and n from eps + trigger (the same eps: `mitigation.backdoor_features`'s Philox chunks at latent shape) through
    the latent loop of `LDMPipeline.__call__`, chunk by chunk, and compare the two sets twice: on the final latents and on the decoded images
    the pipeline returns.  trigger: latent-shaped, or pixel-shaped (then encoded once).  Each chunk is decoded, measured, merged and freed
    (`ImageSetAccumulator`): nothing larger than one chunk of decoded images is held.  The scheduler's seed and offset are handled as
    `mitigation.backdoor_features` handles them and put back afterwards."""
    from .pipelines import DiffusionPipeline
    _check_pipeline(pipeline, "backdoor_features")
    space = _space_of("backdoor_features", pipeline, trigger)
    _check_count("backdoor_features", "n", n)
    _check_count("backdoor_features", "batch", batch)
    if n < 2:
        raise ValueError(f"backdoor_features: a pairwise statistic needs n >= 2 images, got {n}")
    steps = int(num_inference_steps) if num_inference_steps is not None else int(pipeline.default_steps)
    if steps < 1:
        raise ValueError(f"backdoor_features: num_inference_steps must be positive, got {steps}")
    sch = pipeline.scheduler

    from . import lib
    lib.require_device()
    dev = pipeline.device
    zshape, pshape = _shapes(pipeline)
    tau = _latent(pipeline, trigger, space)
    own_seed = hasattr(sch, "device_rng_seed") and sch.device_rng_seed is None
    off0 = getattr(sch, "_rng_offset", None)
    if own_seed:
        sch.device_rng_seed = int(seed) + 1
    try:
        inits = _feature_inits(pipeline, n, batch, seed)
        sets = []
        for shifted in (False, True):
            if off0 is not None:
                sch._rng_offset = off0                    # the shifted set draws the step noise the clean one drew
            lat_acc, pix_acc = ImageSetAccumulator(zshape, dev, postprocess=False), ImageSetAccumulator(pshape, dev, postprocess=True)
            for c in inits:
                if shifted:
                    ops.add_strided(c, tau.unsqueeze(0).expand_as(c), accumulate=True)      # eps + tau, in place: the same eps
                lat = DiffusionPipeline.__call__(pipeline, init=c, num_inference_steps=steps, return_tensor=True)
                lat_acc.add(lat)
                pix_acc.add(pipeline.vqvae.decode(lat).sample)                              # (freed before the next chunk is decoded)
            sets.append((lat_acc.result(), pix_acc.result()))
    finally:
        if own_seed:
            sch.device_rng_seed = None
            if off0 is not None:
                sch._rng_offset = off0
    (lc, pc), (ls, ps) = sets
    return LDMBackdoorFeatures(clean=pc, shifted=ps, uniformity_ratio=_ratio(ps.uniformity, pc.uniformity), tv_ratio=_ratio(ps.tv, pc.tv), n=n,
                               batch=batch, num_inference_steps=steps, seed=int(seed), latent_clean=lc, latent_shifted=ls,
                               latent_uniformity_ratio=_ratio(ls.uniformity, lc.uniformity), space=space)


# ------------------------------------------------------------------------------------------------------------------------------ removal
def remove_backdoor(pipeline, trigger: torch.Tensor, *, steps: int, batch: int, lr: float, w_clean: float = 1.0, w_shift: float = 1.0,
                    max_grad_norm: Optional[float] = 1.0, seed: int = 0, timestep: Optional[int] = None,
                    noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None, anchor_lambda: Optional[float] = None,
                    fisher: Optional[torch.Tensor] = None) -> BackdoorRemoval:
    """`mitigation.remove_backdoor(pipeline.unet, pipeline.scheduler, tau, ...)` at tau = the trigger in latent space (a pixel-shaped trigger is
    encoded once): the latent UNet is fine-tuned IN PLACE, the curves and the weights afterwards are that call's.  The VQ-VAE is untouched."""
    # everything that can be checked is checked before the device is touched (a pixel trigger is encoded on the device)
    _check_pipeline(pipeline, "remove_backdoor")
    space = _space_of("remove_backdoor", pipeline, trigger)
    unet, sched = pipeline.unet, pipeline.scheduler
    _check_removal_args("remove_backdoor", float(w_clean), float(w_shift), max_grad_norm)
    _check_f16("remove_backdoor", unet)
    mitigation._anchor_args("remove_backdoor", unet, anchor_lambda, fisher)
    _check_loop_args("remove_backdoor", unet, steps, batch, float(lr), noise, _shape(unet))
    _vp_timestep("remove_backdoor", sched, timestep)
    if space == "pixel":
        from . import lib
        lib.require_device()
    tau = _latent(pipeline, trigger, space) if space == "pixel" else trigger
    return mitigation.remove_backdoor(unet, sched, tau, steps=steps, batch=batch, lr=lr, w_clean=w_clean,
                                      w_shift=w_shift, max_grad_norm=max_grad_norm, seed=seed, timestep=timestep, noise=noise,
                                      **({} if anchor_lambda is None else dict(anchor_lambda=anchor_lambda, fisher=fisher)))
