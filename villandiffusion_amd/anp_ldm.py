"""Adversarial Neuron Pruning (`anp`, whose module docstring states the method) for the latent-diffusion pipeline: `LDMPipeline` with a
`VQModel`, a VP-type latent `UNet2DModel` and a VP-type scheduler.  The same function names and result types as `anp` (pixel-space VP models)
and `anp_ve` (NCSN++); every function here takes the pipeline, like `defense_ldm`, whose `_check_pipeline` decides what is accepted.

The mask is over the latent UNet alone: its neuron table is `anp.neuron_table(pipeline.unet)` (multi-head attention projections are ordinary
rows under layers="all"), and the VQ-VAE is never written.  The clean loss is `LossFn(scheduler, SDE_LDM, psi=1)` on latents.  `clean` lives in
one of two spaces, told apart by its shape as `defense_ldm` tells triggers apart:

* latent `[N, C, h, w]` (the UNet's input shape): used as it is;
* pixel `[N, 3, S, S]` (the VQ-VAE's input shape): encoded once up front with `pipeline.encode`, in chunks of `batch`, no grad, VQ-VAE frozen.

The pass sequence, the loops, the argument checks and the restore discipline are `anp`'s.  Single process; the VQ-VAE runs in f32, the UNet in
its own arithmetic.  No efficacy is claimed: no genuinely backdoored LDM checkpoint exists to try it on.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import torch

from . import anp
from .anp import NeuronMask, NeuronTable  # noqa: F401
from .defense import _frozen
from .defense_ldm import _check_pipeline as _check_ldm_pipeline
from .defense_ldm import _shapes
from .mitigation import _check_f16

__all__ = ["NeuronTable", "neuron_table", "clean_space", "anp_objective", "NeuronMask", "learn_neuron_mask", "prune_neurons", "pruning_curve"]


# ------------------------------------------------------------------------------------------------------------------- what is accepted
def _check_pipeline(what, pipeline):
    """`defense_ldm._check_pipeline`, after the two other families have been told where their ANP lives.  Touches no device."""
    from .ncsnpp import NCSNppModel
    from .pipelines import DiffusionPipeline, LDMPipeline
    from .unet import UNet2DModel
    name = type(pipeline).__name__
    if isinstance(pipeline, NCSNppModel) or (isinstance(pipeline, DiffusionPipeline) and isinstance(pipeline.unet, NCSNppModel)):
        raise NotImplementedError(f"{what}: {name} is score-SDE (VE); use villandiffusion_amd.anp_ve (anp_ldm is for LDMPipeline: VQModel + latent "
                                  f"UNet2DModel)")
    if isinstance(pipeline, UNet2DModel) or (isinstance(pipeline, DiffusionPipeline) and
                                             (not isinstance(pipeline, LDMPipeline) or getattr(pipeline, "vqvae", None) is None)):
        raise NotImplementedError(f"{what}: {name} is pixel-space; use villandiffusion_amd.anp with the UNet2DModel and its scheduler (anp_ldm "
                                  f"takes an LDMPipeline: VQModel + latent UNet2DModel)")
    _check_ldm_pipeline(pipeline, what)
    _check_f16(what, pipeline.unet)


def _space_of(what, pipeline, clean) -> str:
    z, p = _shapes(pipeline)
    shape = tuple(clean.shape) if torch.is_tensor(clean) else None
    if shape is not None and len(shape) == 4 and shape[0] >= 1 and clean.is_floating_point():
        if shape[1:] == z:                                 # (a pipeline whose two shapes coincide has no downsampling: latent it is)
            return "latent"
        if shape[1:] == p:
            return "pixel"
    raise ValueError(f"{what}: clean must be a float tensor of latents [N, {', '.join(map(str, z))}] or of pixel images "
                     f"[N, {', '.join(map(str, p))}], got {shape if shape is not None else type(clean).__name__}")


def clean_space(pipeline, clean: torch.Tensor) -> str:
    """"latent" or "pixel", by the shape of `clean`; ValueError for neither."""
    _check_pipeline("clean_space", pipeline)
    return _space_of("clean_space", pipeline, clean)


def _family(what, pipeline, clean) -> anp._Family:
    """The LDM family: the VP-type calls with the SDE_LDM loss tables; a pixel-shaped `clean` is encoded once, after every check, in chunks of
    `batch`, no grad, the VQ-VAE frozen."""
    from .loss import SDE_LDM, LossFn
    lf = LossFn(pipeline.scheduler, SDE_LDM, psi=1)
    if _space_of(what, pipeline, clean) == "latent":
        return anp._vp_family(pipeline.scheduler, lf)

    def encode(x, batch):
        x = x.detach().to(pipeline.device, torch.float32).contiguous()
        with torch.no_grad(), _frozen(pipeline.vqvae):
            return torch.cat([pipeline.encode(x[i:i + batch]) for i in range(0, x.shape[0], batch)])
    return anp._vp_family(pipeline.scheduler, lf, clean_shape=_shapes(pipeline)[1], prepare=encode)


def neuron_table(pipeline, layers: str = "conv") -> NeuronTable:
    """`anp.neuron_table` of the pipeline's latent UNet."""
    _check_pipeline("neuron_table", pipeline)
    return anp.neuron_table(pipeline.unet, layers)


# ------------------------------------------------------------------------------------------------------------------------- the functions
def anp_objective(pipeline, clean: torch.Tensor, t: torch.Tensor, eps: torch.Tensor, mask: torch.Tensor, delta: Optional[torch.Tensor] = None,
                  xi: Optional[torch.Tensor] = None, layers: Optional[str] = None):
    """`anp.anp_objective` of the latent UNet with the LDM clean loss: (loss [1], gmask [n], gxi [n]) device tensors.  clean: latents or pixel
    images (encoded first, as one chunk); eps: latent-shaped noise, one per image."""
    what = "anp_objective"
    _check_pipeline(what, pipeline)
    fam = _family(what, pipeline, clean)
    tab = anp._check_objective_args(what, pipeline.unet, clean, t, eps, mask, delta, xi, layers, fam.clean_shape)
    return anp._run_objective(what, pipeline.unet, tab, fam, clean, t, eps, mask, delta, xi)


def learn_neuron_mask(pipeline, clean: torch.Tensor, *, steps: int, batch: int, anp_eps: float = 0.4, anp_steps: int = 1, anp_alpha: float = 0.2,
                      lr: float = 0.2, momentum: float = 0.9, layers: str = "conv", seed: int = 0,
                      timesteps: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      perturbation: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None) -> NeuronMask:
    """`anp.learn_neuron_mask` (its docstring: the step, the draws, the arguments) on the pipeline's latent UNet.  clean: latents
    [N, C, h, w], or pixel images [N, 3, S, S] in the VQ-VAE's range, encoded once up front in chunks of `batch`.  noise and timesteps are the
    UNet's: latent-shaped.  The UNet is left exactly as it was found and the VQ-VAE is never written."""
    what = "learn_neuron_mask"
    _check_pipeline(what, pipeline)
    return anp._run_learning(what, pipeline.unet, _family(what, pipeline, clean), clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum,
                             layers, seed, timesteps, noise, perturbation)


def prune_neurons(pipeline, mask, *, threshold: Optional[float] = None, fraction: Optional[float] = None):
    """`anp.prune_neurons` on the pipeline's latent UNet, in place; the VQ-VAE is untouched."""
    _check_pipeline("prune_neurons", pipeline)
    return anp.prune_neurons(pipeline.unet, mask, threshold=threshold, fraction=fraction)


def pruning_curve(pipeline, clean: torch.Tensor, mask, *, thresholds=None, fractions=None, seed: int = 0,
                  timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> List[dict]:
    """`anp.pruning_curve` (its docstring) of the latent UNet with the LDM clean loss.  clean: ONE batch of latents, or of pixel images (encoded
    first, as one chunk)."""
    what = "pruning_curve"
    _check_pipeline(what, pipeline)
    return anp._run_curve(what, pipeline.unet, _family(what, pipeline, clean), clean, mask, thresholds, fractions, seed, timesteps, noise)
