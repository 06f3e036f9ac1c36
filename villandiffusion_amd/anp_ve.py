"""Adversarial Neuron Pruning (`anp`, whose module docstring states the method) for the score network of SDE-VE: `NCSNppModel` with
`ScoreSdeVeScheduler`.  The same function names and result types as `anp`, which stays VP-only; the neuron table, the pass sequence, the state
vectors, the argument checks, the loops and the restore discipline are `anp`'s, imported.  What is here is what SDE-VE alone needs.

The clean loss is the VE training loss with a zero poison image, `LossFn(noise_sched, SDE_VE, psi=0)`:

      x_t = x0 + sigma_t * eps,        L = mean((-sigma_t * model(x_t, sigma_t) - eps)^2),

through `LossFn.get_inputs_targets` and `ops.mse_fwd_bwd(..., pscale=-sigma_t)`: the model is called with the noise level and its score is read
as the noise prediction -sigma * s.  `timesteps` index the ascending TRAINING sigma table of `num_train_timesteps` entries, rebuilt from
`scheduler.config` as `defense_ve` rebuilds it (a pipeline's `set_sigmas(n)` shrinks the scheduler's own table to n inference steps; that one is
never read here).  Clean images are in the VE range [0, 1].

Neurons: `anp.neuron_table`.  The heads of the output-image pyramid (`conv_out.weight`, `up_blocks.*.skip_conv.weight`: their rows are the image
channels) are never selected; `down_blocks.*.skip_conv.weight`, a 1x1 convolution from the 3 image channels with 3-float rows, is an ordinary
layer.  `time_proj.weight`, the fixed Fourier features, is no layer and stays frozen in every pass.

bf16x3 and f32 arithmetic, single process.  No efficacy is claimed: no genuinely backdoored NCSN++ checkpoint exists to try it on.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import torch

from . import anp
from .anp import NeuronMask, NeuronTable, neuron_table  # noqa: F401

__all__ = ["NeuronTable", "neuron_table", "anp_objective", "NeuronMask", "learn_neuron_mask", "prune_neurons", "pruning_curve"]


# ------------------------------------------------------------------------------------------------------------------- what is accepted
def _check_model(what, model, noise_sched):
    """NotImplementedError for what this module is not built for, saying which and where to go instead.  -> the scheduler.  Touches no device."""
    from .ncsnpp import NCSNppModel
    from .pipelines import DiffusionPipeline, ScoreSdeVePipeline
    from .schedulers import ScoreSdeVeScheduler
    from .unet import UNet2DModel
    if isinstance(model, DiffusionPipeline):
        raise NotImplementedError(f"{what}: {type(model).__name__} is a pipeline; anp_ve takes the NCSNppModel and its ScoreSdeVeScheduler (an "
                                  f"LDMPipeline goes to villandiffusion_amd.anp_ldm)")
    if not isinstance(model, NCSNppModel):
        if isinstance(model, UNet2DModel):
            raise NotImplementedError(f"{what}: {type(model).__name__} is a VP-type network; use villandiffusion_amd.anp (pixel space) or "
                                      f"villandiffusion_amd.anp_ldm (an LDMPipeline); anp_ve is for NCSNppModel with ScoreSdeVeScheduler")
        raise TypeError(f"{what} needs a villandiffusion_amd NCSNppModel, got {type(model).__name__}")
    if isinstance(noise_sched, ScoreSdeVePipeline):
        noise_sched = noise_sched.scheduler
    if not isinstance(noise_sched, ScoreSdeVeScheduler):
        raise NotImplementedError(f"{what}: {type(noise_sched).__name__} is out of scope; anp_ve is built for ScoreSdeVeScheduler only (VP-type "
                                  f"schedulers belong to villandiffusion_amd.anp and villandiffusion_amd.anp_ldm)")
    mode = getattr(model, "conv_math", None)
    if mode in ("f16", "bf16"):
        raise NotImplementedError(f"{what}: conv_math '{mode}' is not supported for the NCSN++ defences; use 'bf16x3' or 'f32'")
    return noise_sched


def _family(model, noise_sched) -> anp._Family:
    """The SDE-VE family: the loss tables of a scheduler rebuilt from the configuration (the training table), the model called with sigma_t, the
    loss kernel scaling its output by -sigma_t, and the Fourier features never unfrozen."""
    from .loss import SDE_VE, LossFn
    lf = LossFn(type(noise_sched)(**vars(noise_sched.config)), SDE_VE, psi=0)

    def call(t):
        sig = lf._tables(t.device)[3][t].contiguous()
        return sig, (-sig).contiguous()
    return anp._Family(loss=lf, call=call, skip=(model.time_proj.weight,), T_train=int(lf._sigmas_asc.numel()))


# ------------------------------------------------------------------------------------------------------------------------- the functions
def anp_objective(model, noise_sched, clean: torch.Tensor, t: torch.Tensor, eps: torch.Tensor, mask: torch.Tensor,
                  delta: Optional[torch.Tensor] = None, xi: Optional[torch.Tensor] = None, layers: Optional[str] = None):
    """`anp.anp_objective` for the VE clean loss of the module docstring: (loss [1], gmask [n], gxi [n]) device tensors at the weights
    (mask + delta) * w rows and (1 + xi) * b biases.  t: indices into the ascending training sigma table.  `flat_param` is restored bit for bit,
    the requires_grad flags come back on exit and `time_proj.weight` is never unfrozen."""
    what = "anp_objective"
    sched = _check_model(what, model, noise_sched)
    tab = anp._check_objective_args(what, model, clean, t, eps, mask, delta, xi, layers)
    fam = _family(model, sched)
    if t.is_floating_point() or int(t.min()) < 0 or int(t.max()) >= fam.T_train:
        raise ValueError(f"{what}: t must hold integer indices into the training sigma table, [0, {fam.T_train})")
    return anp._run_objective(what, model, tab, fam, clean, t, eps, mask, delta, xi)


def learn_neuron_mask(model, noise_sched, clean: torch.Tensor, *, steps: int, batch: int, anp_eps: float = 0.4, anp_steps: int = 1,
                      anp_alpha: float = 0.2, lr: float = 0.2, momentum: float = 0.9, layers: str = "conv", seed: int = 0,
                      timesteps: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      perturbation: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None) -> NeuronMask:
    """`anp.learn_neuron_mask` (its docstring: the step, the draws, the arguments) on an NCSNppModel with the VE clean loss.  noise_sched: a
    ScoreSdeVeScheduler (or a ScoreSdeVePipeline, for its scheduler).  clean: [N, C, H, W] in [0, 1].  timesteps: indices into the ascending
    training sigma table; None draws torch.randint(0, num_train_timesteps, (steps, batch)) from a CPU Generator(seed + 1).  noise: unit
    variance.  The model is left exactly as it was found."""
    what = "learn_neuron_mask"
    sched = _check_model(what, model, noise_sched)
    return anp._run_learning(what, model, _family(model, sched), clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, seed,
                             timesteps, noise, perturbation)


def prune_neurons(model, mask, *, threshold: Optional[float] = None, fraction: Optional[float] = None):
    """`anp.prune_neurons` on an NCSNppModel: a mask that names `conv_out.weight` or an `up_blocks.*.skip_conv.weight` is a ValueError."""
    from .ncsnpp import NCSNppModel
    if not isinstance(model, NCSNppModel):
        raise TypeError(f"prune_neurons needs a villandiffusion_amd NCSNppModel, got {type(model).__name__} (villandiffusion_amd.anp prunes a "
                        f"UNet2DModel)")
    return anp.prune_neurons(model, mask, threshold=threshold, fraction=fraction)


def pruning_curve(model, noise_sched, clean: torch.Tensor, mask, *, thresholds=None, fractions=None, seed: int = 0,
                  timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> List[dict]:
    """`anp.pruning_curve` (its docstring) with the VE clean loss: one record per candidate after record 0, the unpruned model."""
    what = "pruning_curve"
    sched = _check_model(what, model, noise_sched)
    return anp._run_curve(what, model, _family(model, sched), clean, mask, thresholds, fractions, seed, timesteps, noise)
