"""Adversarial Neuron Pruning (Wu & Wang, NeurIPS 2021) on the HIP path: the clean-data, trigger-free defence BadDiffusion evaluates beside
inference-time clipping.  A neuron is an output row of a weight tensor.  ANP learns a mask m in [0, 1] over the neurons on a small clean set,

      min_m   alpha * L(m * w, b)  +  (1 - alpha) * max_{|delta|, |xi| <= eps} L((m + delta) * w, (1 + xi) * b),

L the clean noise-prediction loss mse(model(q_sample(x0, noise, t), t), noise), and prunes the neurons whose mask collapses: the ones a backdoor
lives in are the ones that are sensitive to the perturbation and useless on clean data.

Every parameter is a view of one flat f32 buffer (`flatnet`), so a neuron-scaled network is "write (m + delta) * w0 rows into `flat_param`, run the
ordinary forward and backward", and the chain rule through the scaling is a row dot product of the ordinary weight gradient with the base weights:

      dL/dm_j = dL/ddelta_j = sum_k g[j, k] * w0[j, k],        dL/dxi_j = g[bias j] * w0[bias j].

Three kernels do it, each ONE launch for the whole network over a neuron table built once on the host (`neuron_table`): `vd_neuron_scale` writes
the scaled weights, `vd_neuron_grad` the row dots, `vd_neuron_step` the projected sign / momentum steps of delta, xi and m.  No convolution kernel
is touched.  One learning step with a perturbation is anp_steps + 2 forward + backward passes, each after its own write of the weights; the
base weights live in a clone and `flat_param` is restored from it bit for bit on exit: learning a mask never changes the model.  Nothing syncs with
the host inside the loop.

`prune_neurons` then zeroes the weight rows of the selected neurons (biases stay); the result is an ordinary diffusers-format checkpoint.

This module is the pixel-space VP-type `UNet2DModel`'s; `anp_ve` (NCSN++ with `ScoreSdeVeScheduler`) and `anp_ldm` (`LDMPipeline`) carry the same
names.  The pass sequence, the state vectors, the argument checks, the restore discipline, `NeuronMask` and the three loops (`_run_objective`,
`_run_learning`, `_run_curve`) live here once, parameterised by a `_Family`: a loss object, how the model is called (t or sigma_t, without or
with a `pscale`) and the parameters that are never unfrozen.  Single process.  (Data-parallel mask learning is not built.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from . import ops
from .defense import _check_loop_args, _noise_of, _shape, _trainable
from .mitigation import _check_f16

__all__ = ["NeuronTable", "neuron_table", "anp_objective", "NeuronMask", "learn_neuron_mask", "prune_neurons"]     # (+ pruning_curve, by name)

LAYERS = ("conv", "all")


def _check_model(what, model, noise_sched):
    """NotImplementedError for what ANP is not built for, saying which."""
    from .schedulers import KarrasVeScheduler, ScoreSdeVeScheduler
    from .unet import UNet2DModel
    if not isinstance(model, UNet2DModel):
        raise TypeError(f"{what} needs a villandiffusion_amd UNet2DModel, got {type(model).__name__}")
    if not getattr(model, "_input_grad", False):
        raise NotImplementedError(f"{what}: {type(model).__name__} is a score-SDE (VE) network; use villandiffusion_amd.anp_ve (anp is for the "
                                  f"pixel-space VP-type UNet2DModel; an LDMPipeline goes to villandiffusion_amd.anp_ldm)")
    if isinstance(noise_sched, (ScoreSdeVeScheduler, KarrasVeScheduler)) or not hasattr(noise_sched, "alphas_cumprod"):
        raise NotImplementedError(f"{what}: {type(noise_sched).__name__} is a VE-type scheduler; the clean loss here is the VP-type (DDPM-style) "
                                  f"noise-prediction loss (NCSNppModel with ScoreSdeVeScheduler goes to villandiffusion_amd.anp_ve)")


# ------------------------------------------------------------------------------------------------------------------------------ the neuron table
@dataclass
class NeuronTable:
    """jobs: one (weight offset in floats, rows, row length, bias offset or -1, index of the layer's first neuron, first workgroup) per selected
    weight tensor -- the rows of the device table of vd_neuron_scale / vd_neuron_grad, where a job owns ceil(rows / 4) workgroups.  slices: the
    weight's dotted name -> its slice of a per-neuron vector (jobs are in the order of this dict).  Unpacks as (jobs, n_neurons, slices)."""
    jobs: List[Tuple[int, int, int, int, int, int]]
    n_neurons: int
    slices: Dict[str, slice]
    layers: Optional[str] = None
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        neuron = block = 0
        if not self.jobs:
            raise ValueError("neuron table: no jobs")
        for k, (off, rows, ln, boff, n0, b0) in enumerate(self.jobs):
            if off < 0 or rows < 1 or ln < 1 or boff < -1 or n0 != neuron or b0 != block:
                raise ValueError(f"neuron table: job {k} = {(off, rows, ln, boff, n0, b0)} (expected first neuron {neuron}, first workgroup {block})")
            neuron += rows
            block += (rows + 3) // 4
        if neuron != self.n_neurons:
            raise ValueError(f"neuron table: the jobs hold {neuron} neurons, not {self.n_neurons}")
        self.n_jobs, self.total_blocks = len(self.jobs), block
        self.weight_floats = sum(j[1] * j[2] for j in self.jobs)
        self.n_bias = sum(j[1] for j in self.jobs if j[3] >= 0)
        self.extent = max(max(j[0] + j[1] * j[2], j[3] + j[1] if j[3] >= 0 else 0) for j in self.jobs)     # floats a flat buffer must hold

    def __iter__(self):
        return iter((self.jobs, self.n_neurons, self.slices))

    def device_table(self, device) -> torch.Tensor:
        """The [n_jobs, 6] int64 table on `device`, uploaded once."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = ops.upload_table(torch.tensor(self.jobs, dtype=torch.int64), device)
        return self._dev[key]


def _is_output_head(name: str) -> bool:
    return name == "conv_out.weight" or (name.startswith("up_blocks.") and name.endswith(".skip_conv.weight"))


def neuron_table(model, layers: str = "conv") -> NeuronTable:
    """The neurons of `model` (any flat-parameter network; pure host code, a device="cpu" model will do).  layers="conv": every parameter named
    *.weight with 4 dimensions; "all": every parameter with >= 2 dimensions (adds the attention projections and the time-embedding linears).
    A weight whose rows are the network's output (image) channels is never selected: `conv_out.weight`, and the heads of NCSN++'s output-image
    pyramid, `up_blocks.*.skip_conv.weight` (`down_blocks.*.skip_conv.weight`, whose rows are feature channels, is an ordinary layer).  A 1-d
    parameter (NCSN++'s fixed `time_proj.weight`) is no layer.  A neuron's bias is <prefix>.bias where the model has one."""
    if layers not in LAYERS:
        raise ValueError(f"neuron_table: layers must be one of {LAYERS}, got {layers!r}")
    jobs, slices, neuron, block = [], {}, 0, 0
    for name, shape, _ in model._layout:
        if _is_output_head(name) or not (len(shape) >= 2 if layers == "all" else (len(shape) == 4 and name.endswith(".weight"))):
            continue
        off, n, _ = model._offs[name]
        rows = int(shape[0])
        bias = name[:-len("weight")] + "bias" if name.endswith(".weight") else None
        boff = model._offs[bias][0] if bias in model._offs and model._offs[bias][1] == rows else -1
        jobs.append((int(off), rows, n // rows, int(boff), neuron, block))
        slices[name] = slice(neuron, neuron + rows)
        neuron += rows
        block += (rows + 3) // 4
    if not jobs:
        raise ValueError(f"neuron_table: {type(model).__name__} has no layer for layers={layers!r}")
    return NeuronTable(jobs, neuron, slices, layers)


# ------------------------------------------------------------------------------------------------------------------------------ one evaluation
@dataclass(frozen=True)
class _Family:
    """What a model family brings to the shared passes.  loss: an object with `get_inputs_targets(x0, R, t, eps)` (a `LossFn`); call: t (int64
    timestep indices on the device) -> (what the model is called with, the `pscale` of the loss kernel or None); skip: parameters that are
    never unfrozen; T_train: how many timesteps the loss tables hold.  clean_shape / prepare: a family whose clean set may arrive in another
    space (latent diffusion's pixel images) names that set's (C, H, W) and the map onto the model's input, which runs once, on the device, after
    every check; None: the clean set is the model's input."""
    loss: object
    call: Callable
    skip: tuple
    T_train: int
    clean_shape: Optional[tuple] = None
    prepare: Optional[Callable] = None


def _loss_fn(noise_sched):
    from .loss import SDE_VP, LossFn
    return LossFn(noise_sched, SDE_VP, psi=1)


def _vp_family(noise_sched, loss=None, clean_shape=None, prepare=None) -> _Family:
    """The VP-type family: the model is called with the timestep itself and predicts the noise."""
    return _Family(loss=loss if loss is not None else _loss_fn(noise_sched), call=lambda t: (t, None), skip=(),
                   T_train=int(noise_sched.config.num_train_timesteps), clean_shape=clean_shape, prepare=prepare)


class _Passes:
    """The state the passes of one call share: the base weights `w0` (a clone), the table, the loss tables and the scratch of the loss kernel.
    family: a `_Family` (default: the VP-type one of `noise_sched`)."""

    def __init__(self, model, noise_sched, tab: NeuronTable, family: Optional[_Family] = None):
        self.fam = family if family is not None else _vp_family(noise_sched)
        self.model, self.tab, self.lf = model, tab, self.fam.loss
        self.w0 = model.flat_param.detach().clone()
        self.partial = torch.empty(1024, device=model.device, dtype=torch.float32)
        self.zero_R = None
        self._called = (None, None, None)

    def inputs(self, x0, eps, t):
        """(x_t, y): the noised clean images and the target of the clean loss (the noise: the poison image is zero)."""
        if self.zero_R is None or self.zero_R.shape != x0.shape:
            self.zero_R = torch.zeros_like(x0)
        return self.lf.get_inputs_targets(x0, self.zero_R, t, eps)

    def call_args(self, t):
        """(what the model is called with, pscale) at the timesteps t; worked out once per batch, not once per pass."""
        if self._called[0] is not t:
            self._called = (t,) + tuple(self.fam.call(t))
        return self._called[1:]

    def write(self, mask, delta, xi):
        """flat_param <- the neuron-scaled base weights.  A raw-pointer write: no version counter sees it, so the caches derived from the weights
        (packed split-precision operands, transposed weights) are invalidated by hand, as trainer._swap_ema does."""
        ops.neuron_scale(self.w0, self.model.flat_param, self.tab, mask, delta, xi)
        ops.WEIGHTS_EPOCH += 1
        self.model.weights_changed()

    def run(self, x_t, y, t, mask, delta, xi, loss):
        """Forward + backward at (mask + delta, 1 + xi): `loss` ([1] view) is written, model.flat_grad holds the weight gradients of this pass."""
        model = self.model
        tm, pscale = self.call_args(t)
        self.write(mask, delta, xi)
        model.zero_grad()
        with torch.enable_grad():
            pred = model(x_t, tm)[0]
        if pred.grad_fn is None:
            raise RuntimeError("adversarial neuron pruning: the model did not take its training forward (are all of its parameters frozen?)")
        dpred = torch.empty_like(pred)
        ops.mse_fwd_bwd(pred.detach().contiguous(), y, dpred, loss, self.partial, pscale=pscale)
        pred.backward(dpred)

    def forward_loss(self, x_t, y, t, mask, loss):
        """The no-grad forward at the weights mask * w0 (biases as they are): `loss` ([1] view) is written.  No gradient is touched."""
        tm, pscale = self.call_args(t)
        self.write(mask, None, None)
        with torch.no_grad():
            pred = self.model(x_t, tm)[0]
        ops.mse_fwd_bwd(pred.contiguous(), y, torch.empty_like(pred), loss, self.partial, pscale=pscale)

    def grad(self, gmask, gxi, scale=1.0, accumulate=False):
        """gmask (+)= scale * dL/dmask, gxi (+)= scale * dL/dxi of the pass that has just run."""
        ops.neuron_grad(self.model.flat_grad, self.w0, self.tab, gmask, gxi, scale=scale, accumulate=accumulate)

    def step(self, st, x_t, y, t, start, cfg, curves):
        """One step of `learn_neuron_mask` (its docstring) on the state `st` (mask, buf, gm, gd, gx, delta, xi); start: the [2, n] draws;
        curves: [2 + anp_steps] view -- natural, robust, the ascent passes.  (tools/anp_step_ab.py times this very function.)"""
        eps, k_asc, alpha = cfg.anp_eps, cfg.anp_steps, cfg.anp_alpha
        adversarial = eps > 0.0
        if adversarial:
            st.delta.copy_(start[0])
            st.xi.copy_(start[1])
            for k in range(k_asc):
                self.run(x_t, y, t, st.mask, st.delta, st.xi, curves[2 + k:3 + k])
                self.grad(st.gd, st.gx)
                ops.neuron_step(st.delta, st.gd, lr=-eps / k_asc, lo=-eps, hi=eps, use_sign=True)
                ops.neuron_step(st.xi, st.gx, lr=-eps / k_asc, lo=-eps, hi=eps, use_sign=True)
            self.run(x_t, y, t, st.mask, st.delta, st.xi, curves[1:2])
            self.grad(st.gm, None, scale=1.0 - alpha)
        self.run(x_t, y, t, st.mask, None, None, curves[0:1])
        self.grad(st.gm, None, scale=alpha if adversarial else 1.0, accumulate=adversarial)
        ops.neuron_step(st.mask, st.gm, st.buf, lr=cfg.lr, momentum=cfg.momentum, lo=0.0, hi=1.0)

    def restore(self):
        with torch.no_grad():
            self.model.flat_param.copy_(self.w0)                   # bit for bit
        ops.WEIGHTS_EPOCH += 1
        self.model.weights_changed()
        self.model.zero_grad()


def _state(n, dev):
    """The per-neuron vectors of the loop: the mask starts at 1, the momentum buffer and xi's gradient (bias-less neurons keep 0) at 0."""
    new = lambda fill: torch.full((n,), fill, device=dev, dtype=torch.float32)
    return SimpleNamespace(mask=new(1.0), buf=new(0.0), gm=new(0.0), gd=new(0.0), gx=new(0.0), delta=new(0.0), xi=new(0.0))


def _check_clean(what, clean, shape):
    if not torch.is_tensor(clean) or clean.dim() != 4 or tuple(clean.shape[1:]) != shape or clean.shape[0] < 1 or not clean.is_floating_point():
        raise ValueError(f"{what}: clean must be a float [N, C, H, W] tensor with (C, H, W) = {shape}, got "
                         f"{tuple(clean.shape) if torch.is_tensor(clean) else type(clean).__name__}")


def _check_per_neuron(what, name, v, n):
    if not torch.is_tensor(v) or v.dim() != 1 or v.numel() != n:
        raise ValueError(f"{what}: {name} must be a [{n}] tensor (one entry per neuron), got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")


def _check_objective_args(what, model, clean, t, eps, mask, delta, xi, layers, clean_shape=None):
    """-> the neuron table.  Everything about one evaluation that can be checked without the device."""
    _check_clean(what, clean, clean_shape or _shape(model))
    B = clean.shape[0]
    if not torch.is_tensor(eps) or tuple(eps.shape) != (B,) + _shape(model):
        raise ValueError(f"{what}: eps must be like clean {(B,) + _shape(model)}, got {tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}")
    if not torch.is_tensor(t) or t.numel() != B:
        raise ValueError(f"{what}: t must hold one timestep per image ({B})")
    if not torch.is_tensor(mask) or mask.dim() != 1:
        raise ValueError(f"{what}: mask must be a 1-d tensor, one entry per neuron")
    tabs = [neuron_table(model, layers)] if layers is not None else [neuron_table(model, k) for k in LAYERS]
    tab = next((tb for tb in tabs if tb.n_neurons == mask.numel()), None)
    if tab is None:
        raise ValueError(f"{what}: mask has {mask.numel()} entries; the model has {', '.join(f'{tb.n_neurons} ({tb.layers})' for tb in tabs)} neurons")
    for name, v in (("delta", delta), ("xi", xi)):
        if v is not None:
            _check_per_neuron(what, name, v, tab.n_neurons)
    return tab


def _run_objective(what, model, tab, family, clean, t, eps, mask, delta, xi):
    """One evaluation for any family, after the caller's checks: (loss [1], gmask [n], gxi [n]) on the device.  `flat_param` is restored bit for
    bit and the requires_grad flags come back on exit."""
    from . import lib
    lib.require_device()
    dev = model.device
    up = lambda v: None if v is None else v.detach().to(dev, torch.float32).contiguous()
    mask, delta, xi = up(mask), up(delta), up(xi)
    if family.prepare is not None:
        clean = family.prepare(clean, int(clean.shape[0]))
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    gmask = torch.empty(tab.n_neurons, device=dev, dtype=torch.float32)
    gxi = torch.zeros(tab.n_neurons, device=dev, dtype=torch.float32)
    with _trainable(model, family.skip):
        ps = _Passes(model, None, tab, family)
        try:
            tt = t.to(dev).reshape(-1).to(torch.int64)
            x_t, y = ps.inputs(up(clean), up(eps), tt)
            ps.run(x_t, y, tt, mask, delta, xi, loss)
            ps.grad(gmask, gxi)
        finally:
            ps.restore()
    return loss, gmask, gxi


def anp_objective(model, noise_sched, clean: torch.Tensor, t: torch.Tensor, eps: torch.Tensor, mask: torch.Tensor,
                  delta: Optional[torch.Tensor] = None, xi: Optional[torch.Tensor] = None, layers: Optional[str] = None):
    """(loss, gmask, gxi) device tensors of the clean loss mse(model(q_sample(clean, eps, t), t), eps) at the weights (mask + delta) * w rows and
    (1 + xi) * b biases: loss [1], gmask = dL/dmask = dL/ddelta [n], gxi = dL/dxi [n] (zero where a neuron has no bias).  mask (delta, xi): one
    entry per neuron in `neuron_table` order; layers=None takes the selection whose neuron count mask has.  `flat_param` is restored bit for bit and
    the requires_grad flags come back on exit.  For tests and for callers with an optimiser of their own."""
    what = "anp_objective"
    _check_model(what, model, noise_sched)
    _check_f16(what, model)
    tab = _check_objective_args(what, model, clean, t, eps, mask, delta, xi, layers)
    return _run_objective(what, model, tab, _vp_family(noise_sched), clean, t, eps, mask, delta, xi)


# ------------------------------------------------------------------------------------------------------------------------------ learning the mask
@dataclass
class NeuronMask:
    masks: Dict[str, torch.Tensor]         # weight name -> [rows] f32 on the host, in neuron-table order
    natural: List[float]                   # per step: the clean loss at (m, 1) at the START of the step (read once, after the loop)
    robust: List[float]                    # per step: the loss at the perturbed weights (m + delta, 1 + xi); empty when anp_eps == 0
    layers: str
    steps: int
    batch: int
    anp_eps: float
    anp_steps: int
    anp_alpha: float
    lr: float
    momentum: float
    seed: int
    last_delta: Optional[torch.Tensor] = None      # delta and xi after the last step's ascent, on the host (None when anp_eps == 0)
    last_xi: Optional[torch.Tensor] = None

    @property
    def n_neurons(self) -> int:
        return sum(int(v.numel()) for v in self.masks.values())

    def flat(self) -> torch.Tensor:
        return torch.cat([v.reshape(-1) for v in self.masks.values()])

    def settings(self) -> dict:
        return {k: getattr(self, k) for k in ("layers", "steps", "batch", "anp_eps", "anp_steps", "anp_alpha", "lr", "momentum", "seed")} | \
            {"n_neurons": self.n_neurons}


def _check_learn_args(what, model, clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, timesteps, noise, perturbation,
                      shape, T_train):
    """-> the neuron table.  Everything that can be checked without the device."""
    _check_clean(what, clean, shape)
    _check_loop_args(what, model, steps, batch, lr, noise, shape)
    if not isinstance(anp_steps, int) or isinstance(anp_steps, bool) or anp_steps < 1:
        raise ValueError(f"{what}: anp_steps must be a positive int, got {anp_steps!r}")
    if not (anp_eps >= 0.0 and math.isfinite(anp_eps)):
        raise ValueError(f"{what}: anp_eps must be finite and non-negative, got {anp_eps!r}")
    if not 0.0 <= anp_alpha <= 1.0:
        raise ValueError(f"{what}: anp_alpha must lie in [0, 1], got {anp_alpha!r}")
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"{what}: momentum must lie in [0, 1), got {momentum!r}")
    tab = neuron_table(model, layers)                            # ValueError for an unknown selection
    if torch.is_tensor(timesteps):
        if tuple(timesteps.shape) != (steps, batch) or timesteps.is_floating_point():
            raise ValueError(f"{what}: timesteps must be an integer [steps, batch] = {(steps, batch)} tensor, got {tuple(timesteps.shape)} "
                             f"{timesteps.dtype}")
        if int(timesteps.min()) < 0 or int(timesteps.max()) >= T_train:
            raise ValueError(f"{what}: timesteps outside the scheduler's [0, {T_train})")
    elif timesteps is not None and not callable(timesteps):
        raise TypeError(f"{what}: timesteps is None, a tensor or a callable step -> [batch]")
    if torch.is_tensor(perturbation):
        if tuple(perturbation.shape) != (steps, 2, tab.n_neurons):
            raise ValueError(f"{what}: perturbation must be [steps, 2, neurons] = {(steps, 2, tab.n_neurons)}, got {tuple(perturbation.shape)}")
        if float(perturbation.abs().max()) > anp_eps * (1.0 + 1e-6):            # (an f32 anp_eps may round above the double)
            raise ValueError(f"{what}: perturbation leaves [-anp_eps, anp_eps] = +-{anp_eps}")
    elif perturbation is not None and not callable(perturbation):
        raise TypeError(f"{what}: perturbation is None, a tensor or a callable step -> [2, neurons]")
    return tab


def _of_step(what, name, src, it, shape, dev, dtype):
    v = src[it] if torch.is_tensor(src) else src(it)
    if not torch.is_tensor(v) or tuple(v.shape) != shape:
        raise ValueError(f"{what}: {name}({it}) must be {shape}, got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
    return v.detach().to(dev, dtype).contiguous()


def _run_learning(what, model, family, clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, seed, timesteps, noise,
                  perturbation) -> NeuronMask:
    """The mask-learning loop of `learn_neuron_mask` (its docstring) for any family: the argument checks that need no device, the draws, the
    loop, the restore.  The caller has checked that `model` (and its arithmetic) belongs to `family`."""
    anp_eps, anp_alpha, lr, momentum = float(anp_eps), float(anp_alpha), float(lr), float(momentum)
    shape = _shape(model)
    T_train = family.T_train
    if family.clean_shape is not None:                     # the clean set arrives in another space: its own shape check, then a stand-in
        _check_clean(what, clean, family.clean_shape)
        stand_in = torch.empty((clean.shape[0],) + shape, device="meta", dtype=torch.float32)
    else:
        stand_in = clean
    tab = _check_learn_args(what, model, stand_in, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, timesteps, noise,
                            perturbation, shape, T_train)
    n = tab.n_neurons
    adversarial = anp_eps > 0.0
    if adversarial and perturbation is None:
        perturbation = (torch.rand((steps, 2, n), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32) * 2 - 1) * anp_eps
    if timesteps is None:
        timesteps = torch.randint(0, T_train, (steps, batch), generator=torch.Generator().manual_seed(int(seed) + 1))

    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = model.device
    if family.prepare is not None:
        clean = family.prepare(clean, batch)
    data = clean.detach().to(dev, torch.float32).contiguous()
    N = data.shape[0]
    if torch.is_tensor(timesteps):
        timesteps = timesteps.to(dev, torch.int64)
    if torch.is_tensor(perturbation):
        perturbation = perturbation.to(dev, torch.float32)
    cfg = SimpleNamespace(anp_eps=anp_eps, anp_steps=anp_steps, anp_alpha=anp_alpha, lr=lr, momentum=momentum)
    st = _state(n, dev)
    curves = torch.zeros((steps, 2 + anp_steps), device=dev, dtype=torch.float32)      # natural, robust, the ascent passes
    eps_buf = torch.empty((batch,) + shape, device=dev, dtype=torch.float32)
    x0_buf = torch.empty_like(eps_buf)
    per_iter = (eps_buf.numel() + 3) // 4                  # Philox counters one step's noise consumes (four normals each)
    with _trainable(model, family.skip):                   # every weight gradient is needed; the caller's flags come back on exit
        ps = _Passes(model, None, tab, family)
        try:
            for it in range(steps):
                first = (it * batch) % N
                if first + batch <= N:
                    x0 = data[first:first + batch]
                else:                                      # the batch wraps round the end of the clean set
                    for k in range(batch):
                        x0_buf[k].copy_(data[(first + k) % N])
                    x0 = x0_buf
                eps = _noise_of(what, noise, it, eps_buf, seed, per_iter, dev)
                t = _of_step(what, "timesteps", timesteps, it, (batch,), dev, torch.int64)
                start = _of_step(what, "perturbation", perturbation, it, (2, n), dev, torch.float32) if adversarial else None
                x_t, y = ps.inputs(x0, eps, t)
                ps.step(st, x_t, y, t, start, cfg, curves[it])
        finally:
            ps.restore()
    host, m = curves.cpu(), st.mask.cpu()                     # the one read of the loop's results
    res = NeuronMask(masks={name: m[sl].clone() for name, sl in tab.slices.items()}, natural=[float(v) for v in host[:, 0].tolist()],
                     robust=[float(v) for v in host[:, 1].tolist()] if adversarial else [], layers=layers, steps=steps, batch=batch,
                     anp_eps=anp_eps, anp_steps=anp_steps, anp_alpha=anp_alpha, lr=lr, momentum=momentum, seed=int(seed))
    if adversarial:
        res.last_delta, res.last_xi = st.delta.cpu(), st.xi.cpu()
    return res


def learn_neuron_mask(model, noise_sched, clean: torch.Tensor, *, steps: int, batch: int, anp_eps: float = 0.4, anp_steps: int = 1,
                      anp_alpha: float = 0.2, lr: float = 0.2, momentum: float = 0.9, layers: str = "conv", seed: int = 0,
                      timesteps: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      noise: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None,
                      perturbation: Union[None, torch.Tensor, Callable[[int], torch.Tensor]] = None) -> NeuronMask:
    """Learn ANP's neuron mask on the clean images `clean` ([N, C, H, W] f32 in the model's value range; used in order and cyclically, `batch`
    per step).  The model is left exactly as it was found.  One step, with the same images, timesteps and noise in every pass:

      1. anp_eps > 0: delta, xi <- U(-anp_eps, anp_eps); anp_steps times: pass at (m + delta, 1 + xi), then
         delta, xi <- clamp(. + (anp_eps / anp_steps) * sign(gradient), +-anp_eps);
      2. anp_eps > 0: the robust pass at (m + delta, 1 + xi):  gm  = (1 - anp_alpha) * dL/dm;
      3. the natural pass at (m, 1):                           gm += anp_alpha * dL/dm     (anp_eps == 0: the only pass, weight 1);
      4. buf <- momentum * buf + gm;  m <- clamp(m - lr * buf, 0, 1).

    The mask starts at 1.  The uniform draws are (torch.rand((steps, 2, n), generator=CPU Generator(seed)) * 2 - 1) * anp_eps, drawn up front
    -- row [step, 0] is delta's start, [step, 1] xi's -- unless `perturbation` supplies them (that tensor, or a callable step -> [2, n]).
    timesteps: None -- torch.randint(0, T, (steps, batch)) from a CPU Generator(seed + 1), drawn up front; a [steps, batch] tensor or a callable
    step -> [batch].  noise: None -- fresh per step from the device Philox stream of `seed`; a [steps, batch, C, H, W] tensor or a callable
    step -> [batch, C, H, W].  Tensors and callables make a run reproducible against another implementation."""
    what = "learn_neuron_mask"
    _check_model(what, model, noise_sched)
    _check_f16(what, model)
    return _run_learning(what, model, _vp_family(noise_sched), clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, seed,
                         timesteps, noise, perturbation)


# ------------------------------------------------------------------------------------------------------------------------------------- pruning
def _selection(who, model, mask, threshold=None, fraction=None):
    """-> (the "all" neuron table, drop: a bool per neuron of that table, picks: weight name -> the row indices to zero, for the layers `mask`
    names).  The selection rule of `prune_neurons` (its docstring), with every check of it; pure host code, nothing is written."""
    if (threshold is None) == (fraction is None):
        raise ValueError(f"{who}: give exactly one of threshold and fraction")
    masks = mask.masks if isinstance(mask, NeuronMask) else mask
    if not isinstance(masks, dict) or not masks:
        raise TypeError(f"{who}: mask must be a NeuronMask or a non-empty dict name -> [rows] tensor, got {type(mask).__name__}")
    full = neuron_table(model, "all")
    order = [name for name in full.slices if name in masks]          # neuron-table order, whatever the dict's
    unknown = [name for name in masks if name not in order]
    if unknown:
        raise ValueError(f"{who}: {unknown[:3]} are not neuron layers of this {type(model).__name__}")
    for name in order:
        rows = int(model._offs[name][2][0])
        if not torch.is_tensor(masks[name]) or masks[name].numel() != rows:
            raise ValueError(f"{who}: the mask of {name} must hold {rows} entries")
    flat = torch.cat([masks[name].detach().reshape(-1).to("cpu", torch.float32) for name in order])
    n = flat.numel()
    if threshold is not None:
        threshold = float(threshold)
        if not math.isfinite(threshold):
            raise ValueError(f"{who}: threshold must be finite, got {threshold!r}")
        drop = flat < threshold
    else:
        fraction = float(fraction)
        if not 0.0 <= fraction < 1.0:
            raise ValueError(f"{who}: fraction must lie in [0, 1), got {fraction!r}")
        drop = torch.zeros(n, dtype=torch.bool)
        drop[torch.sort(flat, stable=True).indices[:int(math.floor(fraction * n))]] = True      # stable: ties by neuron index
    picks, first = {}, 0
    dropped = torch.zeros(full.n_neurons, dtype=torch.bool)
    for name in order:
        rows = masks[name].numel()
        idx = drop[first:first + rows].nonzero().reshape(-1)
        if idx.numel() == rows:
            raise ValueError(f"{who}: the selection prunes every neuron of {name}; nothing was written")
        picks[name] = idx
        dropped[full.slices[name]] = drop[first:first + rows]
        first += rows
    return full, dropped, picks


def prune_neurons(model, mask, *, threshold: Optional[float] = None, fraction: Optional[float] = None) -> Dict[str, int]:
    """Zero the weight rows of the neurons `mask` (a NeuronMask, or a weight name -> [rows] dict) selects, in place: threshold prunes m_j <
    threshold (ANP's default is 0.2); fraction prunes the floor(fraction * n) smallest masks of the whole network, ties by neuron index.  Biases
    stay and every other float keeps its bits.  A selection that would prune a whole layer raises ValueError naming it before anything is
    written; so does a mask that names a weight that is no neuron layer (`conv_out.weight`, NCSN++'s `up_blocks.*.skip_conv.weight`).  Plain
    torch writes: works on a device="cpu" model, a `UNet2DModel` or an `NCSNppModel`.  -> weight name -> rows pruned."""
    _, _, picks = _selection("prune_neurons", model, mask, threshold=threshold, fraction=fraction)
    with torch.no_grad():
        for name, idx in picks.items():
            if idx.numel():
                model.P[name][idx.to(model.P[name].device)] = 0.0
    ops.WEIGHTS_EPOCH += 1                                  # writes through .data views: no version counter of flat_param sees them
    model.weights_changed()
    return {name: int(idx.numel()) for name, idx in picks.items()}


# ------------------------------------------------------------------------------------------------------------------------- the pruning curve
def _run_curve(what, model, family, clean, mask, thresholds, fractions, seed, timesteps, noise) -> List[dict]:
    """`pruning_curve` (its docstring) for any family, after the caller's checks of the model."""
    if (thresholds is None) == (fractions is None):
        raise ValueError(f"{what}: give exactly one of thresholds and fractions")
    key, cands = ("threshold", thresholds) if thresholds is not None else ("fraction", fractions)
    try:
        cands = [float(c) for c in cands]
    except TypeError:
        raise TypeError(f"{what}: {key}s must be a sequence of numbers, got {type(cands).__name__}") from None
    shape = _shape(model)
    _check_clean(what, clean, family.clean_shape or shape)
    B = int(clean.shape[0])
    if int(model.out_channels) != shape[0]:
        raise ValueError(f"{what}: the loss compares the model's output with its input: out_channels {model.out_channels} != in_channels "
                         f"{model.in_channels}")
    if timesteps is not None:
        if not torch.is_tensor(timesteps) or tuple(timesteps.shape) != (B,) or timesteps.is_floating_point():
            raise ValueError(f"{what}: timesteps must be None or an integer [{B}] tensor, one per image")
        if int(timesteps.min()) < 0 or int(timesteps.max()) >= family.T_train:
            raise ValueError(f"{what}: timesteps outside the scheduler's [0, {family.T_train})")
    if noise is not None and (not torch.is_tensor(noise) or tuple(noise.shape) != (B,) + shape):
        raise ValueError(f"{what}: noise must be None or a {(B,) + shape} tensor, one unit-variance image per clean image")
    sels = [_selection(what, model, mask, **{key: c}) for c in cands]             # ValueError for an emptied layer, before anything runs
    tab = sels[0][0] if sels else neuron_table(model, "all")
    hard = torch.ones((len(sels) + 1, tab.n_neurons), dtype=torch.float32)        # row 0: the unpruned model
    for k, (_, dropped, _) in enumerate(sels):
        hard[k + 1][dropped] = 0.0
    if timesteps is None:
        timesteps = torch.randint(0, family.T_train, (1, B), generator=torch.Generator().manual_seed(int(seed) + 1))[0]

    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = model.device
    hard = hard.to(dev)
    if family.prepare is not None:
        clean = family.prepare(clean, B)
    x0 = clean.detach().to(dev, torch.float32).contiguous()
    t = timesteps.to(dev, torch.int64).contiguous()
    eps_buf = torch.empty_like(x0)
    eps = _noise_of(what, None if noise is None else noise.unsqueeze(0), 0, eps_buf, seed, (eps_buf.numel() + 3) // 4, dev)
    losses = torch.zeros(len(sels) + 1, device=dev, dtype=torch.float32)
    ps = _Passes(model, None, tab, family)
    try:
        x_t, y = ps.inputs(x0, eps, t)
        for k in range(len(sels) + 1):
            ps.forward_loss(x_t, y, t, hard[k], losses[k:k + 1])
    finally:
        ps.restore()
    host = losses.cpu().tolist()                           # the one read of the results
    return [{key: None, "pruned": 0, "loss": float(host[0])}] + \
        [{key: c, "pruned": int(sel[1].sum()), "loss": float(v)} for c, sel, v in zip(cands, sels, host[1:])]


def pruning_curve(model, noise_sched, clean: torch.Tensor, mask, *, thresholds=None, fractions=None, seed: int = 0,
                  timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> List[dict]:
    """The clean loss a learnt mask costs at each candidate selection: what an ANP user chooses the threshold with.  mask: a NeuronMask or a
    name -> [rows] dict; thresholds= or fractions=: the candidates, each read as `prune_neurons` reads it.  -> one record per candidate,
    {"threshold" | "fraction": the candidate, "pruned": rows it zeroes, "loss": the clean loss of the model with exactly those rows zeroed},
    after record 0, the unpruned model (candidate None, pruned 0).

    `clean` ([B, C, H, W]) is ONE batch; every record is a no-grad forward over the same images, timesteps and noise, at weights written by
    `vd_neuron_scale` with a mask of zeros and ones and no xi (so biases, and the rows that stay, keep their bits).  timesteps: None --
    torch.randint(0, T, (1, B)) from a CPU Generator(seed + 1), step 0's draw of the learning loop at batch B; or an integer [B] tensor.
    noise: None -- the learning loop's step-0 draw from the device Philox stream of `seed`; or a tensor like clean.  A candidate that would
    empty a layer raises ValueError naming it before anything runs.  The model is restored bit for bit, also after an exception."""
    what = "pruning_curve"
    _check_model(what, model, noise_sched)
    _check_f16(what, model)
    return _run_curve(what, model, _vp_family(noise_sched), clean, mask, thresholds, fractions, seed, timesteps, noise)
