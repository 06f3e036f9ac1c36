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

Pixel-space VP-type `UNet2DModel`s, single process.  (NCSN++ / SDE-VE, latent diffusion and data-parallel mask learning are not built.)
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

__all__ = ["NeuronTable", "neuron_table", "anp_objective", "NeuronMask", "learn_neuron_mask", "prune_neurons"]

LAYERS = ("conv", "all")


def _check_model(what, model, noise_sched):
    """NotImplementedError for what ANP is not built for, saying which."""
    from .schedulers import KarrasVeScheduler, ScoreSdeVeScheduler
    from .unet import UNet2DModel
    if not isinstance(model, UNet2DModel):
        raise TypeError(f"{what} needs a villandiffusion_amd UNet2DModel, got {type(model).__name__}")
    if not getattr(model, "_input_grad", False):
        raise NotImplementedError(f"{what}: {type(model).__name__} is out of scope (NCSN++ / score-SDE models are not built; VP-type UNet2DModel only)")
    if isinstance(noise_sched, (ScoreSdeVeScheduler, KarrasVeScheduler)) or not hasattr(noise_sched, "alphas_cumprod"):
        raise NotImplementedError(f"{what}: {type(noise_sched).__name__} is a VE-type scheduler; the clean loss here is the VP-type (DDPM-style) "
                                  f"noise-prediction loss")


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


def neuron_table(model, layers: str = "conv") -> NeuronTable:
    """The neurons of `model` (any flat-parameter network; pure host code, a device="cpu" model will do).  layers="conv": every parameter named
    *.weight with 4 dimensions; "all": every parameter with >= 2 dimensions (adds the attention projections and the time-embedding linears).
    `conv_out.weight` is never selected: its rows are the image channels.  A neuron's bias is <prefix>.bias where the model has one."""
    if layers not in LAYERS:
        raise ValueError(f"neuron_table: layers must be one of {LAYERS}, got {layers!r}")
    jobs, slices, neuron, block = [], {}, 0, 0
    for name, shape, _ in model._layout:
        if name == "conv_out.weight" or not (len(shape) >= 2 if layers == "all" else (len(shape) == 4 and name.endswith(".weight"))):
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
def _loss_fn(noise_sched):
    from .loss import SDE_VP, LossFn
    return LossFn(noise_sched, SDE_VP, psi=1)


class _Passes:
    """The state the passes of one call share: the base weights `w0` (a clone), the table, the loss tables and the scratch of the loss kernel."""

    def __init__(self, model, noise_sched, tab: NeuronTable):
        self.model, self.tab, self.lf = model, tab, _loss_fn(noise_sched)
        self.w0 = model.flat_param.detach().clone()
        self.partial = torch.empty(1024, device=model.device, dtype=torch.float32)
        self.zero_R = None

    def inputs(self, x0, eps, t):
        """(x_t, y): q_sample of clean images and the target of the clean loss (the noise: the poison image is zero)."""
        if self.zero_R is None or self.zero_R.shape != x0.shape:
            self.zero_R = torch.zeros_like(x0)
        return self.lf.get_inputs_targets(x0, self.zero_R, t, eps)

    def write(self, mask, delta, xi):
        """flat_param <- the neuron-scaled base weights.  A raw-pointer write: no version counter sees it, so the caches derived from the weights
        (packed split-precision operands, transposed weights) are invalidated by hand, as trainer._swap_ema does."""
        ops.neuron_scale(self.w0, self.model.flat_param, self.tab, mask, delta, xi)
        ops.WEIGHTS_EPOCH += 1
        self.model.weights_changed()

    def run(self, x_t, y, t, mask, delta, xi, loss):
        """Forward + backward at (mask + delta, 1 + xi): `loss` ([1] view) is written, model.flat_grad holds the weight gradients of this pass."""
        model = self.model
        self.write(mask, delta, xi)
        model.zero_grad()
        with torch.enable_grad():
            pred = model(x_t, t)[0]
        if pred.grad_fn is None:
            raise RuntimeError("adversarial neuron pruning: the model did not take its training forward (are all of its parameters frozen?)")
        dpred = torch.empty_like(pred)
        ops.mse_fwd_bwd(pred.detach().contiguous(), y, dpred, loss, self.partial)
        pred.backward(dpred)

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


def anp_objective(model, noise_sched, clean: torch.Tensor, t: torch.Tensor, eps: torch.Tensor, mask: torch.Tensor,
                  delta: Optional[torch.Tensor] = None, xi: Optional[torch.Tensor] = None, layers: Optional[str] = None):
    """(loss, gmask, gxi) device tensors of the clean loss mse(model(q_sample(clean, eps, t), t), eps) at the weights (mask + delta) * w rows and
    (1 + xi) * b biases: loss [1], gmask = dL/dmask = dL/ddelta [n], gxi = dL/dxi [n] (zero where a neuron has no bias).  mask (delta, xi): one
    entry per neuron in `neuron_table` order; layers=None takes the selection whose neuron count mask has.  `flat_param` is restored bit for bit and
    the requires_grad flags come back on exit.  For tests and for callers with an optimiser of their own."""
    what = "anp_objective"
    _check_model(what, model, noise_sched)
    _check_f16(what, model)
    shape = _shape(model)
    _check_clean(what, clean, shape)
    if not torch.is_tensor(eps) or tuple(eps.shape) != tuple(clean.shape):
        raise ValueError(f"{what}: eps must be like clean {tuple(clean.shape)}, got {tuple(eps.shape) if torch.is_tensor(eps) else type(eps).__name__}")
    B = clean.shape[0]
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
    from . import lib
    lib.require_device()
    dev = model.device
    up = lambda v: None if v is None else v.detach().to(dev, torch.float32).contiguous()
    mask, delta, xi = up(mask), up(delta), up(xi)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    gmask = torch.empty(tab.n_neurons, device=dev, dtype=torch.float32)
    gxi = torch.zeros(tab.n_neurons, device=dev, dtype=torch.float32)
    with _trainable(model):
        ps = _Passes(model, noise_sched, tab)
        try:
            tt = t.to(dev).reshape(-1).to(torch.int64)
            x_t, y = ps.inputs(up(clean), up(eps), tt)
            ps.run(x_t, y, tt, mask, delta, xi, loss)
            ps.grad(gmask, gxi)
        finally:
            ps.restore()
    return loss, gmask, gxi


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
    anp_eps, anp_alpha, lr, momentum = float(anp_eps), float(anp_alpha), float(lr), float(momentum)
    _check_model(what, model, noise_sched)
    _check_f16(what, model)
    shape = _shape(model)
    T_train = int(noise_sched.config.num_train_timesteps)
    tab = _check_learn_args(what, model, clean, steps, batch, anp_eps, anp_steps, anp_alpha, lr, momentum, layers, timesteps, noise, perturbation,
                            shape, T_train)
    n = tab.n_neurons
    adversarial = anp_eps > 0.0
    if adversarial and perturbation is None:
        perturbation = (torch.rand((steps, 2, n), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32) * 2 - 1) * anp_eps
    if timesteps is None:
        timesteps = torch.randint(0, T_train, (steps, batch), generator=torch.Generator().manual_seed(int(seed) + 1))

    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = model.device
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
    with _trainable(model):                                # every weight gradient is needed; the caller's flags come back on exit
        ps = _Passes(model, noise_sched, tab)
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


# ------------------------------------------------------------------------------------------------------------------------------------- pruning
def prune_neurons(model, mask, *, threshold: Optional[float] = None, fraction: Optional[float] = None) -> Dict[str, int]:
    """Zero the weight rows of the neurons `mask` (a NeuronMask, or a weight name -> [rows] dict) selects, in place: threshold prunes m_j <
    threshold (ANP's default is 0.2); fraction prunes the floor(fraction * n) smallest masks of the whole network, ties by neuron index.  Biases
    stay and every other float keeps its bits.  A selection that would prune a whole layer raises ValueError naming it before anything is
    written.  Plain torch writes: works on a device="cpu" model.  -> weight name -> rows pruned."""
    if (threshold is None) == (fraction is None):
        raise ValueError("prune_neurons: give exactly one of threshold and fraction")
    masks = mask.masks if isinstance(mask, NeuronMask) else mask
    if not isinstance(masks, dict) or not masks:
        raise TypeError(f"prune_neurons: mask must be a NeuronMask or a non-empty dict name -> [rows] tensor, got {type(mask).__name__}")
    order = [name for name in neuron_table(model, "all").slices if name in masks]          # neuron-table order, whatever the dict's
    unknown = [name for name in masks if name not in order]
    if unknown:
        raise ValueError(f"prune_neurons: {unknown[:3]} are not neuron layers of this {type(model).__name__}")
    for name in order:
        rows = int(model._offs[name][2][0])
        if not torch.is_tensor(masks[name]) or masks[name].numel() != rows:
            raise ValueError(f"prune_neurons: the mask of {name} must hold {rows} entries")
    flat = torch.cat([masks[name].detach().reshape(-1).to("cpu", torch.float32) for name in order])
    n = flat.numel()
    if threshold is not None:
        threshold = float(threshold)
        if not math.isfinite(threshold):
            raise ValueError(f"prune_neurons: threshold must be finite, got {threshold!r}")
        drop = flat < threshold
    else:
        fraction = float(fraction)
        if not 0.0 <= fraction < 1.0:
            raise ValueError(f"prune_neurons: fraction must lie in [0, 1), got {fraction!r}")
        drop = torch.zeros(n, dtype=torch.bool)
        drop[torch.sort(flat, stable=True).indices[:int(math.floor(fraction * n))]] = True      # stable: ties by neuron index
    picks, first = {}, 0
    for name in order:
        rows = masks[name].numel()
        idx = drop[first:first + rows].nonzero().reshape(-1)
        if idx.numel() == rows:
            raise ValueError(f"prune_neurons: the selection prunes every neuron of {name}; nothing was written")
        picks[name] = idx
        first += rows
    with torch.no_grad():
        for name, idx in picks.items():
            if idx.numel():
                model.P[name][idx.to(model.P[name].device)] = 0.0
    ops.WEIGHTS_EPOCH += 1                                  # writes through .data views: no version counter of flat_param sees them
    model.weights_changed()
    return {name: int(idx.numel()) for name, idx in picks.items()}
