"""Activation-based channel pruning on the HIP path: what a channel does on data, where ANP (`anp`) asks what its weights do under perturbation.

* Fine-Pruning (Liu, Dolan-Gavitt & Garg, RAID 2018): prune the channels that stay dormant on clean inputs, then fine-tune with the pruned
  channels held at zero (`Trainer(keep_pruned=...)`).
* Trigger-sensitivity pruning (the pruning half of Diff-Cleanse-style defences): given an inverted trigger, prune the channels whose activation
  statistics move most when the trigger is added to the input.

The tap points are the hidden channels of every ResnetBlock: a = silu(norm2(h1)), h1 = conv1's output plus the time embedding, the post-activation
of `conv1`'s output channels.  They are the only channels of a UNet that can be pruned structurally -- the residual stream is shared -- so "the
conv1 rows of every ResnetBlock" is the layer set.  A `save=True` forward keeps h1 and norm2's mean and rstd for every block; one table-driven
launch after the forward (`vd_channel_stats`) reads every h1 once and leaves the per-channel sum and sum of squares of a for the whole network.
No convolution, GroupNorm or attention kernel is touched, the weights are never written, and nothing is read back inside the loop over batches.

The scores are plain `weight name -> [rows]` dicts: they go straight into `prune_neurons` / `pruning_curve` of `anp` (the smallest score is
pruned first).  Biases stay, as with ANP: a pruned channel's pre-activation is its bias plus its time-embedding row, constant over space, not
zero.  Pixel-space `UNet2DModel` with a VP-type scheduler, and the latent UNet of an `LDMPipeline`; NCSN++ is not built.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import anp, ops
from .defense import _check_count, _check_trigger, _noise_of, _shape
from .mitigation import _check_f16

__all__ = ["ActivationTable", "activation_table", "ChannelStats", "channel_stats", "dormancy_scores", "sensitivity_scores", "PruneMask",
           "fine_prune"]

ACTS = tuple(ops.CHANNEL_ACTS)           # "raw": h1 itself; "silu_gn": silu(norm2(h1))
MASK_FILE = "prune_mask.pt"


# --------------------------------------------------------------------------------------------------------------------------- the tap table
@dataclass
class ActivationTable:
    """names: the `conv1.weight` of every ResnetBlock in tape order (down, mid, up: the order a save=True forward records them in); slices:
    name -> its slice of a per-channel vector; n_channels: their total."""
    names: List[str]
    slices: Dict[str, slice]
    n_channels: int

    def __iter__(self):
        return iter((self.names, self.slices, self.n_channels))


def _unet_of(what, model):
    """The UNet2DModel the statistics are taken of: `model` itself, or the latent UNet of an LDMPipeline.  NotImplementedError, naming what
    is missing, for NCSN++."""
    from .ncsnpp import NCSNppModel
    from .pipelines import DiffusionPipeline
    from .unet import UNet2DModel
    net = model.unet if isinstance(model, DiffusionPipeline) else model
    if isinstance(net, NCSNppModel):
        raise NotImplementedError(f"{what}: NCSNppModel is not built: its ResnetBlocks (FIR up/down-sampling inside the block, skip rescaling, "
                                  f"per-layer group counts) record their hidden tensor and norm statistics in a tape layout of their own, "
                                  f"which the job table here does not read; UNet2DModel (pixel-space VP, or the latent UNet of an LDMPipeline) only")
    if not isinstance(net, UNet2DModel):
        raise TypeError(f"{what} needs a villandiffusion_amd UNet2DModel or LDMPipeline, got {type(model).__name__}")
    return net


def _blocks(net):
    """The ResnetBlocks in tape order."""
    return [r for blk in net.down for r in blk["res"]] + list(net.mid_res) + [r for blk in net.up for r in blk["res"]]


def activation_table(model) -> ActivationTable:
    """The tap points of `model` (a UNet2DModel, or an LDMPipeline for its latent UNet): pure host code, a device="cpu" model will do.  Every
    name is a row of `anp.neuron_table(model, "conv")`, so a score dict over these names is a valid `prune_neurons` mask."""
    net = _unet_of("activation_table", model)
    names, slices, n = [], {}, 0
    for r in _blocks(net):
        name = r.prefix + ".conv1.weight"
        names.append(name)
        slices[name] = slice(n, n + r.cout)
        n += r.cout
    conv = anp.neuron_table(net, "conv").slices
    for name in names:
        assert name in conv and conv[name].stop - conv[name].start == slices[name].stop - slices[name].start, name
    return ActivationTable(names, slices, n)


# --------------------------------------------------------------------------------------------------------------------------- the statistics
@dataclass
class ChannelStats:
    """Per-channel sums of the tapped activation over `count[name]` values per channel (images x pixels), on the host in float64."""
    table: ActivationTable
    count: Dict[str, int]
    sum: np.ndarray                        # [n_channels] float64
    sumsq: np.ndarray                      # [n_channels] float64
    act: str = "silu_gn"
    batch: int = 0
    n_images: int = 0
    seed: int = 0
    triggered: bool = False
    settings_extra: dict = field(default_factory=dict)

    def _counts(self) -> np.ndarray:
        n = np.empty(self.table.n_channels, dtype=np.float64)
        for name, sl in self.table.slices.items():
            n[sl] = self.count[name]
        return n

    def mean(self) -> np.ndarray:
        return self.sum / self._counts()

    def rms(self) -> np.ndarray:
        return np.sqrt(self.sumsq / self._counts())

    def var(self) -> np.ndarray:
        """The (biased) variance, clamped at 0 against the cancellation of the two-sum form."""
        m = self.mean()
        return np.maximum(self.sumsq / self._counts() - m * m, 0.0)

    def per_layer(self, name: str) -> dict:
        sl = self.table.slices[name]
        return {"count": self.count[name], "sum": self.sum[sl], "sumsq": self.sumsq[sl], "mean": self.mean()[sl], "rms": self.rms()[sl],
                "var": self.var()[sl]}

    def settings(self) -> dict:
        return {"act": self.act, "batch": self.batch, "n_images": self.n_images, "seed": self.seed, "triggered": self.triggered,
                "n_channels": self.table.n_channels, "layers": len(self.table.names)} | self.settings_extra


def _family(what, model, noise_sched, images):
    """(the UNet, its `anp._Family`): the VP-type one of a pixel-space model, or the LDM one of a pipeline (pixel images are encoded by the
    helper `anp_ldm` uses)."""
    from .pipelines import DiffusionPipeline
    net = _unet_of(what, model)
    if isinstance(model, DiffusionPipeline) and getattr(model, "vqvae", None) is not None:
        from . import anp_ldm
        anp_ldm._check_pipeline(what, model)
        return net, anp_ldm._family(what, model, images)
    if isinstance(model, DiffusionPipeline):
        noise_sched = model.scheduler if noise_sched is None else noise_sched
    anp._check_model(what, net, noise_sched)
    _check_f16(what, net)
    return net, anp._vp_family(noise_sched)


def _taps(net, st, tab: ActivationTable, act: str):
    """The job list of one save=True forward: one tap per "res" record of the tape, in tape order."""
    recs = [rec for rec in st.saved if rec[0] == "res"]
    if len(recs) != len(tab.names):
        raise RuntimeError(f"channel_stats: the forward recorded {len(recs)} ResnetBlocks, the table holds {len(tab.names)}")
    taps = []
    for name, (_, res, saved) in zip(tab.names, recs):
        if res.prefix + ".conv1.weight" != name:
            raise RuntimeError(f"channel_stats: the tape holds {res.prefix} where the table expects {name}")
        h1, m2, r2 = saved[4], saved[6], saved[7]
        if act == "raw":
            taps.append((h1, None, None, None, None, res.norm2.groups, tab.slices[name].start))
        else:
            taps.append((h1, m2, r2, net.P[res.prefix + ".norm2.weight"], net.P[res.prefix + ".norm2.bias"], res.norm2.groups,
                         tab.slices[name].start))
    return taps


def channel_stats(model, noise_sched, images: torch.Tensor, *, batch: int, timesteps: Optional[torch.Tensor] = None,
                  noise: Optional[torch.Tensor] = None, seed: int = 0, trigger: Optional[torch.Tensor] = None, act: str = "silu_gn") -> ChannelStats:
    """Per-channel statistics of the hidden activation of every ResnetBlock over `images` ([N, C, H, W] f32 in the model's value range), `batch`
    at a time (the last batch may be shorter).  Per batch k: x_t = LossFn.get_inputs_targets(x0, R, t, eps) with R = 0 (clean inputs) or
    R = trigger ([C, H, W], added to every image as the attack's poison image is -- what `anp._Passes.inputs` forms with R = 0), then a no-grad
    save=True forward and ONE statistics launch over its tape into pass k's slot of a [passes, n_channels, 2] device buffer.  The tape is
    dropped before the next batch; the buffer is read once at the end and the passes are added in float64.

    timesteps: None -- torch.randint(0, T, (passes, batch)) from a CPU Generator(seed + 1), `learn_neuron_mask`'s draw; or an integer
    [passes, batch] tensor.  noise: None -- per pass from the device Philox stream of `seed`, as `learn_neuron_mask` draws it; or a
    [passes, batch, C, H, W] tensor (a short last batch uses the leading rows).  act: "silu_gn" -- silu(norm2(h1)), the quantity Fine-Pruning
    ranks; "raw" -- h1 itself.  model: a UNet2DModel with a VP-type scheduler, or an LDMPipeline (noise_sched may be None; images are latents or
    pixel images, the trigger, timesteps and noise are the latent UNet's).  The model's weights are never written."""
    what = "channel_stats"
    if act not in ACTS:
        raise ValueError(f"{what}: act must be one of {ACTS}, got {act!r}")
    _check_count(what, "batch", batch)
    net, fam = _family(what, model, noise_sched, images)
    _check_f16(what, net)
    shape = _shape(net)
    anp._check_clean(what, images, fam.clean_shape or shape)
    N = int(images.shape[0])
    passes = (N + batch - 1) // batch
    if trigger is not None:
        _check_trigger(what, trigger, shape)
    if timesteps is not None:
        if not torch.is_tensor(timesteps) or tuple(timesteps.shape) != (passes, batch) or timesteps.is_floating_point():
            raise ValueError(f"{what}: timesteps must be None or an integer [passes, batch] = {(passes, batch)} tensor")
        if int(timesteps.min()) < 0 or int(timesteps.max()) >= fam.T_train:
            raise ValueError(f"{what}: timesteps outside the scheduler's [0, {fam.T_train})")
    else:
        timesteps = torch.randint(0, fam.T_train, (passes, batch), generator=torch.Generator().manual_seed(int(seed) + 1))
    if noise is not None and (not torch.is_tensor(noise) or tuple(noise.shape) != (passes, batch) + shape):
        raise ValueError(f"{what}: noise must be None or a [passes, batch, C, H, W] = {(passes, batch) + shape} tensor")
    tab = activation_table(net)

    from . import lib
    lib.require_device()                                   # VillanHipError without an MI355X: there is no fallback
    dev = net.device
    if fam.prepare is not None:
        images = fam.prepare(images, batch)
    data = images.detach().to(dev, torch.float32).contiguous()
    timesteps = timesteps.to(dev, torch.int64)
    R_full = torch.zeros((batch,) + shape, device=dev, dtype=torch.float32)
    if trigger is not None:
        R_full += trigger.detach().to(dev, torch.float32)
    eps_buf = torch.empty((batch,) + shape, device=dev, dtype=torch.float32)
    per_iter = (eps_buf.numel() + 3) // 4
    out = torch.zeros((passes, tab.n_channels, 2), device=dev, dtype=torch.float32)
    count = {name: 0 for name in tab.names}
    keep: list = []                                        # job tables and workspaces: alive until the one read below
    with torch.no_grad():
        for k in range(passes):
            x0 = data[k * batch:(k + 1) * batch]
            b = int(x0.shape[0])
            eps = _noise_of(what, noise, k, eps_buf, seed, per_iter, dev)[:b]
            t = timesteps[k, :b].contiguous()
            x_t, _ = fam.loss.get_inputs_targets(x0, R_full[:b], t, eps)
            tm, _ = fam.call(t)
            _, st = net._run_forward(x_t.contiguous(), tm.to(torch.float32).contiguous(), save=True)
            taps = _taps(net, st, tab, act)
            ops.channel_stats(taps, out[k], act, keep=keep)
            for name, tp in zip(tab.names, taps):
                count[name] += tp[0].numel() // tp[0].shape[1]
            del st, taps                                   # (the launch is queued behind the forward on the same stream: the allocator may reuse)
    host = out.cpu().to(torch.float64).sum(dim=0).numpy()   # the one read: the passes added in float64
    keep.clear()
    return ChannelStats(table=tab, count=count, sum=host[:, 0].copy(), sumsq=host[:, 1].copy(), act=act, batch=batch, n_images=N, seed=int(seed),
                        triggered=trigger is not None)


# --------------------------------------------------------------------------------------------------------------------------------- scores
def _as_dict(tab: ActivationTable, v: np.ndarray) -> Dict[str, torch.Tensor]:
    return {name: torch.from_numpy(np.ascontiguousarray(v[sl])).to(torch.float32) for name, sl in tab.slices.items()}


def dormancy_scores(stats: ChannelStats) -> Dict[str, torch.Tensor]:
    """weight name -> the root mean square of each channel's activation; the smallest value is the most dormant channel.  Fine-Pruning ranks
    ReLU channels by their mean activation, which is non-negative; SiLU is signed (a channel can be busy around a mean of zero), so the RMS
    plays here the role the mean plays for ReLU."""
    return _as_dict(stats.table, stats.rms())


def sensitivity_scores(clean: ChannelStats, triggered: ChannelStats, eps: float = 1e-6) -> Dict[str, torch.Tensor]:
    """weight name -> -|mean_trig - mean_clean| / sqrt(var_clean + eps) per channel: negated, so that the smallest score is the most
    trigger-sensitive channel and the dict goes straight into `prune_neurons(..., fraction=)` and `pruning_curve(..., fractions=)`.  The two
    statistics must share a table, the counts and the activation; ValueError otherwise."""
    if clean.table.names != triggered.table.names or clean.table.n_channels != triggered.table.n_channels or \
            {k: (s.start, s.stop) for k, s in clean.table.slices.items()} != {k: (s.start, s.stop) for k, s in triggered.table.slices.items()}:
        raise ValueError("sensitivity_scores: the two statistics were taken over different tables")
    if clean.count != triggered.count:
        raise ValueError("sensitivity_scores: the two statistics were taken over different counts (images x pixels per channel)")
    if clean.act != triggered.act:
        raise ValueError(f"sensitivity_scores: the two statistics are of different activations ({clean.act!r}, {triggered.act!r})")
    if not eps > 0.0:
        raise ValueError(f"sensitivity_scores: eps must be positive, got {eps!r}")
    s = -np.abs(triggered.mean() - clean.mean()) / np.sqrt(clean.var() + float(eps))
    return _as_dict(clean.table, s)


# ----------------------------------------------------------------------------------------------------------------------------------- mask
@dataclass
class PruneMask:
    """keep: a 0/1 f32 vector over `anp.neuron_table(model, "all")` (0: the row is pruned and a masked fine-tune holds it at zero); pruned:
    weight name -> rows pruned, for the layers that have any."""
    keep: torch.Tensor
    pruned: Dict[str, int]

    @property
    def n_pruned(self) -> int:
        return int((self.keep == 0).sum())

    def save(self, path: str) -> str:
        """Writes `prune_mask.pt` (into `path` if that is a directory)."""
        if os.path.isdir(path):
            path = os.path.join(path, MASK_FILE)
        torch.save({"keep": self.keep.detach().to("cpu", torch.float32).contiguous(), "pruned": dict(self.pruned)}, path)
        return path

    @classmethod
    def load(cls, path: str) -> "PruneMask":
        if os.path.isdir(path):
            path = os.path.join(path, MASK_FILE)
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or "keep" not in d or not torch.is_tensor(d["keep"]) or d["keep"].dim() != 1:
            raise ValueError(f"PruneMask.load: {path} holds no prune mask")
        keep = d["keep"].to(torch.float32)
        if not bool(((keep == 0) | (keep == 1)).all()):
            raise ValueError(f"PruneMask.load: {path}: keep must hold zeros and ones")
        return cls(keep=keep, pruned={str(k): int(v) for k, v in d.get("pruned", {}).items()})

    @classmethod
    def from_model(cls, model, names=None) -> "PruneMask":
        """The mask that marks the rows of `names` (default: every layer of the "all" table) that are exactly zero in `model` (+0 or -0 in
        every float)."""
        net = _unet_of("PruneMask.from_model", model)
        full = anp.neuron_table(net, "all")
        names = list(full.slices) if names is None else list(names)
        keep = torch.ones(full.n_neurons, dtype=torch.float32)
        pruned = {}
        for name in names:
            if name not in full.slices:
                raise ValueError(f"PruneMask.from_model: {name} is no neuron layer of this {type(net).__name__}")
            w = net.P[name].detach().to("cpu")
            zero = (w.reshape(w.shape[0], -1) == 0).all(dim=1)
            keep[full.slices[name]][zero] = 0.0
            if int(zero.sum()):
                pruned[name] = int(zero.sum())
        return cls(keep=keep, pruned=pruned)


def fine_prune(model, scores, *, fraction: Optional[float] = None, threshold: Optional[float] = None) -> PruneMask:
    """`anp.prune_neurons(model, scores, ...)` -- the floor(fraction * n) smallest scores of the scored layers, or every score below
    `threshold` -- and the mask of exactly the rows it zeroed.  A selection that would empty a layer raises ValueError before anything is
    written.  Plain torch writes: works on a device="cpu" model."""
    net = _unet_of("fine_prune", model)
    full, dropped, picks = anp._selection("fine_prune", net, scores, threshold=threshold, fraction=fraction)     # every check, nothing written
    counts = anp.prune_neurons(net, scores, threshold=threshold, fraction=fraction)
    keep = torch.ones(full.n_neurons, dtype=torch.float32)
    keep[dropped] = 0.0
    return PruneMask(keep=keep, pruned={k: v for k, v in counts.items() if v})
