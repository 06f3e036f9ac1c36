"""LoRA (Hu et al., ICLR 2022) fine-tuning on the HIP path: the rank-constrained form of the backdoor fine-tune, the way the reference delivers its
Stable Diffusion backdoor (`--use_lora --lora_r 4`, `LoRAAttnProcessor` on the attention projections).  Every adapted weight tensor, viewed as
[M rows, L = numel / M], becomes

      W = W0 + s * B A,        A [r, L],  B [M, r],  s = alpha / r,

with W0 frozen and only (A, B) trained.  For a convolution this is peft's / diffusers' conv LoRA: a k x k down-convolution to r channels followed by
a 1 x 1 up-convolution.  Every parameter is a view of one flat f32 buffer (`flatnet`), so, as with adversarial neuron pruning (`anp`), the
adapted network is "write the merged weights into `flat_param`, run the ordinary forward and backward", and the chain rule is read off the
ordinary weight gradient G in `flat_grad`:

      dL/dB = s * G A^T,       dL/dA = s * B^T G.

Two kernels do it, each ONE launch for the whole network over an adapter table built once on the host (`adapter_table`): `vd_lora_merge` and
`vd_lora_grad`.  No convolution, GroupNorm or attention kernel is touched, and by default (backward="full") the backward still forms every weight
gradient.  backward="adapted" (`BackwardRoute`) routes every weight gradient of `UNet2DModel`'s explicit backward instead: a tensor without an
adapter gets none (nor its bias and GroupNorm sums), an adapted 1x1 layer gets its (dA, dB) straight from the activations (`vd_lora_act_grad`),
and only the other adapted layers still form G in `flat_grad` for `vd_lora_grad`.

The adapter lives in one flat f32 buffer per network (per job A, then B, every piece at a multiple of 4 floats, padding zero), its gradient in a
mirror of it, so the global-norm kernel and the Adam kernel serve the whole adapter in one launch each.  Single process; one rank for all layers.
"""
from __future__ import annotations

import bisect
import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import ops

__all__ = ["LoRAConfig", "AdapterTable", "adapter_table", "LoRAAdapter", "LoRAAdam", "TARGETS", "MAX_RANK", "BACKWARDS", "backward_routes",
           "BackwardRoute"]

TARGETS = ("attn", "conv", "all")
BACKWARDS = ("full", "adapted")
MAX_RANK = 32
_ATTN = re.compile(r"(^|\.)attentions\.\d+\.(to_q|to_k|to_v|to_out\.0)\.weight$")
_DIRECT = re.compile(r"(^|\.)(attentions\.\d+\.(to_q|to_k|to_v|to_out\.0)|conv_shortcut)\.weight$")
_TEMB = re.compile(r"(^time_embedding\.linear_[12]|\.time_emb_proj)\.weight$")
TILE = 256                                               # columns of a column workgroup of vd_lora_grad


@dataclass(frozen=True)
class LoRAConfig:
    """r: the rank, 1 .. 32, one for every layer.  alpha: None means alpha = r (s = 1, diffusers' `LoRAAttnProcessor` default).  target: "attn" --
    `*.attentions.*.{to_q,to_k,to_v,to_out.0}.weight`, the reference's choice; "conv" -- every 4-d `*.weight`; "all" -- every parameter with at
    least 2 dimensions.  seed: of the host draw of A."""
    r: int
    alpha: Optional[float] = None
    target: str = "attn"
    seed: int = 0

    def __post_init__(self):
        if not isinstance(self.r, int) or isinstance(self.r, bool) or not 1 <= self.r <= MAX_RANK:
            raise ValueError(f"LoRAConfig: r must be an int in [1, {MAX_RANK}], got {self.r!r}")
        if self.target not in TARGETS:
            raise ValueError(f"LoRAConfig: target must be one of {TARGETS}, got {self.target!r}")
        if self.alpha is not None and not (isinstance(self.alpha, (int, float)) and not isinstance(self.alpha, bool)
                                           and math.isfinite(self.alpha) and self.alpha > 0):
            raise ValueError(f"LoRAConfig: alpha must be None or a positive finite number, got {self.alpha!r}")
        if not isinstance(self.seed, int) or isinstance(self.seed, bool):
            raise ValueError(f"LoRAConfig: seed must be an int, got {self.seed!r}")

    @property
    def lora_alpha(self) -> float:
        return float(self.r if self.alpha is None else self.alpha)

    @property
    def s(self) -> float:
        return self.lora_alpha / self.r

    def to_dict(self) -> dict:
        return {"r": self.r, "alpha": self.alpha, "target": self.target, "seed": self.seed}


# ----------------------------------------------------------------------------------------------------------------------------- the adapter table
@dataclass
class AdapterTable:
    """jobs: one (weight offset in floats, rows M, row length L, offset of A, offset of B, first row workgroup, first column workgroup) per adapted
    weight tensor -- the rows of the device table of vd_lora_merge / vd_lora_grad, where a job owns ceil(M / 4) row workgroups and ceil(L / 256)
    column workgroups.  slices: the weight's dotted name -> (slice of A [r, L], slice of B [M, r]) in the adapter buffer (jobs are in the order of
    this dict).  numel: floats of the adapter buffer (padding included).  skipped: selected layers with min(M, L) <= r, which get no adapter."""
    jobs: List[Tuple[int, int, int, int, int, int, int]]
    slices: Dict[str, Tuple[slice, slice]]
    numel: int
    r: int
    s: float = 1.0
    skipped: List[str] = field(default_factory=list)
    shapes: Dict[str, Tuple[int, ...]] = field(default_factory=dict)
    target: Optional[str] = None
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        if not self.jobs:
            raise ValueError("adapter table: no jobs")
        if not isinstance(self.r, int) or not 1 <= self.r <= MAX_RANK:
            raise ValueError(f"adapter table: the rank must lie in [1, {MAX_RANK}], got {self.r!r}")
        r, rb, cb, pieces = self.r, 0, 0, []
        for k, (off, rows, ln, aoff, boff, b0, c0) in enumerate(self.jobs):
            if off < 0 or rows < 1 or ln < 1 or aoff < 0 or boff < 0 or aoff % 4 or boff % 4 or b0 != rb or c0 != cb:
                raise ValueError(f"adapter table: job {k} = {(off, rows, ln, aoff, boff, b0, c0)} (expected first row workgroup {rb}, first "
                                 f"column workgroup {cb}, A and B at multiples of 4 floats)")
            pieces += [(aoff, aoff + r * ln), (boff, boff + rows * r)]
            rb += (rows + 3) // 4
            cb += (ln + TILE - 1) // TILE
        pieces.sort()
        if any(a[1] > b[0] for a, b in zip(pieces, pieces[1:])) or pieces[-1][1] > self.numel:
            raise ValueError(f"adapter table: the pieces of the adapter buffer overlap or leave its {self.numel} floats")
        self.n_jobs, self.row_blocks, self.col_blocks = len(self.jobs), rb, cb
        self.weight_floats = sum(j[1] * j[2] for j in self.jobs)
        self.adapter_floats = sum(r * (j[1] + j[2]) for j in self.jobs)          # without the padding
        self.extent = max(j[0] + j[1] * j[2] for j in self.jobs)                 # floats a flat weight buffer must hold

    def device_table(self, device) -> torch.Tensor:
        """The [n_jobs, 7] int64 table on `device`, uploaded once."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = ops.upload_table(torch.tensor(self.jobs, dtype=torch.int64), device)
        return self._dev[key]

    def padding_mask(self) -> torch.Tensor:
        """[numel] bool on the host: True where the adapter buffer holds padding."""
        pad = torch.ones(self.numel, dtype=torch.bool)
        for a, b in self.slices.values():
            pad[a] = False
            pad[b] = False
        return pad


def _selected(name: str, shape, target: str) -> bool:
    if target == "attn":
        return len(shape) >= 2 and _ATTN.search(name) is not None
    if target == "conv":
        return len(shape) == 4 and name.endswith(".weight")
    return len(shape) >= 2


def adapter_table(model, cfg: LoRAConfig) -> AdapterTable:
    """The adapted layers of `model` (any flat-parameter network with a gradient buffer; pure host code, a device="cpu" model will do), in layout
    order.  A selected layer with min(M, L) <= r gets no adapter and is listed in `skipped` (r = 4: `conv_out`, NCSN++'s 3-row / 3-float
    `skip_conv` layers).  1-d parameters are never layers; biases and GroupNorm parameters stay frozen (peft bias="none")."""
    if not isinstance(cfg, LoRAConfig):
        raise TypeError(f"adapter_table: cfg must be a LoRAConfig, got {type(cfg).__name__}")
    if not hasattr(model, "_layout") or not hasattr(model, "flat_grad") or not torch.is_tensor(getattr(model, "flat_grad", None)):
        raise TypeError(f"adapter_table needs a flat-parameter network with a gradient buffer, got {type(model).__name__}")
    r = cfg.r
    jobs, slices, shapes, skipped, cursor, rb, cb = [], {}, {}, [], 0, 0, 0
    for name, shape, _ in model._layout:
        if not _selected(name, shape, cfg.target):
            continue
        off, n, _ = model._offs[name]
        M = int(shape[0])
        L = n // M
        if min(M, L) <= r:
            skipped.append(name)
            continue
        aoff = cursor
        boff = aoff + (r * L + 3) // 4 * 4
        cursor = boff + (M * r + 3) // 4 * 4
        jobs.append((int(off), M, L, aoff, boff, rb, cb))
        slices[name] = (slice(aoff, aoff + r * L), slice(boff, boff + M * r))
        shapes[name] = tuple(int(d) for d in shape)
        rb += (M + 3) // 4
        cb += (L + TILE - 1) // TILE
    if not jobs:
        raise ValueError(f"adapter_table: {type(model).__name__} has no layer for target={cfg.target!r} at rank {r}")
    return AdapterTable(jobs, slices, cursor, r, cfg.s, skipped, shapes, cfg.target)


def _peft_shapes(shape, r):
    """(lora_A.weight shape, lora_B.weight shape) of a layer of `shape`, as peft lays them out."""
    if len(shape) == 4:
        return (r,) + tuple(shape[1:]), (shape[0], r, 1, 1)
    return (r, int(math.prod(shape[1:]))), (shape[0], r)


def _layer(name: str) -> str:
    return name[:-len(".weight")] if name.endswith(".weight") else name


def _target_modules(tab: AdapterTable) -> List[str]:
    """peft's `target_modules`: the distinct module names (last path component; `to_out.0` keeps its index) of the adapted layers."""
    return sorted({"to_out.0" if _layer(n).endswith(".to_out.0") else _layer(n).rsplit(".", 1)[-1] for n in tab.slices})


# ----------------------------------------------------------------------------------------------------------------------- the adapted backward
def _check_backward(model, backward: str):
    """The refusals of backward=..., before the device is touched."""
    if backward not in BACKWARDS:
        raise ValueError(f"LoRA: backward must be one of {BACKWARDS}, got {backward!r}")
    if backward == "adapted" and not getattr(model, "_lora_adapted_backward", False):
        raise NotImplementedError(f"LoRA backward='adapted' is not built for {type(model).__name__} (its weight gradients bypass UNet2DModel.wgrad); "
                                  f"use backward='full'")


def backward_routes(model, tab: AdapterTable) -> dict:
    """How backward="adapted" treats the jobs of `tab` on `model` (a UNet2DModel; pure host code): {"direct": names whose (dA, dB) come straight
    from the activations -- the 1x1 layers whose weight gradient UNet2DModel queues as a plain product of two f32 images: the attention projections
    and `conv_shortcut`; "full": the other adapted layers, which keep G in flat_grad and vd_lora_grad; "temb": whether the time-embedding MLP's
    backward still runs (one of its weights has an adapter)}.  Every other parameter of the network gets no gradient at all."""
    direct = [n for n in tab.slices if _DIRECT.search(n)]
    full = [n for n in tab.slices if not _DIRECT.search(n)]
    return {"direct": direct, "full": full, "temb": any(_TEMB.search(n) for n in full)}


class BackwardRoute:
    """What `UNet2DModel.lora_route` holds in adapted mode: the routing of `backward_routes` by flat-gradient offset, the queue of direct jobs of
    the running backward pass and the launch that serves them (`flush`, called from the network's weight-gradient flush, on its side stream when
    there is one).  Direct jobs ACCUMULATE into `gab` (the adapter's gradient buffer): `LoRAAdapter.zero_grad` clears it."""

    def __init__(self, model, tab: AdapterTable, ab: torch.Tensor, gab: torch.Tensor):
        routes = backward_routes(model, tab)
        self.table, self.ab, self.gab, self.temb = tab, ab, gab, routes["temb"]
        by_name = dict(zip(tab.slices, tab.jobs))
        self.direct = {by_name[n][0]: by_name[n] for n in routes["direct"]}          # weight offset -> job
        self.direct_offs = sorted(self.direct)
        self.full_offs = {by_name[n][0] for n in routes["full"]}
        self.full_names = routes["full"]
        self.full_table = self._sub_table(tab, routes["full"]) if routes["full"] else None
        self.jobs: list = []                                                          # (job row, dy, x) of the running pass
        self._plans: Dict[tuple, "ops.ActPlan"] = {}
        self.ws: Optional[torch.Tensor] = None

    @staticmethod
    def _sub_table(tab: AdapterTable, names) -> AdapterTable:
        """The jobs of `names` as a table of their own over the SAME adapter buffer (vd_lora_grad's workgroup columns renumbered)."""
        by_name = dict(zip(tab.slices, tab.jobs))
        jobs, rb, cb = [], 0, 0
        for n in names:
            off, M, L, aoff, boff, _, _ = by_name[n]
            jobs.append((off, M, L, aoff, boff, rb, cb))
            rb += (M + 3) // 4
            cb += (L + TILE - 1) // TILE
        return AdapterTable(jobs, {n: tab.slices[n] for n in names}, tab.numel, tab.r, tab.s, [], {n: tab.shapes[n] for n in names}, tab.target)

    def wants(self, net, dw2d) -> bool:
        """Does the gradient view `dw2d` hold an adapted tensor (full or direct)?"""
        off = (dw2d.data_ptr() - net.flat_grad.data_ptr()) // 4
        if off in self.full_offs:
            return True
        return bisect.bisect_left(self.direct_offs, off) < bisect.bisect_left(self.direct_offs, off + dw2d.numel())

    def take(self, net, dy, x, dw2d, mode) -> bool:
        """Route one weight gradient of the running backward pass.  True: nothing more to do for it (no adapter: skipped; direct: queued here).
        False: the full route -- the caller forms G in flat_grad as ever."""
        from .lib import B_PLAIN
        off = (dw2d.data_ptr() - net.flat_grad.data_ptr()) // 4
        if off in self.full_offs:
            return False
        rows, ln = dw2d.shape
        lo = bisect.bisect_left(self.direct_offs, off)
        hi = bisect.bisect_left(self.direct_offs, off + rows * ln)
        for joff in self.direct_offs[lo:hi]:                                          # (the fused q, k, v gradient holds three adapters)
            _, M, L, aoff, boff, _, _ = self.direct[joff]
            if (mode != B_PLAIN or isinstance(dy, ops.PreSplit) or isinstance(x, ops.PreSplit) or L != ln or (joff - off) % ln
                    or (joff - off) // ln + M > rows):
                raise RuntimeError(f"LoRA adapted backward: the layer at flat offset {joff} is routed direct but its weight gradient is no plain "
                                   f"product of two f32 images (mode {mode}, [{rows}, {ln}] at {off})")
            Bn, Cy, H, W, dbs = ops._img(dy)
            Bx, Cx, Hx, Wx, xbs = ops._img(x)
            assert (Bx, Cx, Hx * Wx, Cy) == (Bn, L, H * W, rows), (x.shape, dy.shape, dw2d.shape)
            m0 = (joff - off) // ln
            self.jobs.append(((dy.data_ptr() + 4 * m0 * H * W, dbs, x.data_ptr(), xbs, Bn, M, L, H * W, aoff, boff), dy, x))
        return True

    def flush(self, device):
        """One vd_lora_act_grad launch over the direct jobs queued so far (on the current stream); -> the jobs, whose operands the caller keeps
        referenced until that stream is joined."""
        jobs, self.jobs = self.jobs, []
        if not jobs:
            return jobs
        key = tuple(j[0] for j in jobs)
        plan = self._plans.get(key)
        if plan is None:                                                              # steady-state training repeats the addresses
            if len(self._plans) > 64:
                self._plans.clear()
            plan = self._plans[key] = ops.lora_act_plan(key, self.table.r)
        if self.ws is None or self.ws.numel() < plan.ws_floats:
            self.ws = torch.empty(max(plan.ws_floats, 1 << 20), device=device, dtype=torch.float32)
        ops.lora_act_grad(plan, self.ab, self.gab, self.table.s, self.ws, accumulate=True)
        return jobs


# ------------------------------------------------------------------------------------------------------------------------------------ the adapter
class LoRAAdapter:
    """The adapter of one network: `base` (a clone of `flat_param` at construction: W0 and every frozen parameter), `param` and `grad` (the flat
    adapter buffers) and the table.  A ~ U(+-1/sqrt(L)) (torch's kaiming_uniform_(a=sqrt(5)) on [r, L]) drawn on the host in table order from
    cfg.seed, B = 0: the adapted network starts as the base.  As a context manager it un-merges on exit, also after an exception.

    backward: "full" -- the network forms every weight gradient and `backward_()` reads (dA, dB) off flat_grad; "adapted" -- the network's
    `lora_route` is set (see `BackwardRoute`): direct layers accumulate into `grad` during each backward pass, `backward_()` writes the slots of
    the full-route layers from flat_grad and leaves the others alone, so `zero_grad()` belongs where `model.zero_grad()` is called.  Either way
    `grad` is the whole adapter gradient after `loss.backward(); adapter.backward_()`.  The mode belongs to the run: no state records it.
    `detach()` takes the route off the network again."""

    def __init__(self, model, cfg: LoRAConfig, backward: str = "full"):
        _check_backward(model, backward)
        self.table = adapter_table(model, cfg)                # every check before the device is touched
        self.model, self.cfg, self.backward = model, cfg, backward
        host = self._init_host(self.table, cfg)
        if model.device.type != "cpu":
            from . import lib
            lib.require_device()
        dev = model.flat_param.device
        self.base = model.flat_param.detach().clone()
        self.param = host.to(dev)
        self.grad = torch.zeros_like(self.param)
        self.route = None
        if backward == "adapted":
            self.route = model.lora_route = BackwardRoute(model, self.table, self.param, self.grad)

    def detach(self):
        """Take this adapter's route off the network: its backward forms every weight gradient again."""
        if self.route is not None and getattr(self.model, "lora_route", None) is self.route:
            self.model.lora_route = None

    def zero_grad(self):
        """grad <- 0 (one launch).  Adapted mode accumulates the direct layers' gradients into it during every backward pass."""
        if self.grad.device.type == "cpu":
            self.grad.zero_()
        else:
            ops.scale_(self.grad, 0.0)

    @staticmethod
    def _init_host(tab: AdapterTable, cfg: LoRAConfig) -> torch.Tensor:
        gen = torch.Generator().manual_seed(int(cfg.seed))
        host = torch.zeros(tab.numel, dtype=torch.float32)
        for (_, M, L, *_), (a, _) in zip(tab.jobs, tab.slices.values()):
            host[a] = (torch.rand(cfg.r * L, generator=gen) * 2 - 1) * (1.0 / math.sqrt(L))
        return host

    # -------------------------------------------------------------------------------------------- device passes
    def _weights_written(self):
        ops.WEIGHTS_EPOCH += 1                                # raw-pointer writes: no version counter sees them
        self.model.weights_changed()

    def merge_(self):
        """flat_param <- base + s * B A on the adapted layers (one launch); every other float of flat_param is left as it is."""
        ops.lora_merge(self.base, self.model.flat_param, self.table, self.param)
        self._weights_written()

    def unmerge_(self):
        """flat_param <- base, bit for bit."""
        with torch.no_grad():
            self.model.flat_param.copy_(self.base)
        self._weights_written()

    def backward_(self, accumulate: bool = False):
        """grad (+)= the gradient of (A, B) from the weight gradients in model.flat_grad (one launch).  Adapted mode: over the full-route layers
        only (no launch when there is none); the direct layers' slots already hold their gradient."""
        if self.route is None:
            ops.lora_grad(self.model.flat_grad, self.table, self.param, self.grad, accumulate=accumulate)
        elif self.route.full_table is not None:
            ops.lora_grad(self.model.flat_grad, self.route.full_table, self.param, self.grad, accumulate=accumulate)

    def __enter__(self):
        self.merge_()
        return self

    def __exit__(self, *exc):
        self.unmerge_()
        return False

    # -------------------------------------------------------------------------------------------- state
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """peft-shaped host tensors: `<layer>.lora_A.weight` [r, Cin, kh, kw] or [r, in], `<layer>.lora_B.weight` [M, r, 1, 1] or [M, r]."""
        host, r, sd = self.param.detach().cpu(), self.cfg.r, {}
        for name, (a, b) in self.table.slices.items():
            sa, sb = _peft_shapes(self.table.shapes[name], r)
            layer = _layer(name)
            sd[layer + ".lora_A.weight"] = host[a].clone().view(sa)
            sd[layer + ".lora_B.weight"] = host[b].clone().view(sb)
        return sd

    @staticmethod
    def _wanted(tab: AdapterTable) -> Dict[str, Tuple[slice, Tuple[int, ...]]]:
        """key -> (slice of the adapter buffer, peft shape) for every tensor of an adapter laid out by `tab`; ValueError-free, host only."""
        want = {}
        for name, (a, b) in tab.slices.items():
            sa, sb = _peft_shapes(tab.shapes[name], tab.r)
            want[_layer(name) + ".lora_A.weight"] = (a, sa)
            want[_layer(name) + ".lora_B.weight"] = (b, sb)
        return want

    @classmethod
    def _check_state(cls, tab: AdapterTable, sd) -> Dict[str, Tuple[slice, Tuple[int, ...]]]:
        """Every layer of the table must be in `sd` with its shape, and nothing else: ValueError naming the first mismatch."""
        want = cls._wanted(tab)
        for key, (_, shape) in want.items():
            if key not in sd:
                raise ValueError(f"LoRA adapter: the state holds no {key} (this network adapts it at rank {tab.r}, target {tab.target!r})")
            if tuple(sd[key].shape) != tuple(shape):
                raise ValueError(f"LoRA adapter: {key} is {tuple(sd[key].shape)} in the state, {tuple(shape)} on this network")
        extra = [k for k in sd if k not in want]
        if extra:
            raise ValueError(f"LoRA adapter: the state holds {extra[0]}, which is no adapted layer of this network ({len(extra)} such keys)")
        return want

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Every layer of this adapter must be there with its shape, and nothing else: ValueError naming the first mismatch, before a float is
        written."""
        want = self._check_state(self.table, sd)
        host = torch.zeros(self.table.numel, dtype=torch.float32)
        for key, (sl, _) in want.items():
            host[sl] = sd[key].detach().to("cpu", torch.float32).reshape(-1)
        self.param.copy_(host)

    def train_state(self) -> Dict:
        """What a bit-exact resume needs beyond the optimiser's moments: the adapter, the base it sits on and its configuration."""
        return {"param": self.param, "base": self.base, "config": self.cfg.to_dict()}

    def load_train_state(self, lo: Dict):
        """Inverse of `train_state`: adapter and base are taken over and flat_param rewritten from them (frozen floats from the base, adapted
        layers from the merge).  ValueError where the state belongs to another adapter layout."""
        cfg = LoRAConfig(**lo["config"])
        if (cfg.r, cfg.lora_alpha, cfg.target) != (self.cfg.r, self.cfg.lora_alpha, self.cfg.target):
            raise ValueError(f"load_state_dict: the state's adapter is {cfg}, this trainer's {self.cfg}")
        if lo["param"].numel() != self.param.numel() or lo["base"].numel() != self.base.numel():
            raise ValueError(f"load_state_dict: the state's adapter holds {lo['param'].numel()} floats on a base of {lo['base'].numel()}, this "
                             f"trainer's {self.param.numel()} on {self.base.numel()}")
        self.cfg = cfg
        self.param.copy_(lo["param"])
        self.base.copy_(lo["base"])
        self.unmerge_()
        self.merge_()

    def save(self, directory: str):
        """`adapter_config.json` + `adapter_model.safetensors` in `directory` (peft's file names and key shapes; loading into peft is unverified)."""
        from safetensors.torch import save_file
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "adapter_config.json"), "w") as f:
            json.dump({"peft_type": "LORA", "r": self.cfg.r, "lora_alpha": self.cfg.lora_alpha, "target_modules": _target_modules(self.table),
                       "bias": "none", "target": self.cfg.target, "seed": self.cfg.seed,
                       "layers": [_layer(n) for n in self.table.slices]}, f, indent=2)
        save_file({k: v.contiguous() for k, v in self.state_dict().items()}, os.path.join(directory, "adapter_model.safetensors"))

    @staticmethod
    def read_config(directory: str) -> LoRAConfig:
        path = os.path.join(directory, "adapter_config.json")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{directory}: no adapter_config.json (not a LoRA adapter folder)")
        with open(path) as f:
            c = json.load(f)
        if c.get("peft_type") != "LORA" or c.get("bias", "none") != "none" or "target" not in c:
            raise ValueError(f"{path}: not an adapter written by LoRAAdapter.save (peft_type {c.get('peft_type')!r}, bias {c.get('bias')!r}, "
                             f"target {c.get('target')!r})")
        r, alpha = int(c["r"]), float(c["lora_alpha"])
        return LoRAConfig(r=r, alpha=None if alpha == r else alpha, target=c["target"], seed=int(c.get("seed", 0)))

    @classmethod
    def load(cls, model, directory: str) -> "LoRAAdapter":
        """The adapter of `directory` on `model`, which becomes its base (possibly another base than it was trained on).  A network whose adapted
        layers differ in name or shape raises ValueError naming the first mismatch."""
        from safetensors.torch import load_file
        cfg = cls.read_config(directory)
        sd = load_file(os.path.join(directory, "adapter_model.safetensors"))
        cls._check_state(adapter_table(model, cfg), sd)       # on the host, before the device is touched
        ad = cls(model, cfg)
        ad.load_state_dict(sd)
        return ad


# ---------------------------------------------------------------------------------------------------------------------------------- the optimiser
class LoRAAdam:
    """`trainer.FusedAdam`'s interface over the adapter only: torch.optim.Adam(betas=(0.9, 0.999), eps=1e-8) on (A, B) with the global-norm clip
    of the adapter gradient -- the trainable parameters, as `clip_grad_norm_` would see them.  One step: `vd_lora_grad` from the accumulated
    `flat_grad`, `vd_l2norm_sq` and `vd_adam_step` on the adapter buffers, `vd_lora_merge`.  The padding of the buffers has a zero gradient and
    zero moments, so Adam leaves it zero."""
    ema = None
    ema_cfg = None
    ema_step = 0

    def __init__(self, adapter: LoRAAdapter, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: Optional[float] = 1.0):
        self.adapter, self.model = adapter, adapter.model
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.exp_avg = torch.zeros_like(adapter.param)
        self.exp_avg_sq = torch.zeros_like(adapter.param)
        self.step_count = 0
        dev = adapter.param.device
        self._partial = torch.empty(1024, device=dev, dtype=torch.float32)
        self.grad_norm_sq = torch.zeros(1, device=dev, dtype=torch.float32)
        self.skipped = torch.zeros(1, device=dev, dtype=torch.int32)

    def step(self, lr: Optional[float] = None, grad_inv_scale: float = 1.0, need_norm: bool = False):
        ad = self.adapter
        self.step_count += 1
        ad.backward_()
        nsq = None
        if self.max_grad_norm is not None or need_norm:
            ops.l2norm_sq(ad.grad, self._partial, self.grad_norm_sq)
            nsq = self.grad_norm_sq
        max_norm = float(self.max_grad_norm if self.max_grad_norm is not None else 3.0e38)
        ops.adam_step(ad.param, ad.grad, self.exp_avg, self.exp_avg_sq, nsq, max_norm, grad_inv_scale, self.lr if lr is None else lr,
                      self.betas[0], self.betas[1], self.eps, self.step_count, skipped=self.skipped if nsq is not None else None, weights=False)
        ad.merge_()                                           # (bumps WEIGHTS_EPOCH: the network's weights are what changed)

    def grad_norm(self, grad_inv_scale: float = 1.0) -> float:
        """Global L2 norm of the adapter gradient of the last step -- synchronises; for logging/tests only."""
        return math.sqrt(float(self.grad_norm_sq)) * grad_inv_scale

    def state_dict(self) -> Dict:
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count, "lr": self.lr}

    def load_state_dict(self, sd: Dict):
        if "ema" in sd:
            raise ValueError("load_state_dict: the state holds an EMA shadow but this optimiser trains a LoRA adapter (no EMA with LoRA)")
        if sd["exp_avg"].numel() != self.exp_avg.numel():
            raise ValueError(f"load_state_dict: the state's moments hold {sd['exp_avg'].numel()} floats, this adapter {self.exp_avg.numel()} "
                             f"(a state of a full fine-tune, or of another adapter)")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])
        self.lr = float(sd.get("lr", self.lr))
