"""One optimiser step of the poisoned fine-tune loop (T1/T2 in SURVEY.md §8a; reference VillanDiffusion.py:1141-1176
plus the accelerate semantics of SURVEY Appendix B), one process per GPU.

* backward of micro-step k accumulates into the model's flat gradient buffer; the loss gradient is pre-divided by the
  gradient-accumulation count G inside the MSE kernel (``accelerator.backward``);
* on a sync step: ONE RCCL all-reduce (SUM) of the flat fp32 gradient bucket over xGMI (replaces nn.DataParallel's
  per-step parameter broadcast + gradient reduce, VillanDiffusion.py:440), then ONE l2-norm kernel and ONE fused
  clip + Adam kernel over the flat param/grad/m/v buffers (``clip_grad_norm_(…, 1.0)`` + ``torch.optim.Adam``);
  the 1/world averaging and the clip coefficient are folded into the Adam kernel's gradient scale;
* LR = base_lr * cosine-with-warmup(sync_step_count), advanced only on sync steps (accelerate's scheduler wrapper).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from dataclasses import asdict, dataclass
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist

from . import ops
from .anchor import AnchorConfig, check_anchor
from .schedulers import get_cosine_schedule_with_warmup_lambda


@dataclass
class EMAConfig:
    """The exponential moving average of the weights, with the parameters (and defaults) of diffusers' ``EMAModel``."""
    decay: float = 0.9999
    min_decay: float = 0.0
    update_after_step: int = 0
    use_ema_warmup: bool = False
    inv_gamma: float = 1.0
    power: float = 2 / 3


def ema_decay_at(k: int, cfg: EMAConfig) -> float:
    """diffusers ``EMAModel.get_decay`` for the k-th EMA update (k counts updates, the current one included), in Python doubles:
    n = max(0, k - update_after_step - 1); n <= 0 gives 0 (the shadow takes the parameters as they are); else (1 + n) / (10 + n), or
    1 - (1 + n / inv_gamma) ** -power with warm-up, clamped to [min_decay, decay]."""
    n = max(0, int(k) - int(cfg.update_after_step) - 1)
    if n <= 0:
        return 0.0
    d = 1.0 - (1.0 + n / cfg.inv_gamma) ** -cfg.power if cfg.use_ema_warmup else (1.0 + n) / (10.0 + n)
    return max(min(d, float(cfg.decay)), float(cfg.min_decay))


def ema_one_minus_decay(k: int, cfg: EMAConfig) -> float:
    """1 - ema_decay_at(k, cfg) as the C float the kernel receives."""
    return ctypes.c_float(1.0 - ema_decay_at(k, cfg)).value


SAM_MODES = ("sam", "asam", "neuron")


@dataclass
class SAMConfig:
    """Sharpness-aware minimisation: every optimiser step takes its gradient at w + e, e = rho * T^2 g / ||T g|| with g the gradient at w.
    mode "sam" (Foret et al. 2021): T = 1; "asam" (Kwon et al. 2021): T_i = |w_i| + eta; "neuron": one T per neuron of
    ``anp.neuron_table(model, layers)``, the root mean square of its weight row plus eta -- neurons with large weights are perturbed more, in the
    spirit of FT-SAM (Zhu et al. 2023), and only those weight rows are perturbed.  ``layers`` is read by "neuron" alone."""
    rho: float
    mode: str = "sam"
    eta: float = 0.01
    layers: str = "conv"

    def __post_init__(self):
        from .anp import LAYERS
        if isinstance(self.rho, bool) or not isinstance(self.rho, (int, float)) or not math.isfinite(self.rho) or self.rho <= 0:
            raise ValueError(f"SAMConfig: rho must be a positive finite number, got {self.rho!r}")
        if isinstance(self.eta, bool) or not isinstance(self.eta, (int, float)) or not math.isfinite(self.eta) or self.eta < 0:
            raise ValueError(f"SAMConfig: eta must be a finite number >= 0, got {self.eta!r}")
        if self.mode not in SAM_MODES:
            raise ValueError(f"SAMConfig: mode must be one of {SAM_MODES}, got {self.mode!r}")
        if self.layers not in LAYERS:
            raise ValueError(f"SAMConfig: layers must be one of {LAYERS}, got {self.layers!r}")


def check_sam(sam, grad_accum: int = 1, lora=None, graph_micro_step: Optional[bool] = None, world: int = 1, conv_math: Optional[str] = None):
    """What a SAM trainer is not built for, each refusal saying which; pure host code, shared by Trainer and the drivers' setup()."""
    if sam is None:
        return
    if not isinstance(sam, SAMConfig):
        raise TypeError(f"Trainer: sam must be a SAMConfig, got {type(sam).__name__}")
    if max(1, int(grad_accum)) > 1:
        raise ValueError(f"Trainer: sam with grad_accum={grad_accum} is not built (the second pass would have to replay the whole accumulation "
                         f"window at the perturbed weights); use grad_accum=1")
    if lora is not None:
        raise ValueError("Trainer: sam together with lora is not built (the perturbation belongs to the adapter, which SAM does not see)")
    if graph_micro_step:
        raise ValueError("Trainer: sam with graph_micro_step=True is not built (a SAM step runs its two passes eagerly)")
    if world > 1:
        raise NotImplementedError("Trainer: sam in a process group of more than one rank is not built (the first pass's gradient would need an "
                                  "all-reduce of its own)")
    if conv_math == "f16":
        raise NotImplementedError("Trainer: sam with conv_math='f16' is not built (an overflow in the first pass has no skip path)")


def check_keep_pruned(keep_pruned, lora=None, sam=None, world: int = 1):
    """What a masked fine-tune is not built with, each refusal saying which; pure host code, shared by Trainer and the drivers' setup()."""
    if keep_pruned is None:
        return
    from .actprune import PruneMask
    if not isinstance(keep_pruned, PruneMask):
        raise TypeError(f"Trainer: keep_pruned must be an actprune.PruneMask, got {type(keep_pruned).__name__}")
    if lora is not None:
        raise ValueError("Trainer: keep_pruned together with lora is not built (the merge W0 + s B A writes every row; the adapter would need "
                         "the mask on B)")
    if sam is not None:
        raise ValueError("Trainer: keep_pruned together with sam is not built (the first pass's gradient would perturb the pruned rows away "
                         "from zero for the second pass; it needs a mask launch between the passes)")
    if world > 1:
        raise NotImplementedError("Trainer: keep_pruned in a process group of more than one rank is not built (the mask launch would have to "
                                  "follow the bucketed all-reduce)")


class FusedAdam:
    """torch.optim.Adam(betas=(0.9, 0.999), eps=1e-8, weight_decay=0) on one flat buffer, with the global-norm clip
    fused in.  ``state_dict`` is flat too (exp_avg / exp_avg_sq / step).  With an ``EMAConfig`` the same launch keeps ``self.ema``, the
    exponential moving average of the parameters (a copy of them at construction), and ``self.ema_step`` counts its updates."""

    def __init__(self, model, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: Optional[float] = 1.0,
                 ema: Optional[EMAConfig] = None):
        self.model = model
        self.ema_cfg = ema
        self.ema = model.flat_param.detach().clone() if ema is not None else None
        self.ema_step = 0
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.exp_avg = torch.zeros_like(model.flat_param)
        self.exp_avg_sq = torch.zeros_like(model.flat_param)
        self.step_count = 0
        self._partial = torch.empty(1024, device=model.flat_param.device, dtype=torch.float32)
        self.grad_norm_sq = torch.zeros(1, device=model.flat_param.device, dtype=torch.float32)
        # steps the Adam kernel skipped because the gradient norm was not finite (device word, bumped by the kernel; read lazily by Trainer)
        self.skipped = torch.zeros(1, device=model.flat_param.device, dtype=torch.int32)

    def step(self, lr: Optional[float] = None, grad_inv_scale: float = 1.0, need_norm: bool = False):
        m = self.model
        self.step_count += 1
        nsq = None
        if self.max_grad_norm is not None or need_norm:          # need_norm: the overflow guard of the f16 mode reads it (no clipping: max_norm = inf)
            ops.l2norm_sq(m.flat_grad, self._partial, self.grad_norm_sq)
            nsq = self.grad_norm_sq
        max_norm = float(self.max_grad_norm if self.max_grad_norm is not None else 3.0e38)
        if self.ema is None:
            ops.adam_step(m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, nsq, max_norm, grad_inv_scale, self.lr if lr is None else lr,
                          self.betas[0], self.betas[1], self.eps, self.step_count, skipped=self.skipped if nsq is not None else None)
            return
        # a step the kernel skips leaves the shadow alone; Trainer.check_skipped takes it back out of ema_step, as out of step_count
        self.ema_step += 1
        ops.adam_ema_step(m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, self.ema, nsq, max_norm, grad_inv_scale,
                          self.lr if lr is None else lr, self.betas[0], self.betas[1], self.eps, self.step_count,
                          ema_one_minus_decay(self.ema_step, self.ema_cfg), skipped=self.skipped if nsq is not None else None)

    def grad_norm(self, grad_inv_scale: float = 1.0) -> float:
        """Global L2 norm of the (averaged) gradient of the last step -- synchronises; for logging/tests only."""
        return math.sqrt(float(self.grad_norm_sq)) * grad_inv_scale

    def state_dict(self) -> Dict:
        sd = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count, "lr": self.lr}
        if self.ema is not None:
            sd.update(ema=self.ema, ema_step=self.ema_step, ema_config=asdict(self.ema_cfg))
        return sd

    def load_state_dict(self, sd: Dict):
        """A state without a shadow loads into an optimiser without EMA, one with a shadow (its counter, its configuration) into an optimiser
        with EMA; either mismatch raises: the shadow cannot be made up, and dropping one silently would lose it at the next checkpoint."""
        if ("ema" in sd) != (self.ema is not None):
            raise ValueError("load_state_dict: the state " + ("holds" if "ema" in sd else "holds no") + " EMA shadow but this optimiser was built "
                             + ("without" if "ema" in sd else "with") + " EMA (FusedAdam / Trainer ema=...)")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])
        self.lr = float(sd.get("lr", self.lr))
        if self.ema is not None:
            self.ema.copy_(sd["ema"])
            self.ema_step = int(sd["ema_step"])
            self.ema_cfg = EMAConfig(**sd["ema_config"])


def allreduce_flat_grad(flat_grad: torch.Tensor, n_buckets: int = 4, even_alone: bool = False):
    """SUM all-reduce of the flat gradient in a few large buckets (RCCL over xGMI: ring all-reduce is per-link bound,
    so few large messages; backend "nccl" IS RCCL on ROCm, "gloo" in the CPU tests)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not even_alone):
        return
    n = flat_grad.numel()
    per = (n + n_buckets - 1) // n_buckets
    per = (per + 1023) // 1024 * 1024
    works = []
    for s in range(0, n, per):
        works.append(dist.all_reduce(flat_grad[s:min(n, s + per)], op=dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()


def shard_indices(n_items: int, epoch: int, rank: int, world: int, seed: int = 0, shuffle: bool = True) -> torch.Tensor:
    """DistributedSampler-style deterministic sharding: a seeded epoch permutation, padded to a multiple of `world`,
    rank r takes the contiguous slice r.  Poison flags travel with the sample index."""
    if shuffle:
        g = torch.Generator().manual_seed(seed + epoch)
        perm = torch.randperm(n_items, generator=g)
    else:
        perm = torch.arange(n_items)
    total = (n_items + world - 1) // world * world
    if total > n_items:
        perm = torch.cat([perm, perm[: total - n_items]])
    per = total // world
    return perm[rank * per:(rank + 1) * per]


_DEBUG = bool(__import__("os").environ.get("VD_GRAPH_DEBUG"))


class GraphedMicroStep:
    """q-sample -> UNet forward -> loss (+ its gradient) -> UNet backward of ONE micro-batch, captured once into a HIP graph per batch shape
    and replayed (BASELINE config #1: `--batch 4` with gradient accumulation 32, VillanDiffusion.py:287 -- a micro-step is ~470 launches of
    5-20 us kernels, so eager launch is host-bound: the GPU idles between them).  The graph calls the network's explicit launch sequences
    directly (no autograd tape inside the capture), accumulates into the flat gradient buffer like `loss.backward()` does and leaves the
    un-divided micro-batch loss in `self.loss`.  Static inputs: clean image, poison residual, noise, timesteps, and the poison flags of a shaped
    loss (LossFn snr_gamma / poison_weight / track_split: the shaped loss kernel is what the capture holds then).  Single-process VP / LDM
    training only (the bucketed all-reduce hooks of a multi-rank step fire from inside the backward pass and are not captured)."""

    def __init__(self, trainer, x0, R, noise, t, flags=None):
        import torch.cuda
        net, lf = trainer.model, trainer.loss_fn
        self.trainer, self.net = trainer, net
        dev = net.device
        self.x0, self.R, self.noise = (torch.zeros_like(v, device=dev, dtype=torch.float32) for v in (x0, R, noise))
        self.t = torch.zeros(t.shape, device=dev, dtype=torch.int64)
        self.tf = torch.zeros(t.shape, device=dev, dtype=torch.float32)
        self.loss = torch.zeros(1, device=dev, dtype=torch.float32)
        self.key = self._key()
        for buf, v in ((self.x0, x0), (self.R, R), (self.noise, noise), (self.t, t)):
            buf.copy_(v)
        self.flags = self.ws = None
        if getattr(lf, "shaped", False):                  # the shaped loss: static flags, and a workspace of this graph's own (its address is captured)
            self.flags = None if flags is None else flags.clone()
            self.ws = torch.empty(ops.loss_sample_plan(x0.shape[0], x0[0].numel())[2], device=dev, dtype=torch.float32)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        keep = net.flat_grad.clone()
        route = getattr(net, "lora_route", None)          # LoRA's adapted backward accumulates into the adapter's gradient buffer as well
        keep_ad = route.gab.clone() if route is not None else None
        with torch.cuda.stream(side):                     # warm-up off the capture: workspaces, job tables, packed operands, allocator pools
            for _ in range(2):
                self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if _DEBUG:
            print("[graph] warm-up done", flush=True)
        net.flat_grad.copy_(keep)                         # the warm-up passes accumulated gradients: undo
        if route is not None:
            route.gab.copy_(keep_ad)
        self._route_ws = route.ws if route is not None else None      # (the direct kernel's workspace: its address is baked into the capture)
        self._keep = (ops.gemm_ws_buffer(dev, 0), ops._WG_WS.get(dev), getattr(net, "_packed", None), net.wgrad_ws, getattr(net, "_packed16", None),
                      ops.gemm_ws_buffer(dev, ops.AUX_WS_SLOT))      # (the auxiliary stream's workspace: its address is baked into the capture too)
        self.graph = torch.cuda.CUDAGraph()
        ops.capture_begin(dev)                            # job tables built during the capture are uploaded right after it (ops.upload_table)
        try:
            with torch.cuda.graph(self.graph):
                self._body()
        finally:
            self._tables = ops.capture_end()              # device job tables the captured launches read: owned by this graph from now on
        self._last = (lf.last_sample_loss, lf.last_split) if self.ws is not None else None      # the capture's own outputs: every replay refills them
        if _DEBUG:
            torch.cuda.synchronize(dev)
            print(f"[graph] captured; {len(self._tables)} job tables", flush=True)

    def _key(self):
        n = self.net
        route = getattr(n, "lora_route", None)
        return (n.conv_math, n.wgrad_stream, n.group_wgrad, n.flat_param.data_ptr(), n.flat_grad.data_ptr(), self.trainer.loss_fn.grad_scale,
                None if route is None else (id(route), route.gab.data_ptr()), None if self.trainer._keep is None else self.trainer._keep.data_ptr(),      # the mask launch's operand
                getattr(self.trainer.loss_fn, "shaping", None))

    def valid(self) -> bool:
        dev = self.net.device
        return (self.key == self._key() and self._keep[0] is ops.gemm_ws_buffer(dev, 0) and self._keep[1] is ops._WG_WS.get(dev)
                and self._keep[3] is self.net.wgrad_ws and self._keep[5] is ops.gemm_ws_buffer(dev, ops.AUX_WS_SLOT)
                and self._route_ws is getattr(getattr(self.net, "lora_route", None), "ws", None))

    def _body(self):
        net, lf = self.net, self.trainer.loss_fn
        x_t, y = lf.get_inputs_targets(self.x0, self.R, self.t, self.noise)
        self.tf.copy_(self.t)                             # int64 -> float32 timesteps, as UNet2DModel.forward does
        pred, st = net._run_forward(x_t, self.tf, save=True)
        dpred = torch.empty_like(pred)
        if self.ws is not None:
            lf.shaped_launch(pred, y, dpred, self.loss, None, self.t, self.flags, ws=self.ws)
        else:
            ops.mse_fwd_bwd(pred, y, dpred, self.loss, lf._partial, pscale=None, gscale=lf.grad_scale, kind=lf._loss_type)
        net._run_backward(st, dpred)
        if self.trainer._keep is not None:                # masking is idempotent: every replay leaves the accumulated gradient masked
            self.trainer._keep_grad()

    def __call__(self, x0, R, noise, t, flags=None):
        net = self.net
        if hasattr(net, "refresh_packed"):                # weights changed since the last replay: rebuild the packed operands (one launch each)
            net.refresh_packed(False)
            net.refresh_packed(True)
        elif getattr(net, "_packed", None) is not None:
            net._packed.refresh(False)
            net._packed.refresh(True)
        self.x0.copy_(x0)
        self.R.copy_(R)
        self.noise.copy_(noise)
        self.t.copy_(t)
        if self.flags is not None:
            self.flags.copy_(flags)
        self.graph.replay()
        if self._last is not None:                        # (overwritten by the next replay, like self.loss)
            self.trainer.loss_fn.last_sample_loss, self.trainer.loss_fn.last_split = self._last
        if _DEBUG:
            torch.cuda.synchronize(net.device)
            print("[graph] replayed", flush=True)
        return self.loss[0].clone()       # the static buffer is overwritten by the next replay: callers keep losses across micro-steps


class Trainer:
    def __init__(self, model, loss_fn, lr: float, total_steps: int, warmup_steps: int = 500, grad_accum: int = 1,
                 max_grad_norm: Optional[float] = 1.0, n_allreduce_buckets: int = 4, graph_micro_step: Optional[bool] = None,
                 force_ddp_path: bool = False, ema: Optional[EMAConfig] = None, lora=None, lora_backward: Optional[str] = None,
                 sam: Optional[SAMConfig] = None, keep_pruned=None, anchor: Optional[AnchorConfig] = None,
                 anchor_weights: Optional[torch.Tensor] = None):
        """anchor: an anchor.AnchorConfig adds the gradient of lam / 2 * sum F (w - w0)^2 to every optimiser step (`_anchor_init`); w0 is the
        network's weights at construction, or `anchor_weights` (a flat tensor: a resumed run anchors to the original start); None changes nothing.
        keep_pruned: an actprune.PruneMask holds the pruned weight rows at +0.0 through the fine-tune (`_keep_init`); None changes nothing.
        sam: a SAMConfig makes every optimiser step a sharpness-aware one (`_sam_micro_step`); None changes nothing.
        lora_backward (with lora only; None means "full"): "full" -- the backward forms every weight gradient; "adapted" -- only what the
        adapter needs (lora.BackwardRoute; UNet2DModel).  The mode belongs to the run: no state records it, a state of either loads in both."""
        self.model, self.loss_fn = model, loss_fn
        self.base_lr = lr
        self.adapter = None
        check_sam(sam, grad_accum, lora, graph_micro_step, dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1,
                  getattr(model, "conv_math", None))              # every SAM refusal comes before the first launch
        self.sam = sam
        check_keep_pruned(keep_pruned, lora, sam, dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1)
        check_anchor(anchor, lora, dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1,
                     getattr(model, "conv_math", None))           # every anchor refusal comes before the first launch
        if anchor is None and anchor_weights is not None:
            raise ValueError("Trainer: anchor_weights needs anchor=AnchorConfig(...)")
        if lora is None and lora_backward is not None:
            raise ValueError(f"Trainer: lora_backward={lora_backward!r} needs lora=LoRAConfig(...)")
        if lora is not None:
            # LoRA fine-tune (lora.py): the weights are frozen in a clone, the optimiser owns the flat adapter buffer alone, and every optimiser
            # step ends by writing the merged weights back into flat_param.  Every check comes before the first launch.
            from .lora import LoRAAdam, LoRAAdapter, LoRAConfig
            if not isinstance(lora, LoRAConfig):
                raise TypeError(f"Trainer: lora must be a LoRAConfig, got {type(lora).__name__}")
            if ema is not None:
                raise ValueError("Trainer: lora together with ema is not built (the shadow would average merged weights the adapter cannot express)")
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise NotImplementedError("Trainer: lora in a process group of more than one rank is not built (the adapter gradient is formed "
                                          "from the local flat_grad)")
            self.adapter = LoRAAdapter(model, lora, backward="full" if lora_backward is None else lora_backward)
            self.opt = LoRAAdam(self.adapter, lr, max_grad_norm=max_grad_norm)
        else:
            self.opt = FusedAdam(model, lr, max_grad_norm=max_grad_norm, ema=ema)
        self._ema_swapped = False
        self.lr_lambda: Callable[[int], float] = get_cosine_schedule_with_warmup_lambda(warmup_steps, total_steps)
        self.grad_accum = max(1, int(grad_accum))
        self.micro = 0
        self.sched_step = 0                       # LambdaLR.last_epoch
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.n_buckets = n_allreduce_buckets
        # f16 mixed-precision mode (model.conv_math == "f16", opt-in): the loss gradient is multiplied by `loss_scale` (a power of two: exact in
        # f32) so that the input gradients survive their conversion to f16 operands, and divided out again inside the Adam kernel; a step whose
        # gradient is not finite is skipped by the kernel and the scale halved at the next check (GradScaler semantics with a lazy host check:
        # the norm is read back every `scale_check_every` optimiser steps, doubled again after `scale_growth_every` clean ones)
        self.loss_scale = float(2 ** 12)
        self.scale_check_every, self.scale_growth_every = 100, 2000
        self._since_growth = 0
        self.overflow_steps_seen = 0
        self._skipped_seen = 0                    # value of opt.skipped at the last lazy check
        self._recheck = False                     # the last lazy check found skipped steps: read the counter after every step until one passes clean
        self.loss_fn.grad_scale = self._scale() / self.grad_accum
        self._pending = []                        # async all-reduce handles of the current optimiser step
        self._sync_now = False
        # HIP-graph replay of the micro-step: on by default where a step is launch-bound (gradient accumulation = small micro-batches), single process
        self.graph_micro_step = (self.grad_accum > 1) if graph_micro_step is None else bool(graph_micro_step)
        self._graphs: Dict = {}
        self.sam_loss_perturbed: Optional[torch.Tensor] = None      # the loss of a SAM step's second pass (device, no sync)
        if sam is not None:
            self._sam_init()
        self.keep_pruned, self._keep, self._keep_tab = keep_pruned, None, None
        if keep_pruned is not None:
            self._keep_init()
        self.anchor = anchor
        if anchor is not None:
            self._anchor_init(anchor_weights)
        # force_ddp_path: the schedule of a multi-rank step (bucket hooks fired from the explicit backward, eager micro-step, one all-reduce per
        # bucket) on a process group of ANY size, including 1 -- what rank 0 of an 8-GPU run executes minus the wire time (bench.py --ddp-path)
        self.ddp_path = (self.world > 1 or (force_ddp_path and dist.is_available() and dist.is_initialized())) and hasattr(model, "grad_buckets")
        if self.ddp_path:
            model.bucket_ready_hook = self._bucket_ready      # overlap the all-reduce with the rest of backward
        model.zero_grad()
        self._zero_adapter_grad()

    def _zero_adapter_grad(self):
        """The adapted backward accumulates the direct layers' gradients into adapter.grad: cleared wherever flat_grad is."""
        if self.adapter is not None and self.adapter.route is not None:
            self.adapter.zero_grad()

    def _bucket_ready(self, i: int):
        """Called from the UNet's explicit backward when gradient bucket i is final (order: up|out, mid, down, temb)."""
        if not self._sync_now:
            return
        s, e = self.model.grad_buckets[i]
        self._pending.append(dist.all_reduce(self.model.flat_grad[s:e], op=dist.ReduceOp.SUM, async_op=True))

    def _scale(self) -> float:
        return self.loss_scale if getattr(self.model, "conv_math", None) == "f16" else 1.0

    def check_skipped(self, force: bool = False, count_step: bool = True):
        """Lazy finite-gradient check, every arithmetic: the Adam kernel leaves the parameters alone when the gradient norm is not finite and
        counts the step on the device; that counter is read back every `scale_check_every` optimiser steps (and from `state_dict`).

        * f16 mode (GradScaler semantics, reference VillanDiffusion.py:260-264 -> accelerate): ANY skipped step since the last check halves the
          loss scale and restarts the growth interval; skipped steps are taken back out of Adam's bias-correction count and the LR schedule
          (GradScaler / accelerate skip both), at the check rather than at the step -- the price of not synchronising every step.  After a check
          that found skipped steps the counter is read after EVERY step until a step passes clean (a persistent overflow then costs one step
          per halving, as under GradScaler, not `scale_check_every` steps);
        * every other arithmetic has no scale to lower: a non-finite gradient norm is a broken run (NaN statistics out of a GroupNorm poll
          timeout, a diverged model, ...) and raises instead of training on silently.

        count_step: this call follows an optimiser step (train_step).  A forced read from `state_dict` passes False: it applies what the
        counter already holds (a checkpoint never records steps the kernel refused) but advances neither the growth interval nor the scale."""
        if count_step:
            self._since_growth += 1
        if not force and not self._recheck and self.sched_step % self.scale_check_every:
            return
        if self.opt.max_grad_norm is None and self._scale() == 1.0:
            return                                   # no norm kernel in this configuration: nothing was counted
        skipped = int(self.opt.skipped)
        new = skipped - self._skipped_seen
        self._skipped_seen = skipped
        if new > 0 and self._scale() == 1.0:
            raise FloatingPointError(f"{new} optimiser step(s) had a non-finite gradient norm and were skipped by the Adam kernel "
                                     f"(arithmetic {getattr(self.model, 'conv_math', '?')!r}; asynchronous kernel errors, e.g. GroupNorm poll "
                                     f"timeouts: {ops.L.load().vd_async_errors(0)}; last library error: {ops.L.last_error()!r})")
        self._recheck = new > 0
        if new > 0:
            self.loss_scale = max(1.0, self.loss_scale * 0.5)
            self.overflow_steps_seen += new
            self._since_growth = 0
            self.opt.step_count = max(0, self.opt.step_count - new)
            self.sched_step = max(0, self.sched_step - new)
            if self.opt.ema is not None:                 # the kernel left the shadow alone on those steps: they are no EMA updates either
                self.opt.ema_step = max(0, self.opt.ema_step - new)
        elif count_step and self._scale() != 1.0 and self._since_growth >= self.scale_growth_every:
            self.loss_scale = min(float(2 ** 24), self.loss_scale * 2.0)
            self._since_growth = 0

    _check_scale = check_skipped

    @property
    def lr(self) -> float:
        return self.base_lr * self.lr_lambda(self.sched_step)

    @contextlib.contextmanager
    def ema_weights(self):
        """While open, the network holds the EMA weights and ``opt.ema`` the raw ones (diffusers' ``store`` / ``copy_to`` / ``restore``): the two
        flat buffers are exchanged in place on entry and again on exit, also after an exception -- no third buffer, no rounding.  The swap writes
        through raw pointers, which no version counter sees, so the operands derived from the weights are dropped each time
        (``model.weights_changed()``); the captured sampler forwards read ``flat_param`` by address and rebuild the packed operands before each
        replay, so they follow without a new capture.  It does not nest, and it cannot be entered inside an accumulation window (the gradients
        accumulated so far belong to the raw weights).  No optimiser step belongs inside."""
        if self.opt.ema is None:
            raise RuntimeError("ema_weights(): this trainer keeps no EMA (construct it with ema=EMAConfig(...))")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest: the network already holds the EMA weights")
        if self.micro % self.grad_accum != 0:
            raise RuntimeError(f"ema_weights() inside an open accumulation window (micro-step {self.micro % self.grad_accum} of {self.grad_accum})")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self.model
        finally:
            self._swap_ema()
            self._ema_swapped = False

    def _swap_ema(self):
        ops.swap(self.model.flat_param, self.opt.ema)
        ops.WEIGHTS_EPOCH += 1                           # caches keyed on (flat_param._version, WEIGHTS_EPOCH): transposed weights, packed operands
        self.model.weights_changed()

    # ---- masked fine-tune (actprune.PruneMask) ----------------------------------------------------------------------------------------------
    def _keep_init(self):
        """The pruned rows of the weights, of both Adam moments and of the EMA shadow are set to +0.0 once, one launch each.  From then on every
        optimiser step zeroes those rows of flat_grad before the norm (so the clip norm excludes them), and that alone keeps them: with a zero
        gradient and zero moments Adam's update is m = b1 * 0 + (1 - b1) * 0 = 0, v = 0, p = 0 - lr * 0 / (sqrt(0) + eps) = +0.0 exactly, and
        the shadow moves by (0 - 0) * (1 - decay) = 0 -- the rows stay +0.0 bit for bit with no second launch."""
        from .anp import neuron_table
        m = self.model
        tab = neuron_table(m, "all")
        keep = self.keep_pruned.keep
        if not torch.is_tensor(keep) or keep.dim() != 1 or keep.numel() != tab.n_neurons:
            raise ValueError(f"Trainer: keep_pruned holds {keep.numel() if torch.is_tensor(keep) else '?'} entries; the model has "
                             f"{tab.n_neurons} neurons (anp.neuron_table(model, 'all'))")
        self._keep_tab = tab
        self._keep = keep.detach().to(m.flat_param.device, torch.float32).contiguous()
        for buf in (m.flat_param, self.opt.exp_avg, self.opt.exp_avg_sq) + ((self.opt.ema,) if self.opt.ema is not None else ()):
            ops.neuron_keep_rows(buf, tab, self._keep)
        ops.WEIGHTS_EPOCH += 1                           # a raw-pointer write of the weights (as in `_swap_ema`)
        m.weights_changed()

    def _keep_grad(self):
        ops.neuron_keep_rows(self.model.flat_grad, self._keep_tab, self._keep)

    # ---- anchored fine-tune (anchor.AnchorConfig) ---------------------------------------------------------------------------------------------
    def _anchor_init(self, anchor_weights):
        """w0 (a clone of the weights as they are now -- after `_keep_init` zeroed pruned rows -- or the given flat tensor), the Fisher on the
        device, the penalty word and the scratch of its sum, allocated once."""
        fp = self.model.flat_param
        for what, v in (("anchor_weights", anchor_weights), ("the anchor's fisher", self.anchor.fisher)):
            if v is not None and (not torch.is_tensor(v) or v.dim() != 1 or v.numel() != fp.numel()):
                raise ValueError(f"Trainer: {what} holds {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}; the model's flat_param has "
                                 f"{fp.numel()} floats")
        self._anchor_lam = float(self.anchor.lam)          # (what the launch reads)
        self._anchor_w0 = (fp if anchor_weights is None else anchor_weights).detach().to(fp.device, torch.float32).clone().contiguous()
        self._anchor_F = None if self.anchor.fisher is None else self.anchor.fisher.detach().to(fp.device, torch.float32).clone().contiguous()
        self._anchor_pen = torch.zeros(1, device=fp.device, dtype=torch.float32)
        self._anchor_partial = torch.empty(1024, device=fp.device, dtype=torch.float32)

    def _anchor_grad(self):
        """flat_grad += lam * F * (w - w0) and the unscaled penalty into its device word: one launch, nothing read back.  At a sync step
        flat_grad holds the MEAN gradient of the accumulation window (the loss gradient is pre-divided by grad_accum), so coef = lam."""
        m = self.model
        ops.anchor_grad(m.flat_grad, m.flat_param, self._anchor_w0, self._anchor_F, self._anchor_lam, self._anchor_partial, self._anchor_pen)

    @property
    def anchor_penalty(self) -> Optional[float]:
        """lam / 2 * sum F (w - w0)^2 at the weights the last optimiser step STARTED from (what the step's gradient saw); None without an
        anchor.  Reading it synchronises; the step itself never does."""
        if self.anchor is None:
            return None
        return 0.5 * self._anchor_lam * float(self._anchor_pen)

    # ---- sharpness-aware minimisation ------------------------------------------------------------------------------------------------------
    def _sam_init(self):
        """The buffers of a SAM step, allocated once: the backup of the weights, the norm word and, in "neuron" mode, the table and three floats
        per neuron."""
        cfg, fp = self.sam, self.model.flat_param
        self._sam_rho = float(cfg.rho)                     # (what the launches read)
        self._sam_backup = torch.empty_like(fp)
        self._sam_norm_sq = torch.zeros(1, device=fp.device, dtype=torch.float32)
        self._sam_partial = torch.empty(1024, device=fp.device, dtype=torch.float32)
        self._sam_tab = None
        if cfg.mode == "neuron":
            from .anp import neuron_table
            self._sam_tab = neuron_table(self.model, cfg.layers)
            self._sam_wsq, self._sam_gsq, self._sam_coef = (torch.zeros(self._sam_tab.n_neurons, device=fp.device, dtype=torch.float32)
                                                            for _ in range(3))

    def _sam_perturb(self):
        """flat_param <- w + e(g), g = flat_grad, and the backup <- w: the norm and the perturbation as single launches over the flat buffers,
        nothing read back.  A raw-pointer write, so the operands derived from the weights are dropped (as in `_swap_ema`)."""
        cfg, m = self.sam, self.model
        w, g, nsq = m.flat_param, m.flat_grad, self._sam_norm_sq
        if cfg.mode == "neuron":
            tab = self._sam_tab
            ops.neuron_grad(w, w, tab, self._sam_wsq)
            ops.neuron_grad(g, g, tab, self._sam_gsq)
            ops.sam_neuron_coef(self._sam_wsq, self._sam_gsq, tab, self._sam_coef, nsq, self._sam_rho, cfg.eta)
            with torch.no_grad():
                self._sam_backup.copy_(w)
            ops.neuron_axpy(w, g, tab, self._sam_coef)
        else:
            if cfg.mode == "sam":
                ops.l2norm_sq(g, self._sam_partial, nsq)
            else:
                ops.sam_norm_sq(g, w, self._sam_partial, nsq, "asam", cfg.eta)
            ops.sam_perturb(w, g, self._sam_backup, nsq, self._sam_rho, cfg.mode, cfg.eta)
        ops.WEIGHTS_EPOCH += 1
        m.weights_changed()

    def _sam_restore(self):
        with torch.no_grad():
            self.model.flat_param.copy_(self._sam_backup)
        ops.WEIGHTS_EPOCH += 1
        self.model.weights_changed()

    def _sam_micro_step(self, batch, timesteps, noise, target_key, poison_key):
        """Both passes of a SAM step on one batch, timesteps, noise and poison flags; leaves the gradient at w + e in flat_grad and the network
        at w (also after an exception in the second pass), and returns the loss at w."""
        m, lf = self.model, self.loss_fn
        if getattr(m, "conv_math", None) == "f16":
            raise NotImplementedError("Trainer: sam with conv_math='f16' is not built (an overflow in the first pass has no skip path)")
        if noise is None:                                  # drawn once, as LossFn.p_loss would: a SAM step consumes the stream like a plain one
            noise = lf._noise(batch[target_key].to(m.device).float())

        def one_pass():
            loss = lf.p_loss_by_keys(batch, m, target_latent_key=target_key, poison_latent_key=poison_key, timesteps=timesteps, noise=noise)
            loss.backward()
            return loss

        sync_now, self._sync_now = self._sync_now, False   # (the bucket hooks of the multi-rank schedule belong to the second pass)
        loss = one_pass()
        kept = (lf.last_sample_loss, lf.last_split)        # a shaped loss's readouts of pass 1: a few floats, cloned before pass 2 refills them
        if getattr(lf, "shaped", False):
            kept = tuple(None if v is None else v.clone() for v in kept)
        self._sam_perturb()
        try:
            m.zero_grad()
            self._sync_now = sync_now
            self.sam_loss_perturbed = one_pass().detach()
        finally:
            self._sam_restore()
        lf.last_sample_loss, lf.last_split = kept
        return loss

    def train_step(self, batch, timesteps: torch.Tensor, noise: Optional[torch.Tensor] = None, last_batch: bool = False,
                   target_key: str = "target", poison_key: str = "pixel_values"):
        """One micro-step; returns the (un-divided) loss tensor of this micro-batch."""
        if self._ema_swapped:
            raise RuntimeError("train_step() inside ema_weights(): the network holds the EMA weights")
        sync = (self.micro + 1) % self.grad_accum == 0 or last_batch   # accelerate: sync on every G-th and on the last batch
        self._sync_now = sync and self.model.bucket_ready_hook is not None
        if self.micro % self.grad_accum == 0:                          # first micro-step of an accumulation window (the scale never changes inside one)
            self._step_scale = self._scale()
        self.loss_fn.grad_scale = self._step_scale / self.grad_accum
        if self.sam is not None and len(batch[target_key]) > 0:
            loss = self._sam_micro_step(batch, timesteps, noise, target_key, poison_key)
        else:
            loss = self._graphed(batch, timesteps, noise, target_key, poison_key)
        masked = self._keep is not None and loss is not None      # a replayed micro-step ends with the mask launch: flat_grad is masked already
        if loss is None:
            loss = self.loss_fn.p_loss_by_keys(batch, self.model, target_latent_key=target_key, poison_latent_key=poison_key,
                                               timesteps=timesteps, noise=noise)
            if torch.is_tensor(loss):
                loss.backward()
        self.micro = 0 if last_batch else self.micro + 1          # accelerate `_do_sync`: the counter restarts at end_of_dataloader
        if sync:
            if self._sync_now and self._pending:
                for w in self._pending:                           # bucketed all-reduces were launched during backward
                    w.wait()
                self._pending = []
            else:
                allreduce_flat_grad(self.model.flat_grad, self.n_buckets, even_alone=self.ddp_path)
            self._sync_now = False
            if self.anchor is not None:
                self._anchor_grad()                               # before the norm: the clip sees the gradient of loss + penalty
            if self._keep is not None and (not masked or self.anchor is not None):
                self._keep_grad()                                 # before the norm: the clip norm excludes the pruned rows (whose w0 need not be 0:
                                                                  # the anchor launch would pull them back, so the mask follows it at every sync)
            self.opt.step(lr=self.lr, grad_inv_scale=1.0 / (self.world * self._step_scale), need_norm=self._step_scale != 1.0)
            self.sched_step += 1
            self._check_scale()
            self.model.zero_grad()
            self._zero_adapter_grad()
        return loss

    def _graphed(self, batch, timesteps, noise, target_key, poison_key):
        """The micro-step as a HIP-graph replay, or None when this step has to run eagerly."""
        m, lf = self.model, self.loss_fn
        if not self.graph_micro_step or self.ddp_path or not hasattr(m, "_run_backward") or getattr(lf, "_sde", None) == "SDE-VE":
            return None
        x0, R = batch[target_key], batch[poison_key]
        if len(x0) == 0 or getattr(m, "device", torch.device("cpu")).type != "cuda" or not hasattr(m, "_packed"):
            return None
        dev = m.device
        flags = None
        if getattr(lf, "shaped", False):                  # a shaped loss: its poison flags ride in the batch; missing ones raise here, before any launch
            flags = lf.shaped_flags(~torch.as_tensor(batch["is_clean"]).bool() if "is_clean" in batch else None, len(x0), dev)
        x0, R = x0.to(dev).float(), R.to(dev).float()
        if noise is None:
            noise = lf._noise(x0)
        lf._tables(dev)
        key = (tuple(x0.shape), flags is not None)
        g = self._graphs.get(key)
        if g is None or not g.valid():
            self._graphs.clear()                          # one shape at a time: a graph's private pool pins the activations of a whole step
            g = self._graphs[key] = GraphedMicroStep(self, x0, R, noise.to(dev), timesteps.to(dev), flags)
        return g(x0, R, noise.to(dev), timesteps.to(dev), flags)

    def state_dict(self) -> Dict:
        if self._ema_swapped:
            raise RuntimeError("state_dict() inside ema_weights(): the network holds the EMA weights and the shadow the raw ones")
        if getattr(self.model, "device", torch.device("cpu")).type == "cuda":
            self.check_skipped(force=True, count_step=False)      # a checkpoint never records steps the kernel refused
        sd = {"optimizer": self.opt.state_dict(), "micro": self.micro, "sched_step": self.sched_step,
              "loss_scale": self.loss_scale, "since_growth": self._since_growth, "overflow_steps_seen": self.overflow_steps_seen}
        if self.adapter is not None:
            sd["lora"] = self.adapter.train_state()
        if self.sam is not None:
            sd["sam"] = asdict(self.sam)                 # for information only: SAM keeps no state between steps, load_state_dict ignores it
        if self.anchor is not None:                      # w0 and F stay out (two more copies of the network): whoever resumes reloads them
            sd["anchor"] = {"lam": float(self.anchor.lam), "mode": self.anchor.mode}
        if self.keep_pruned is not None:
            sd["keep_pruned"] = self.keep_pruned.keep.detach().to("cpu", torch.float32).clone()
        return sd

    def load_state_dict(self, sd: Dict):
        if ("lora" in sd) != (self.adapter is not None):
            raise ValueError("load_state_dict: the state " + ("holds a" if "lora" in sd else "holds no") + " LoRA adapter but this trainer was "
                             "built " + ("without" if "lora" in sd else "with") + " one (Trainer lora=...)")
        if ("keep_pruned" in sd) != (self.keep_pruned is not None):
            raise ValueError("load_state_dict: the state " + ("holds a" if "keep_pruned" in sd else "holds no") + " prune mask but this trainer was "
                             "built " + ("without" if "keep_pruned" in sd else "with") + " one (Trainer keep_pruned=...)")
        if ("anchor" in sd) != (self.anchor is not None):
            raise ValueError("load_state_dict: the state " + ("was written with an" if "anchor" in sd else "was written without an") + " anchor "
                             "but this trainer was built " + ("without" if "anchor" in sd else "with") + " one (Trainer anchor=...)")
        if self.keep_pruned is not None and not torch.equal(sd["keep_pruned"].to("cpu", torch.float32), self.keep_pruned.keep.to("cpu", torch.float32)):
            raise ValueError("load_state_dict: the state was written under a different prune mask than this trainer's keep_pruned")
        if self.adapter is not None:
            self.adapter.load_train_state(sd["lora"])
        self.opt.load_state_dict(sd["optimizer"])
        self.micro, self.sched_step = int(sd["micro"]), int(sd["sched_step"])
        self.loss_scale = float(sd.get("loss_scale", self.loss_scale))          # (absent from checkpoints written before round 5)
        self._since_growth = int(sd.get("since_growth", 0))
        self.overflow_steps_seen = int(sd.get("overflow_steps_seen", 0))
        self._skipped_seen = int(self.opt.skipped)
