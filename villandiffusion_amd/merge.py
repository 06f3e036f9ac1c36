"""Checkpoint merging in weight space: task arithmetic (Ilharco et al., ICLR 2023) and TIES-Merging (Yadav et al., NeurIPS 2023) of up to eight
checkpoints that were fine-tuned from one base.  With tau_i = theta_i - theta_base the task vector of checkpoint i,

* "linear":  theta = theta_base + sum_i lambda_i tau_i  -- the uniform average ("model soup", lambda_i = lam / K), a weighted sum, or negation
             (lambda_i < 0: subtract what a backdoor fine-tune added);
* "ties":    trim each tau_i to its `density` share of largest-magnitude entries, elect one sign per parameter (the sign of the sum of the
             trimmed vectors), average the entries that carry it, theta = theta_base + lam * that mean.

Merging a backdoored fine-tune with other fine-tunes of its base is a data-free mitigation (Arora et al. 2024) -- and the attack surface of
BadMerging.  No data and no pass of the network is needed: K exact selections (ops.merge_select -> vd_merge_select, a radix selection over the
float bits) and ONE launch over the flat buffers (ops.merge_apply -> vd_merge_apply) with no temporary.  Only flat_param is written, so
UNet2DModel, NCSNppModel and the latent UNet all work, and conv_math is not involved.

Two deliberate departures from the published TIES code: the k largest magnitudes are kept with ties at the threshold all kept (the published
code keeps k + 1), and a sign sum of exactly zero elects + (the published code takes the majority sign of the whole vector there).

`drop` > 0 is DARE (Yu et al., ICML 2024): every entry of a task vector is dropped with probability p and the survivors are multiplied by
1 / (1 - p), then "linear" adds them (DARE-linear) or "ties" elects signs over them (DARE-TIES) -- ops.merge_apply_drop -> vd_merge_apply_drop,
still one launch.  The draw is Philox4x32-10 on (seed, task index, element index): the same bits on every device and in tests/merge_drop_ref.py.
Two departures from the published DARE code: the mask is an integer Bernoulli, keep where a 32-bit word >= drop_threshold(p) = floor(p 2^32),
so the realised keep probability is (2^32 - T) / 2^32, while the rescale is that of the nominal p, f32(1 / (1 - p)).

`fine_mix` is Fine-mixing (Zhang et al., Findings of EMNLP 2022) from the same mask: a random share `keep` of a backdoored fine-tune's weights
is kept, the rest is taken from the clean base; the result is then fine-tuned on a little clean data by the ordinary driver."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Union

import torch

from .anchor import _timesteps_of, fisher_draws

MERGE_METHODS = ("ties", "linear")
MAX_TASKS = 8


@dataclass
class MergeConfig:
    """method: "ties" or "linear".  density: the share of each task vector's entries that is kept (the largest magnitudes), in [0, 1]; 1 keeps
    everything and runs no selection.  lam: the scale of the merged task vector.  weights: the per-task weights of "linear" (None: 1 / K each);
    task i enters with lambda_i = lam * weights[i].  drop: the probability with which an entry of a task vector is dropped (DARE), in [0, 1),
    one number or one per task; 0 draws nothing and launches what a merge without it launches.  seed: of the drop, in [0, 2^64); task i uses
    stream i.  rescale: multiply the surviving entries by 1 / (1 - drop)."""
    method: str = "ties"
    density: float = 0.2
    lam: float = 1.0
    weights: Optional[Sequence[float]] = None
    drop: Union[float, Sequence[float]] = 0.0
    seed: int = 0
    rescale: bool = True

    def __post_init__(self):
        if self.method not in MERGE_METHODS:
            raise ValueError(f"MergeConfig: method must be one of {MERGE_METHODS}, got {self.method!r}")
        d = self.density
        if isinstance(d, bool) or not isinstance(d, (int, float)) or not math.isfinite(d) or not 0.0 <= d <= 1.0:
            raise ValueError(f"MergeConfig: density must be a number in [0, 1], got {d!r}")
        if isinstance(self.lam, bool) or not isinstance(self.lam, (int, float)) or not math.isfinite(self.lam):
            raise ValueError(f"MergeConfig: lam must be a finite number, got {self.lam!r}")
        if self.weights is not None:
            if self.method != "linear":
                raise ValueError(f"MergeConfig: weights are the per-task coefficients of method 'linear'; method is {self.method!r}")
            if isinstance(self.weights, (str, bytes)) or not hasattr(self.weights, "__len__") or len(self.weights) == 0:
                raise ValueError(f"MergeConfig: weights must be a non-empty sequence of finite numbers, got {self.weights!r}")
            for v in self.weights:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                    raise ValueError(f"MergeConfig: weights must be a non-empty sequence of finite numbers, got {self.weights!r}")
            self.weights = tuple(float(v) for v in self.weights)
        ok = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v) and 0.0 <= v < 1.0       # noqa: E731
        if isinstance(self.drop, (str, bytes)) or not (ok(self.drop) or (hasattr(self.drop, "__len__") and len(self.drop) > 0 and
                                                                          all(ok(v) for v in self.drop))):
            raise ValueError(f"MergeConfig: drop must be a number in [0, 1) or a non-empty sequence of such numbers, got {self.drop!r}")
        self.drop = tuple(float(v) for v in self.drop) if hasattr(self.drop, "__len__") else float(self.drop)
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or not 0 <= self.seed < 1 << 64:
            raise ValueError(f"MergeConfig: seed must be an integer in [0, 2^64), got {self.seed!r}")
        if not isinstance(self.rescale, bool):
            raise ValueError(f"MergeConfig: rescale must be a bool, got {self.rescale!r}")


def _f32(v: float) -> float:
    return ctypes.c_float(v).value


def rank_of(density: float, n: int) -> int:
    """k of "keep the k largest magnitudes": floor(density * n) in float64, clamped to [0, n].  The one place k comes from."""
    return max(0, min(int(n), int(math.floor(float(density) * float(n)))))


def coefficients(cfg: MergeConfig, K: int, lam: Optional[float] = None) -> List[float]:
    """The K per-task lambda_i of "linear": lam * weights[i] (weights None: lam / K), computed in float64 and rounded once to float32 -- the
    values the kernel receives, and the oracle uses.  lam None: cfg.lam."""
    lam = float(cfg.lam if lam is None else lam)
    if cfg.weights is None:
        return [_f32(lam / K)] * K
    if len(cfg.weights) != K:
        raise ValueError(f"merge: the configuration holds {len(cfg.weights)} weights, but {K} task checkpoints were given")
    return [_f32(lam * w) for w in cfg.weights]


def drop_threshold(p: float) -> int:
    """T of "keep where the 32-bit word >= T": floor(p * 2^32) in float64 -- exact, a scaling by a power of two -- for p in [0, 1].  The one
    place T comes from.  The realised keep probability is (2^32 - T) / 2^32."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"drop_threshold: p must lie in [0, 1], got {p!r}")
    return int(math.floor(p * 4294967296.0))


def rescale_of(p: float) -> float:
    """f32(1 / (1 - p)): the quotient in float64, rounded once.  Of the NOMINAL p, as DARE has it, not of the realised keep probability."""
    return _f32(1.0 / (1.0 - float(p)))


def drops(cfg: MergeConfig, K: int) -> List[float]:
    """The K per-task drop probabilities: cfg.drop for every task, or the sequence itself, whose length must be K."""
    if not isinstance(cfg.drop, tuple):
        return [cfg.drop] * K
    if len(cfg.drop) != K:
        raise ValueError(f"merge: the configuration holds {len(cfg.drop)} drop probabilities, but {K} task checkpoints were given")
    return list(cfg.drop)


def _check(model, base, tasks, cfg, who):
    if not isinstance(cfg, MergeConfig):
        raise TypeError(f"{who}: cfg must be a MergeConfig, got {type(cfg).__name__}")
    tasks = list(tasks)
    if not 1 <= len(tasks) <= MAX_TASKS:
        raise ValueError(f"{who}: {len(tasks)} task checkpoints were given; one launch merges 1 to {MAX_TASKS}")
    n, dev = int(model.flat_numel), model.flat_param.device
    for what, v in [("base", base)] + [(f"tasks[{i}]", t) for i, t in enumerate(tasks)]:
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != n or v.device != dev or not v.is_contiguous():
            got = f"{tuple(v.shape)} {v.dtype} on {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"{who}: {what} must be a flat contiguous float32 tensor of the model's {n} floats (model.flat_numel) on {dev}, got {got}")
    coefficients(cfg, len(tasks))                         # weights of the wrong length
    drops(cfg, len(tasks))                                # drop probabilities of the wrong length
    return tasks, n, dev


class _Trim:
    """The part of a merge that does not depend on lam: the thresholds (K selections, or zeros at density 1) and the task vectors' geometry."""

    def __init__(self, model, base, tasks, cfg, who):
        from . import ops
        self.tasks, self.n, dev = _check(model, base, tasks, cfg, who)
        self.model, self.base, self.cfg = model, base, cfg
        K = self.K = len(self.tasks)
        self.k = rank_of(cfg.density, self.n)
        self.thr = torch.zeros(K, device=dev, dtype=torch.float32)
        self.rec = torch.zeros((K, 3), device=dev, dtype=torch.int64)
        self.drop = drops(cfg, K)
        self.dropped = any(p > 0.0 for p in self.drop)
        self.drop_thr = [drop_threshold(p) for p in self.drop]
        self.partial = torch.empty(ops.MERGE_DROP_PARTIAL if self.dropped else ops.MERGE_PARTIAL, device=dev, dtype=torch.int32)
        self.stats = torch.zeros((3 if self.dropped else 2) * K + 2, device=dev, dtype=torch.int64)
        self.selected = cfg.density < 1.0
        # the geometry: |tau_i|^2, |tau_j|^2 and |tau_i - tau_j|^2 of every pair from one vd_curve_geometry launch each (K = 1: the norm alone)
        pairs = [(i, j) for i in range(K) for j in range(i + 1, K)] or [(0, 0)]
        gpart = torch.empty(3 * 1024, device=dev, dtype=torch.float32)
        self._pairs, self._sums = pairs, torch.zeros((len(pairs), 3), device=dev, dtype=torch.float32)
        for row, (i, j) in enumerate(pairs):
            ops.curve_geometry(self.tasks[i], base, self.tasks[j], gpart, self._sums[row])
        if self.selected:
            ws = torch.empty(ops.merge_plan(self.n)[3], device=dev, dtype=torch.uint8)
            for i, t in enumerate(self.tasks):
                ops.merge_select(t, base, self.k, ws, self.thr[i:i + 1], self.rec[i])
        # one read-back before anything is written: a non-finite task vector is refused here
        rec, sums = self.rec.cpu(), self._sums.cpu().double()
        sq = [0.0] * K
        for (i, j), s in zip(pairs, sums):
            sq[i], sq[j] = float(s[0]), float(s[1])
        for i in range(K):
            if int(rec[i, 2]) != 0 or not math.isfinite(sq[i]):
                count = f"{int(rec[i, 2])} entries of" if self.selected else "the squared norm of"
                raise FloatingPointError(f"{who}: tasks[{i}] minus base is not finite ({count} the task vector are inf or NaN); nothing was merged")
        self.norms = [math.sqrt(max(v, 0.0)) for v in sq]
        cos = [[1.0] * K for _ in range(K)]
        for (i, j), s in zip(pairs, sums):
            if i != j:
                den = 2.0 * math.sqrt(max(float(s[0]), 0.0)) * math.sqrt(max(float(s[1]), 0.0))
                cos[i][j] = cos[j][i] = (float(s[0]) + float(s[1]) - float(s[2])) / den if den > 0.0 else 0.0     # the law of cosines
        self.cosine = cos

    def apply(self, lam: float, out=None):
        """One launch: the merge at `lam` into `out`, or (out None) into the network's flat_param."""
        from . import ops
        cfg = self.cfg
        lams = coefficients(cfg, self.K, lam) if cfg.method == "linear" else None
        rescale = [rescale_of(p) for p in self.drop] if self.dropped and cfg.rescale else None

        def launch(o, weights):
            if not self.dropped:
                return ops.merge_apply(o, self.base, self.tasks, lams, self.thr, cfg.method, _f32(float(lam)), self.partial, self.stats, weights=weights)
            # task i draws from stream i of cfg.seed, at every lam: a scan sees one set of masks
            return ops.merge_apply_drop(o, self.base, self.tasks, lams, self.thr, cfg.method, _f32(float(lam)), self.drop_thr, rescale,
                                        list(range(self.K)), cfg.seed, self.partial, self.stats, weights=weights)

        if out is not None:
            return launch(out, False)
        launch(self.model.flat_param, True)
        self.model.weights_changed()
        return self.model.flat_param

    def report(self) -> Dict:
        """The read-outs of the last `apply` (synchronises)."""
        K, n = self.K, max(self.n, 1)
        stats, thr, rec = [int(v) for v in self.stats.cpu()], [float(v) for v in self.thr.cpu()], self.rec.cpu()
        drawn = []
        if self.dropped:
            drawn, stats = stats[:K], stats[K:]
        kept, won, support, conflict = stats[:K], stats[K:2 * K], stats[2 * K], stats[2 * K + 1]
        if self.dropped:                                  # kept counts the entries that passed the threshold AND the draw
            for i in range(K):
                if kept[i] > drawn[i] or (self.selected and kept[i] > int(rec[i, 0]) + int(rec[i, 1])):
                    raise RuntimeError(f"merge: tasks[{i}]: the merge kept {kept[i]} entries, but drew {drawn[i]} and the selection counted "
                                       f"{int(rec[i, 0]) + int(rec[i, 1])} at or above the threshold")
        elif self.selected:
            for i in range(K):
                if kept[i] != int(rec[i, 0]) + int(rec[i, 1]):
                    raise RuntimeError(f"merge: tasks[{i}]: the merge kept {kept[i]} entries, the selection counted {int(rec[i, 0])} above and "
                                       f"{int(rec[i, 1])} at the threshold")
        out = {"method": self.cfg.method, "density": float(self.cfg.density), "k": self.k if self.selected else self.n, "numel": self.n,
               "tasks": [{"threshold": thr[i], "kept": kept[i], "won": won[i], "kept_share": kept[i] / n, "won_share": won[i] / n,
                          "norm": self.norms[i]} for i in range(K)],
               "support": support, "conflict": conflict, "support_share": support / n, "conflict_share": conflict / support if support else 0.0,
               "cosine": self.cosine}
        if self.dropped:
            out.update(drop=list(self.drop), seed=self.cfg.seed, rescale=self.cfg.rescale)
            for i, row in enumerate(out["tasks"]):
                row.update(drop_threshold=self.drop_thr[i], drawn=drawn[i], drawn_share=drawn[i] / n)
        return out


def merge(model, base: torch.Tensor, tasks: Sequence[torch.Tensor], cfg: Optional[MergeConfig] = None) -> Dict:
    """Merge the task checkpoints into the network: `base` and every task are flat float32 tensors of model.flat_numel on the model's device
    (`tasks[i]` is a whole checkpoint theta_i, not the difference).  K selections where density < 1, one launch into model.flat_param, then
    `model.weights_changed()`.  A task vector with an inf or a NaN raises FloatingPointError, naming the task, before anything is written.

    Returns {"method", "density", "k", "numel", "tasks": [{"threshold", "kept", "won", "kept_share", "won_share", "norm"}], "support",
    "conflict", "support_share", "conflict_share", "cosine"}: threshold the k-th largest |tau_i| (0 at density 1); kept the entries with
    |tau_i| >= threshold and won those that entered the merged value ("linear": the non-zero kept ones), shares of numel; norm = |tau_i|;
    support the positions where any trimmed task vector is non-zero, conflict those where non-zero entries of both signs meet,
    conflict_share = conflict / support; cosine the K x K matrix of cos(tau_i, tau_j), from the three squared sides of each pair by the law of
    cosines in float64.

    With cfg.drop > 0 (DARE) the thresholds are still those of the undropped task vectors, the one launch is vd_merge_apply_drop, and the
    result gains "drop" (the K probabilities), "seed", "rescale" and per task "drop_threshold" (floor(p 2^32)), "drawn" (the entries the draw
    kept, whatever their magnitude) and "drawn_share"; kept then counts the entries that passed the threshold and the draw."""
    cfg = MergeConfig() if cfg is None else cfg
    trim = _Trim(model, base, tasks, cfg, "merge")
    trim.apply(cfg.lam)
    return trim.report()


def _scan(model, restore, loss_fn, batches, seed, trigger, key, values, apply):
    """[{key: v, "loss_clean", "loss_poison"?}] for v in values: `apply(v)` writes the network's weights, the no-grad losses follow; in the end
    the network holds `restore` again."""
    from . import ops
    dev = model.device
    T = _timesteps_of(loss_fn)
    shaped = getattr(loss_fn, "shaped", False)
    out = []
    try:
        with torch.no_grad():
            for v in values:
                apply(v)
                clean, poison = [], []
                for k, b in enumerate(batches):
                    x0 = (b["image"] if isinstance(b, dict) else b).to(dev).float()
                    steps, eps = fisher_draws(x0.shape, T, seed, k)
                    steps, eps = steps.to(dev), eps.to(dev)
                    kw = {"is_poison": torch.zeros(len(x0), dtype=torch.bool, device=dev)} if shaped else {}
                    clean.append(loss_fn.p_loss(model, x0, torch.zeros_like(x0), steps, noise=eps, **kw).detach().reshape(()))
                    if trigger is not None:
                        target = b["target"].to(dev).float()
                        target = target.expand_as(x0) if target.dim() == 3 else target
                        R = trigger.to(dev).float().expand_as(x0)
                        kw = {"is_poison": torch.ones(len(x0), dtype=torch.bool, device=dev)} if shaped else {}
                        poison.append(loss_fn.p_loss(model, target.contiguous(), R.contiguous(), steps, noise=eps, **kw).detach().reshape(()))
                row = {key: v, "loss_clean": float(torch.stack(clean).double().mean())}
                if trigger is not None:
                    row["loss_poison"] = float(torch.stack(poison).double().mean())
                out.append(row)
    finally:
        with torch.no_grad():
            model.flat_param.copy_(restore)
        ops.WEIGHTS_EPOCH += 1
        model.weights_changed()
    return out


def merge_scan(model, base: torch.Tensor, tasks: Sequence[torch.Tensor], cfg: MergeConfig, loss_fn, batches: Iterable, lams: Sequence[float],
               seed: int = 0, trigger: Optional[torch.Tensor] = None):
    """The loss of the merged network at each lam of `lams` (in place of cfg.lam), to choose lam by: the selections run once, the merge is
    launched per lam, and the no-grad clean loss is the mean over `batches`.

    batches, seed and trigger are `curve.curve_scan`'s: clean image (or latent) tensors or dicts that hold them under "image"; batch k uses the
    draws of `anchor.fisher_draws(shape, T, seed, k)` at every lam; with `trigger` every row also holds the poisoned loss (the batches are dicts
    with a "target" then).  Returns [{"lam", "loss_clean", "loss_poison"?}]; afterwards the network holds the weights it held before, bit for
    bit."""
    from . import ops
    batches = list(batches)
    if not batches:
        raise ValueError("merge_scan: no batches")
    lams = [float(v) for v in lams]
    for v in lams:
        if not math.isfinite(v):
            raise ValueError(f"merge_scan: every lam must be finite, got {v!r}")
    if trigger is not None and not all(isinstance(b, dict) and "target" in b and "image" in b for b in batches):
        raise ValueError("merge_scan: with a trigger every batch is a dict with the clean images under 'image' and the backdoor target under 'target'")
    if not isinstance(cfg, MergeConfig):
        raise TypeError(f"merge_scan: cfg must be a MergeConfig, got {type(cfg).__name__}")
    _check(model, base, tasks, cfg, "merge_scan")
    keep = model.flat_param.detach().clone()
    if base.data_ptr() == model.flat_param.data_ptr() or any(torch.is_tensor(t) and t.data_ptr() == model.flat_param.data_ptr() for t in tasks):
        raise ValueError("merge_scan: base and the tasks must be copies, not the network's own flat_param (every lam overwrites it)")
    trim = _Trim(model, base, tasks, cfg, "merge_scan")
    return _scan(model, keep, loss_fn, batches, seed, trigger, "lam", lams, trim.apply)


def fine_mix(model, clean: torch.Tensor, backdoored: torch.Tensor, keep: float, seed: int = 0) -> Dict:
    """Fine-mixing (Zhang et al., Findings of EMNLP 2022), the mixing step: a random share `keep` of the backdoored fine-tune's weights stays,
    every other weight is taken from the clean base it was fine-tuned from -- out = where(mask, backdoored, clean), bits copied, in one launch
    (vd_merge_apply_drop, VD_DROP_COPY) into model.flat_param, then `model.weights_changed()`.  The mask is stream 0 of `seed` at the threshold
    T = 2^32 - floor(keep 2^32): keep = 1 gives the backdoored weights, keep = 0 the clean ones.  The mixed network is then fine-tuned on a
    little clean data by the ordinary driver.  `clean` and `backdoored` are flat float32 tensors of model.flat_numel on the model's device; an
    inf or a NaN in either raises FloatingPointError before anything is written.

    Returns {"keep", "seed", "drop_threshold", "drawn", "drawn_share", "differing", "numel"}: drawn the weights taken from `backdoored`,
    differing those of them that differ from the clean weight (as floats)."""
    from . import ops
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not math.isfinite(keep) or not 0.0 <= keep <= 1.0:
        raise ValueError(f"fine_mix: keep must be a number in [0, 1], got {keep!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"fine_mix: seed must be an integer in [0, 2^64), got {seed!r}")
    n, dev = int(model.flat_numel), model.flat_param.device
    for what, v in (("clean", clean), ("backdoored", backdoored)):
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != n or v.device != dev or not v.is_contiguous():
            got = f"{tuple(v.shape)} {v.dtype} on {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"fine_mix: {what} must be a flat contiguous float32 tensor of the model's {n} floats (model.flat_numel) on {dev}, got {got}")
    T = (1 << 32) - drop_threshold(keep)
    gpart, sums = torch.empty(3 * 1024, device=dev, dtype=torch.float32), torch.zeros(3, device=dev, dtype=torch.float32)
    ops.curve_geometry(backdoored, clean, backdoored, gpart, sums)
    if not math.isfinite(float(sums[0])):
        raise FloatingPointError("fine_mix: backdoored minus clean is not finite (the squared norm of the difference is inf or NaN); nothing was mixed")
    partial = torch.empty(5 * 1024, device=dev, dtype=torch.int32)
    stats = torch.zeros(5, device=dev, dtype=torch.int64)
    ops.merge_apply_drop(model.flat_param, clean, [backdoored], None, None, "linear", 0.0, [T], None, [0], seed, partial, stats, copy=True,
                         weights=True)
    model.weights_changed()
    st = [int(v) for v in stats.cpu()]
    return {"keep": float(keep), "seed": seed, "drop_threshold": T, "drawn": st[0], "drawn_share": st[0] / max(n, 1), "differing": st[3], "numel": n}


def fine_mix_scan(model, clean: torch.Tensor, backdoored: torch.Tensor, loss_fn, batches: Iterable, keeps: Sequence[float], seed: int = 0,
                  data_seed: int = 0, trigger: Optional[torch.Tensor] = None):
    """The loss of the mixed network at each keep share of `keeps`, to choose the share by: `fine_mix(..., keep, seed)` per share (the masks of
    one seed are nested: a weight kept at a share is kept at every larger one), then the no-grad losses as in `merge_scan` (batches, trigger
    and `data_seed` are its batches, trigger and seed).  Returns [{"keep", "loss_clean", "loss_poison"?}]; afterwards the network holds the
    weights it held before, bit for bit."""
    batches = list(batches)
    if not batches:
        raise ValueError("fine_mix_scan: no batches")
    keeps = [float(v) for v in keeps]
    for v in keeps:
        if not (math.isfinite(v) and 0.0 <= v <= 1.0):
            raise ValueError(f"fine_mix_scan: every keep share must lie in [0, 1], got {v!r}")
    if trigger is not None and not all(isinstance(b, dict) and "target" in b and "image" in b for b in batches):
        raise ValueError("fine_mix_scan: with a trigger every batch is a dict with the clean images under 'image' and the backdoor target under 'target'")
    if any(torch.is_tensor(t) and t.data_ptr() == model.flat_param.data_ptr() for t in (clean, backdoored)):
        raise ValueError("fine_mix_scan: clean and backdoored must be copies, not the network's own flat_param (every share overwrites it)")
    restore = model.flat_param.detach().clone()
    return _scan(model, restore, loss_fn, batches, data_seed, trigger, "keep", keeps, lambda v: fine_mix(model, clean, backdoored, v, seed))
