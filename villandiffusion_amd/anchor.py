"""Anchored fine-tuning: a penalty that holds the weights of a fine-tune to the checkpoint it started from.

* L2-SP (Li et al. 2018):          lambda / 2 * sum_i (w_i - w0_i)^2
* EWC (Kirkpatrick et al. 2017):   lambda / 2 * sum_i F_i (w_i - w0_i)^2, F the diagonal Fisher information estimated on clean data -- what
  Selective Amnesia (Heng & Soh 2023) uses to unlearn in diffusion models without forgetting the rest.

`Trainer(anchor=AnchorConfig(...))` adds the penalty's gradient lambda * F * (w - w0) to the flat gradient with ONE launch per optimiser step
(ops.anchor_grad -> vd_anchor_grad), before the norm, so the global-norm clip sees the gradient of loss + penalty as autograd would give it.
`estimate_fisher` forms F with one launch per batch (ops.fisher_accum -> vd_fisher_accum) on the flat gradient buffer, which all three network
families share.  With micro-batches of ONE image F is the empirical Fisher, the mean of the squared per-sample gradients.  With b > 1 images per
batch it is the mean over the batches of the SQUARE OF THE BATCH-MEAN GRADIENT, the usual cheap approximation: smaller by up to a factor b, and
with less of the per-sample spread.
"""
from __future__ import annotations

import hashlib
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Iterable, Optional

import torch

ANCHOR_MODES = ("l2sp", "ewc")
NORMALIZE = ("none", "mean", "max")
FISHER_FILE = "fisher.pt"


@dataclass
class AnchorConfig:
    """lam: the penalty's weight lambda.  mode "l2sp": F = 1, no Fisher; "ewc": `fisher` is the flat float32 Fisher tensor (one entry per float of
    `flat_param`, as `estimate_fisher` returns and `load_fisher` reads)."""
    lam: float
    mode: str = "l2sp"
    fisher: Optional[torch.Tensor] = None

    def __post_init__(self):
        if isinstance(self.lam, bool) or not isinstance(self.lam, (int, float)) or not math.isfinite(self.lam) or self.lam <= 0:
            raise ValueError(f"AnchorConfig: lam must be a positive finite number, got {self.lam!r}")
        if self.mode not in ANCHOR_MODES:
            raise ValueError(f"AnchorConfig: mode must be one of {ANCHOR_MODES}, got {self.mode!r}")
        if self.mode == "ewc":
            if self.fisher is None:
                raise ValueError("AnchorConfig: mode 'ewc' needs a Fisher (fisher=estimate_fisher(...) or load_fisher(...))")
            if not torch.is_tensor(self.fisher) or self.fisher.dtype != torch.float32 or self.fisher.dim() != 1:
                raise ValueError("AnchorConfig: fisher must be a flat float32 tensor")
        elif self.fisher is not None:
            raise ValueError("AnchorConfig: mode 'l2sp' takes no Fisher (its F is 1); use mode='ewc'")


def check_anchor(anchor, lora=None, world: int = 1, conv_math: Optional[str] = None):
    """What an anchored trainer is not built for, each refusal saying which; pure host code, shared by Trainer and the drivers' setup()."""
    if anchor is None:
        return
    if not isinstance(anchor, AnchorConfig):
        raise TypeError(f"Trainer: anchor must be an AnchorConfig, got {type(anchor).__name__}")
    if lora is not None:
        raise ValueError("Trainer: anchor together with lora is not built (the base weights are frozen there; the penalty belongs on the adapter, "
                         "which the flat-buffer launch does not see)")
    if world > 1:
        raise NotImplementedError("Trainer: anchor in a process group of more than one rank is not built (the launch would have to follow the "
                                  "bucketed all-reduce, and no second rank is there to test it on)")
    if conv_math == "f16":
        raise NotImplementedError("Trainer: anchor with conv_math='f16' is not built (flat_grad holds the gradient times the loss scale there; the "
                                  "penalty's gradient would have to be scaled with it)")


# ---- the layout a Fisher belongs to -----------------------------------------------------------------------------------------------------------
def layout_digest(model) -> str:
    """sha256 over the ordered (name, offset, numel, shape) rows of the model's flat layout: `rows_sha256` of tests/golden/flat_layouts.json."""
    rows = [[name, model._offs[name][0], model._offs[name][1], list(shape)] for name, shape, _ in model._layout]
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


def family_of(model) -> str:
    return type(model).__name__


# ---- the estimate -----------------------------------------------------------------------------------------------------------------------------
def _timesteps_of(loss_fn) -> int:
    return len(loss_fn._sigmas_asc) if getattr(loss_fn, "_sde", None) == "SDE-VE" else len(loss_fn._alphas_cumprod)


def fisher_draws(shape, n_timesteps: int, seed: int, k: int):
    """(timesteps, noise) of batch k: drawn on the host from one generator seeded by (seed, k), timesteps first."""
    gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(k)) & 0x7FFFFFFFFFFFFFFF)
    t = torch.randint(0, n_timesteps, (shape[0],), generator=gen)
    return t, torch.randn(tuple(shape), generator=gen)


def normalize_fisher(F: torch.Tensor, normalize: str = "mean") -> torch.Tensor:
    """F divided once by its mean ("mean"), its maximum ("max") or left alone ("none"); raw values are tiny and lambda would be unusable
    otherwise.  Off the step path: a torch op on the flat tensor."""
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    if normalize == "none":
        return F
    d = F.mean(dtype=torch.float64) if normalize == "mean" else F.max().double()
    if not float(d) > 0 or not math.isfinite(float(d)):
        raise FloatingPointError(f"normalize_fisher: the Fisher's {normalize} is {float(d)!r}")
    return (F.double() / d).float()


def estimate_fisher(model, loss_fn, batches: Iterable, seed: int = 0, normalize: str = "mean") -> torch.Tensor:
    """The diagonal Fisher estimate of `model` on clean batches, a flat float32 tensor the size of `flat_param` on the model's device.

    batches: a sequence of clean image (or latent) tensors [b, C, H, W].  Per batch k: zero_grad; the clean loss as the trainer forms it
    (LossFn.p_loss with a zero poison residual) at the timesteps and noise of `fisher_draws(shape, T, seed, k)`; backward; one
    `ops.fisher_accum(F, flat_grad, 1 / K)`; after the last batch F is divided once as `normalize` says ("none": the raw estimate).  Nothing is
    read back until the end, the weights are never written, flat_grad is left zeroed and the loss function's grad_scale is put back.  Only
    flat_grad is touched, so every network family works.  b = 1 gives the empirical Fisher; b > 1 the mean square of the batch-mean
    gradient (see the module's text)."""
    from . import ops
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    batches = list(batches)
    if not batches:
        raise ValueError("estimate_fisher: no batches")
    if getattr(model, "conv_math", None) == "f16":
        raise NotImplementedError("estimate_fisher with conv_math='f16' is not built (flat_grad holds a scaled gradient there)")
    dev = model.device
    F = torch.zeros_like(model.flat_param)
    s = 1.0 / len(batches)
    T = _timesteps_of(loss_fn)
    kept, loss_fn.grad_scale = loss_fn.grad_scale, 1.0
    try:
        for k, x0 in enumerate(batches):
            x0 = x0.to(dev).float()
            t, eps = fisher_draws(x0.shape, T, seed, k)
            model.zero_grad()
            kw = {"is_poison": torch.zeros(len(x0), dtype=torch.bool, device=dev)} if getattr(loss_fn, "shaped", False) else {}
            loss = loss_fn.p_loss(model, x0, torch.zeros_like(x0), t.to(dev), noise=eps.to(dev), **kw)
            loss.backward()
            ops.fisher_accum(F, model.flat_grad, s)
    finally:
        loss_fn.grad_scale = kept
        model.zero_grad()
    return normalize_fisher(F, normalize)


def fisher_stats(F: torch.Tensor) -> Dict[str, float]:
    """mean, max and the share of entries below 1e-12 * max."""
    mx = float(F.max())
    return {"mean": float(F.mean(dtype=torch.float64)), "max": mx, "share_below_1e-12_max": float((F < 1e-12 * mx).double().mean())}


# ---- fisher.pt --------------------------------------------------------------------------------------------------------------------------------
def _fisher_path(path: str) -> str:
    return os.path.join(path, FISHER_FILE) if os.path.isdir(path) else path


def save_fisher(path: str, F: torch.Tensor, model, n_batches: int, batch: int, normalize: str) -> str:
    """fisher.pt: the tensor and what it was estimated on."""
    if F.dim() != 1 or F.numel() != model.flat_numel or F.dtype != torch.float32:
        raise ValueError(f"save_fisher: a flat float32 tensor of {model.flat_numel} entries is expected, got {tuple(F.shape)} {F.dtype}")
    path = _fisher_path(path)
    torch.save({"fisher": F.detach().to("cpu").clone(), "n_batches": int(n_batches), "batch": int(batch), "normalize": str(normalize),
                "family": family_of(model), "numel": int(model.flat_numel), "layout_sha256": layout_digest(model)}, path)
    return path


def load_fisher(path: str, model=None, with_meta: bool = False):
    """The tensor of a fisher.pt (`path`: the file, or a directory that holds one), on the host.  With a model, a file whose numel or layout
    digest differs from the model's raises, naming both."""
    path = _fisher_path(path)
    d = torch.load(path, map_location="cpu")
    if not isinstance(d, dict) or not {"fisher", "numel", "layout_sha256"} <= set(d):
        raise ValueError(f"load_fisher: {path} is no fisher.pt (save_fisher writes fisher / numel / layout_sha256 / ...)")
    F = d["fisher"]
    if not torch.is_tensor(F) or F.dtype != torch.float32 or F.dim() != 1 or F.numel() != int(d["numel"]):
        raise ValueError(f"load_fisher: {path} holds no flat float32 tensor of its recorded {d['numel']} entries")
    if model is not None:
        if int(d["numel"]) != int(model.flat_numel):
            raise ValueError(f"load_fisher: {path} was estimated on a {d.get('family', '?')} of {int(d['numel'])} floats; this "
                             f"{family_of(model)} has {int(model.flat_numel)}")
        if d["layout_sha256"] != layout_digest(model):
            raise ValueError(f"load_fisher: {path} was estimated on a {d.get('family', '?')} whose parameter layout has the digest "
                             f"{d['layout_sha256'][:12]}...; this {family_of(model)} has {layout_digest(model)[:12]}... (other names or offsets)")
    return (F, {k: v for k, v in d.items() if k != "fisher"}) if with_meta else F
