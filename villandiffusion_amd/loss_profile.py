"""The backdoor loss against the timestep, split into clean and poisoned samples: the reference's one diagnostic of this path (a loss-vs-t
plot), available for any model and batch.

For every requested timestep the WHOLE batch is noised at that timestep (the same noise each time: the curve shows the timestep alone), the
network runs once without gradients and one forward-only launch of the shaped loss kernel (``vd_loss_sample_fwd_bwd`` with ``dpred = NULL``)
returns the loss of every sample and the two class sums.  Results stay on the device until the last timestep is done."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from . import ops
from .loss import SDE_LDM, SDE_VE, SDE_VP, LossFn


def _check(model, loss_fn: LossFn):
    """NotImplementedError for what the profile is not built for, saying which."""
    from .ncsnpp import NCSNppModel
    from .unet import UNet2DModel
    sde = getattr(loss_fn, "_sde", None)
    if sde == SDE_LDM:
        raise NotImplementedError("loss_profile: SDE-LDM (latent diffusion) is not built: the batch would have to be encoded to latents first")
    if isinstance(model, UNet2DModel) and sde == SDE_VP:
        return
    if isinstance(model, NCSNppModel) and sde == SDE_VE:
        return
    raise NotImplementedError(f"loss_profile: {type(model).__name__} with a {sde} loss is not built (UNet2DModel with SDE-VP, NCSNppModel with SDE-VE)")


def loss_profile(model, loss_fn: LossFn, batch: Dict, timesteps: Iterable[int], noise_seed: int = 0, target_key: str = "target",
                 poison_key: str = "pixel_values") -> dict:
    """The UNWEIGHTED loss of `batch` at each of `timesteps`, by class -> {"timesteps", "loss_clean", "loss_poison" (means, None for a class
    without a sample), "n_clean", "n_poison", and "snr_weight" (the min-SNR weight of each timestep) when loss_fn has snr_gamma}.
    batch: the training batch keys (`target`, `pixel_values`, `is_clean`).  The model's weights and gradients are left alone."""
    _check(model, loss_fn)
    ts = [int(t) for t in timesteps]
    x0, R = batch[target_key], batch[poison_key]
    if "is_clean" not in batch:
        raise ValueError("loss_profile: the batch has no 'is_clean' flags to split by")
    T = len(loss_fn._sigmas_asc) if loss_fn._sde == SDE_VE else len(loss_fn._alphas_cumprod)
    if not ts or any(t < 0 or t >= T for t in ts):
        raise ValueError(f"loss_profile: timesteps must be a non-empty list inside [0, {T}), got {ts}")
    Bn = len(x0)
    if Bn == 0 or len(R) != Bn or torch.as_tensor(batch["is_clean"]).numel() != Bn:
        raise ValueError("loss_profile: target, poison residual and flags must hold the same (non-zero) number of samples")
    dev = model.device
    x0, R = x0.to(dev).float().contiguous(), R.to(dev).float().contiguous()
    flags = (~torch.as_tensor(batch["is_clean"]).bool()).reshape(Bn).to(dev).contiguous()
    noise = torch.empty_like(x0)
    ops.randn(noise, int(noise_seed) & 0x7FFFFFFFFFFFFFFF, 0)
    loss_fn._tables(dev)
    ws = torch.empty(ops.loss_sample_plan(Bn, x0[0].numel())[2], device=dev, dtype=torch.float32)
    stats = torch.empty(len(ts), 4, device=dev, dtype=torch.float32)
    loss, sample_loss = torch.empty(1, device=dev, dtype=torch.float32), torch.empty(Bn, device=dev, dtype=torch.float32)
    with torch.no_grad():
        for k, t in enumerate(ts):
            tt = torch.full((Bn,), t, device=dev, dtype=torch.int64)
            x_t, y = loss_fn.get_inputs_targets(x0, R, tt, noise)
            if loss_fn._sde == SDE_VE:
                sig = loss_fn._dev_tabs[3][tt].contiguous()
                pred, ps = model(x_t, sig, return_dict=False)[0], (-sig).contiguous()
            else:
                pred, ps = model(x_t, tt, return_dict=False)[0], None
            ops.loss_sample_fwd_bwd(pred.contiguous(), y, None, loss, ws, pscale=ps, flags=flags, sample_loss=sample_loss, stats=stats[k],
                                    kind=loss_fn._loss_type)
    st = stats.cpu().double()
    n_clean, n_poison = int(st[0, 1]), int(st[0, 3])
    out = {"timesteps": ts,
           "loss_clean": [float(r[0] / r[1]) if n_clean else None for r in st],
           "loss_poison": [float(r[2] / r[3]) if n_poison else None for r in st],
           "n_clean": n_clean, "n_poison": n_poison}
    wtab: Optional[torch.Tensor] = loss_fn.snr_table()
    if wtab is not None:
        out["snr_weight"] = [float(wtab[t]) for t in ts]
    return out
