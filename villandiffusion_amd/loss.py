"""Backdoor (poisoned) noise-prediction loss on MI355X -- same surface as the reference's ``loss.LossFn``
(loss.py:825-1006) and the coefficient helpers (loss.py:466-588).

What changed under the surface
* the (step, coef) correction tables (L1-L3 in SURVEY.md §8a) are built ONCE on the host with the reference's fp32 op
  sequence and kept on the device (the reference rebuilds them every step, loss.py:917);
* q-sample + backdoor shift + target (L4) is ONE kernel (``vd_qsample_backdoor``) and MSE forward+backward (L5)
  is ONE kernel pair (``vd_mse_fwd_bwd``); ``loss.backward()`` then drives the UNet's explicit backward;
* a *shaped* loss (``snr_gamma`` / ``poison_weight`` / ``track_split``, all off by default) runs ``vd_loss_sample_fwd_bwd`` in its place: a
  weight per sample in, the loss of every sample and the clean / poisoned split out, still one fused gradient.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from . import ops

SDE_VP, SDE_VE, SDE_LDM = "SDE-VP", "SDE-VE", "SDE-LDM"


# ---------------------------------------------------------------------------------------------- coefficient tables
def get_hs_vp(alphas: torch.Tensor, alphas_cumprod: torch.Tensor) -> torch.Tensor:
    """h_0 = sqrt(1-abar_0); res_i = sqrt(a_i)(h_{i-1}+res_{i-1}); h_i = sqrt(1-abar_i) - res_i  (loss.py:551-559).
    Sequential recurrence on fp32 0-d CPU tensors -- deliberately the SAME torch scalar kernels the reference runs
    (torch's CPU `x ** 0.5` is not always the correctly rounded sqrt, so e.g. numpy float32 would differ in the last bit).
    Runs once per LossFn (the reference caches it too, loss.py:872-874)."""
    a, ac = alphas.detach().float().cpu(), alphas_cumprod.detach().float().cpu()
    h = [(1 - ac[0]) ** 0.5]
    res = torch.zeros(())
    for i in range(1, len(a)):
        res = (a[i] ** 0.5) * (h[i - 1] + res)
        h.append((1 - ac[i]) ** 0.5 - res)
    return torch.stack(h)


def get_ws_ve(sigmas: torch.Tensor) -> torch.Tensor:
    """loss.py:466-474."""
    s_ = sigmas.detach().float().cpu()
    w = [s_[0]]
    res = torch.zeros(())
    for i in range(1, len(s_)):
        res = w[i - 1] ** 2 + res
        w.append((s_[i] ** 2 - res) ** 0.5)
    return torch.stack(w)


def get_hs_ve(rhos_hat: torch.Tensor) -> torch.Tensor:
    """loss.py:476-484."""
    r = rhos_hat.detach().float().cpu()
    h = [r[0]]
    res = torch.zeros(())
    for i in range(1, len(r)):
        res = h[i - 1] + res
        h.append(r[i] - res)
    return torch.stack(h)


def _solver(step, coef, solver_type):
    s = str(solver_type).lower()
    if s == "ode":
        return step, 2 * coef
    if s == "sde":
        return step, coef
    raise NotImplementedError(f"Coefficient solver_type: {solver_type} isn't implemented")


def get_R_coef_gen_vp(alphas_cumprod, alphas, hs=None, psi: float = 1, solver_type: str = "sde", vp_scale: float = 1.0,
                      ve_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """BadDiffusion (psi=1) / TrojDiff (psi=0) correction tables and their psi-blend (loss.py:561-588)."""
    one_m_ac_sqrt = (1 - alphas_cumprod) ** 0.5
    step_b = 1 - alphas_cumprod ** 0.5
    coef_b = vp_scale * (1 - alphas ** 0.5) * one_m_ac_sqrt / (1 - alphas)
    if psi == 1:
        return _solver(step_b, coef_b, solver_type)
    if hs is None:
        raise ValueError(f"Argument hs shouldn't be {hs} when psi is {psi}")
    coef_t = -ve_scale * ((alphas ** 0.5 - 1) * one_m_ac_sqrt * (1 - alphas) - hs * (alphas - alphas_cumprod)) / (1 - alphas)
    return _solver(psi * step_b + (1 - psi) * one_m_ac_sqrt, psi * coef_b + (1 - psi) * coef_t, solver_type)


def get_R_coef_gen_ve_reduce(sigmas, hs=None, rhos_hat_w: float = 1.0, psi: float = 1, solver_type: str = "sde",
                             vp_scale: float = 1.0, ve_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """loss.py:519-549."""
    if psi != 0:
        raise NotImplementedError("Variance Explode model doesn't support BadDiffusion style correction term")
    prev = torch.roll(sigmas, 1, 0)
    prev[0] = 0
    return _solver(rhos_hat_w * sigmas, ve_scale * (sigmas * rhos_hat_w / (sigmas + prev)), solver_type)


# ---------------------------------------------------------------------------------------------- min-SNR weights
def min_snr_table(alphas_cumprod: torch.Tensor, gamma: float) -> torch.Tensor:
    """Min-SNR-gamma weights of an epsilon-prediction loss, one per timestep: snr = abar / (1 - abar), w = min(snr, gamma) / snr, in float32
    torch ops on the host.  Exactly 1 wherever snr <= gamma (x / x), below 1 at the low-noise timesteps."""
    ac = alphas_cumprod.detach().float().cpu()
    snr = ac / (1 - ac)
    return torch.minimum(snr, torch.tensor(float(gamma), dtype=torch.float32)) / snr


def check_shaping(snr_gamma, poison_weight, sde_type=None):
    """The argument errors of the shaped loss, raised before any launch."""
    if snr_gamma is not None:
        if sde_type == SDE_VE:
            raise NotImplementedError("snr_gamma with SDE-VE isn't implemented: the VE loss already carries its own sigma weighting")
        if not (isinstance(snr_gamma, (int, float)) and math.isfinite(snr_gamma) and snr_gamma > 0):
            raise ValueError(f"snr_gamma must be a finite number > 0, got {snr_gamma!r}")
    if not (isinstance(poison_weight, (int, float)) and math.isfinite(poison_weight) and poison_weight >= 0):
        raise ValueError(f"poison_weight must be a finite number >= 0, got {poison_weight!r}")


# ---------------------------------------------------------------------------------------------- fused MSE
class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, y, pscale, gscale, partial, kind="l2"):
        dpred = torch.empty_like(pred)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        ops.mse_fwd_bwd(pred.contiguous(), y, dpred, loss, partial, pscale=pscale, gscale=gscale, kind=kind)
        ctx.save_for_backward(dpred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None, None


class _ShapedLoss(torch.autograd.Function):
    """_MSE for a shaped LossFn: the same one-pass forward + gradient through vd_loss_sample_fwd_bwd."""

    @staticmethod
    def forward(ctx, pred, y, pscale, lf, timesteps, flags, weight):
        dpred = torch.empty_like(pred)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        lf.shaped_launch(pred.contiguous(), y, dpred, loss, pscale, timesteps, flags, weight)
        ctx.save_for_backward(dpred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None, None, None


class LossFn:
    """Drop-in for the reference's ``LossFn`` (same constructor and ``p_loss`` / ``p_loss_by_keys`` signatures)."""
    RANDN_BOUND: float = 2.5

    def __init__(self, noise_sched, sde_type: str, loss_type: str = "l2", psi: float = 1, solver_type: str = "sde",
                 vp_scale: float = 1.0, ve_scale: float = 1.0, rhos_hat_w: float = 1.0, rhos_hat_b: float = 0.0,
                 snr_gamma: Optional[float] = None, poison_weight: float = 1.0, track_split: bool = False):
        """snr_gamma / poison_weight / track_split (after the reference's arguments) shape the loss: min-SNR-gamma weights by timestep
        (VP / LDM), a weight on the poisoned samples, and the clean / poisoned split kept in ``last_split``.  All at their defaults: the loss
        of the reference, through the kernels it always ran."""
        if sde_type not in (SDE_VP, SDE_VE, SDE_LDM):
            raise NotImplementedError(f"sde_type: {sde_type} isn't implemented")
        if loss_type not in ops.LOSS_KINDS:       # loss.py:849-858: l1 / l2 / huber, anything else raises
            raise NotImplementedError(f"loss_type: {loss_type} isn't implemented")
        check_shaping(snr_gamma, poison_weight, sde_type)
        self.snr_gamma, self.poison_weight, self.track_split = snr_gamma, poison_weight, bool(track_split)
        self.last_sample_loss: Optional[torch.Tensor] = None      # [B] unweighted per-sample losses of the last shaped call (device, no sync)
        self.last_split: Optional[torch.Tensor] = None            # [4] {sum l clean, n clean, sum l poisoned, n poisoned} of it
        self._wtab = None                                         # (gamma, {device: table})
        self._ws = None
        self._loss_type = loss_type
        self._sched, self._sde, self._psi, self._solver = noise_sched, sde_type, psi, solver_type
        # the schedule is captured HERE like the reference does (loss.py:829-834): a VE pipeline's set_sigmas(n) later
        # replaces noise_sched.sigmas by the n-step inference table, which must not shrink the training tables
        if sde_type == SDE_VE:
            self._sigmas_asc = noise_sched.sigmas.flip([0]).float().cpu().clone()
        else:
            self._alphas = noise_sched.alphas.float().cpu().clone()
            self._alphas_cumprod = noise_sched.alphas_cumprod.float().cpu().clone()
        self._vp_scale, self._ve_scale, self._w, self._b = vp_scale, ve_scale, rhos_hat_w, rhos_hat_b
        self._dev_tabs = None
        self._partial = None
        self.grad_scale = 1.0            # trainer sets 1/gradient_accumulation_steps (accelerator.backward semantics)
        self.noise_seed: Optional[int] = None
        self._noise_off = 0

    # host tables (fp32, CPU) -- loss.py:860-907
    def get_R_step_coef(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._sde in (SDE_VP, SDE_LDM):
            a, ac = self._alphas, self._alphas_cumprod
            hs = get_hs_vp(a, ac) if self._psi != 1 else None
            return get_R_coef_gen_vp(ac, a, hs=hs, psi=self._psi, solver_type=self._solver, vp_scale=self._vp_scale,
                                     ve_scale=self._ve_scale)
        sig = self._sigmas_asc
        return get_R_coef_gen_ve_reduce(sig, hs=True, rhos_hat_w=self._w, psi=self._psi, solver_type=self._solver,
                                        ve_scale=self._ve_scale)

    def _tables(self, dev):
        if self._dev_tabs is None or self._dev_tabs[0].device != dev:
            step, coef = self.get_R_step_coef()
            if self._sde in (SDE_VP, SDE_LDM):
                ac = self._alphas_cumprod
                ta, ts = ac ** 0.5, (1 - ac) ** 0.5
                self._dev_tabs = (step.to(dev), coef.to(dev), ta.to(dev), ts.to(dev))
            else:
                self._dev_tabs = (step.to(dev), coef.to(dev), None, self._sigmas_asc.to(dev))
            self._partial = torch.empty(1024, device=dev, dtype=torch.float32)
        return self._dev_tabs

    # ---- shaping -----------------------------------------------------------------------------------------------------------------
    @property
    def shaping(self) -> Tuple:
        """(snr_gamma, poison_weight, track_split): what a captured micro-step was recorded with."""
        return (self.snr_gamma, self.poison_weight, self.track_split)

    @property
    def shaped(self) -> bool:
        return self.snr_gamma is not None or self.poison_weight != 1.0 or self.track_split

    def snr_table(self, dev=None) -> Optional[torch.Tensor]:
        """The min-SNR-gamma table [T] (None without snr_gamma): built once per gamma on the host, kept on `dev` beside the other tables."""
        if self.snr_gamma is None:
            return None
        check_shaping(self.snr_gamma, self.poison_weight, self._sde)
        dev = torch.device("cpu") if dev is None else torch.device(dev)
        if self._wtab is None or self._wtab[0] != self.snr_gamma:
            self._wtab = (self.snr_gamma, {})
        tabs = self._wtab[1]                          # one per device, never replaced: a captured micro-step holds the device one's address
        if dev not in tabs:
            tabs[dev] = min_snr_table(self._alphas_cumprod, self.snr_gamma).to(dev).contiguous()
        return tabs[dev]

    def shaped_flags(self, is_poison, Bn: int, dev) -> Optional[torch.Tensor]:
        """The poison flags [B] as device bytes; a poison weight or the split without them is an error (raised before any launch)."""
        check_shaping(self.snr_gamma, self.poison_weight, self._sde)
        if is_poison is None:
            if self.poison_weight != 1.0 or self.track_split:
                raise ValueError("LossFn: poison_weight != 1 or track_split needs the poison flags (is_poison=..., or batch['is_clean'])")
            return None
        flags = torch.as_tensor(is_poison)
        if flags.numel() != Bn:
            raise ValueError(f"LossFn: is_poison has {flags.numel()} entries for a batch of {Bn}")
        return (flags != 0).reshape(Bn).to(dev).contiguous()

    def shaped_launch(self, pred, y, dpred, loss, pscale, timesteps, flags, weight=None, ws=None):
        """One vd_loss_sample_fwd_bwd launch with this LossFn's shaping (dpred None: forward only); leaves last_sample_loss / last_split."""
        dev, Bn = pred.device, pred.shape[0]
        if ws is None:
            need = ops.loss_sample_plan(Bn, pred.numel() // Bn)[2]
            if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
                self._ws = torch.empty(need, device=dev, dtype=torch.float32)
            ws = self._ws
        wtab = self.snr_table(dev)
        sample_loss = torch.empty(Bn, device=dev, dtype=torch.float32)
        stats = torch.empty(4, device=dev, dtype=torch.float32)
        ops.loss_sample_fwd_bwd(pred, y, dpred, loss, ws, pscale=pscale, weight=weight, wtab=wtab,
                                t=timesteps.to(device=dev, dtype=torch.int64).contiguous() if wtab is not None else None, flags=flags,
                                poison_weight=self.poison_weight, sample_loss=sample_loss, stats=stats, gscale=self.grad_scale,
                                kind=self._loss_type)
        self.last_sample_loss, self.last_split = sample_loss, stats
        return loss

    def get_inputs_targets(self, x_start, R, timesteps, noise):
        """(x_t, y) of loss.py:909-939 in one kernel."""
        dev = x_start.device
        step, coef, ta, ts = self._tables(dev)
        x_t, y = torch.empty_like(x_start), torch.empty_like(x_start)
        ops.qsample_backdoor(x_start.contiguous(), R.contiguous(), noise.contiguous(),
                             timesteps.to(device=dev, dtype=torch.int64).contiguous(), ta, ts, step, coef, x_t, y)
        return x_t, y

    def _noise(self, x):
        if self.noise_seed is None:
            self.noise_seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        z = torch.empty_like(x)
        ops.randn(z, self.noise_seed, self._noise_off)
        self._noise_off += (x.numel() + 3) // 4
        return z

    def p_loss(self, model, x_start: torch.Tensor, R: torch.Tensor, timesteps: torch.Tensor, noise: torch.Tensor = None,
               is_poison: Optional[torch.Tensor] = None, sample_weight: Optional[torch.Tensor] = None):
        """is_poison [B] (bool): the samples poison_weight and the split apply to; sample_weight [B]: an explicit weight per sample.  Either
        one makes this call a shaped one."""
        if len(x_start) == 0:
            return 0
        dev = model.device if hasattr(model, "device") else x_start.device
        shaped = self.shaped or sample_weight is not None
        if shaped:                                    # every argument error before the first launch
            flags = self.shaped_flags(is_poison, len(x_start), dev)
            if sample_weight is not None:
                if sample_weight.numel() != len(x_start):
                    raise ValueError(f"LossFn: sample_weight has {sample_weight.numel()} entries for a batch of {len(x_start)}")
                sample_weight = sample_weight.to(dev).float().reshape(-1).contiguous()
        x_start, R = x_start.to(dev).float(), R.to(dev).float()
        timesteps = timesteps.to(dev)
        if noise is None:
            noise = self._noise(x_start)
        x_t, y = self.get_inputs_targets(x_start, R, timesteps, noise.to(dev))
        if self._sde in (SDE_VP, SDE_LDM):
            pred = model(x_t, timesteps.contiguous(), return_dict=False)[0]
            if shaped:
                return _ShapedLoss.apply(pred, y, None, self, timesteps, flags, sample_weight)
            return _MSE.apply(pred, y, None, self.grad_scale, self._partial, self._loss_type)
        sig_t = self._dev_tabs[3][timesteps]
        pred = model(x_t, sig_t.contiguous(), return_dict=False)[0]
        if shaped:
            return _ShapedLoss.apply(pred, y, (-sig_t).contiguous(), self, timesteps, flags, sample_weight)
        return _MSE.apply(pred, y, (-sig_t).contiguous(), self.grad_scale, self._partial, self._loss_type)

    def p_loss_by_keys(self, batch, model, target_latent_key, poison_latent_key, timesteps, vae=None, noise=None,
                       weight_dtype=None, scaling_factor=None):
        x0, R = batch[target_latent_key], batch[poison_latent_key]
        if vae is not None:          # loss.py:942-970: encode on the fly (training itself passes vae=None + precomputed latents)
            x0, R = self.encode_latents(vae, x0, scaling_factor), self.encode_latents(vae, R, scaling_factor)
        is_poison = None
        if self.shaped and "is_clean" in batch:      # (an unshaped loss never looks at the flags: not one more launch)
            is_poison = ~torch.as_tensor(batch["is_clean"]).bool()
        return self.p_loss(model=model, x_start=x0, R=R, timesteps=timesteps, noise=noise, is_poison=is_poison)

    @staticmethod
    def encode_latents(vae, x: torch.Tensor, scaling_factor: Optional[float] = None) -> torch.Tensor:
        """loss.py:941-950  vae.encode(x).latents (* scaling_factor), detached."""
        lat = vae.encode(x).latents
        if scaling_factor is not None:
            lat = lat * scaling_factor
        return lat.detach()

    @staticmethod
    def decode_latents(vae, x: torch.Tensor, scaling_factor: Optional[float] = None) -> torch.Tensor:
        """loss.py:951-962  vae.decode(x).sample (/ scaling_factor), detached."""
        out = vae.decode(x).sample
        if scaling_factor is not None:
            out = out / scaling_factor
        return out.detach()
