"""Mode Connectivity Repair (Zhao et al., ICLR 2020, on the curves of Garipov et al., NeurIPS 2018): a post-hoc repair from two checkpoints of one
architecture -- two backdoored models, or a backdoored model and its fine-tuned copy -- and a little clean data.

A one-bend curve phi(t), t in [0, 1], joins the flat weight buffers A (t = 0) and B (t = 1) through a trainable bend theta:

* "bezier":     phi(t) = (1 - t)^2 A + 2 t (1 - t) theta + t^2 B
* "polychain":  A -> theta on [0, 1/2], theta -> B on [1/2, 1]

Every point is ca(t) A + cm(t) theta + cb(t) B, ONE launch over the flat buffers (ops.curve_point -> vd_curve_point) with no temporary.  The bend
is trained on clean data so that the loss stays low along the whole curve: every optimiser step draws a t, the network holds phi(t), and the
bend's gradient is cm(t) * dL/dphi -- `vd_adam_step` on theta with inv_scale = cm, no third kernel.  The repaired model is the point at an
interior t (`CurveAdam.hold`, tools/mcr_repair.py), chosen by the loss along the curve (`curve_scan`): the endpoints carry the backdoor,
interior points keep the clean behaviour and tend to lose it.  `curve_step` is one eager optimiser step of that training; the curve is not a
mode of `trainer.Trainer`.

The networks use GroupNorm: MCR's second stage, re-estimating BatchNorm statistics at the chosen t, does not exist here.  Only flat_param and
flat_grad are touched, so UNet2DModel, NCSNppModel and the latent UNet all work."""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from .anchor import _timesteps_of, family_of, fisher_draws, layout_digest

CURVE_KINDS = ("bezier", "polychain")
CURVE_FILE = "curve.pt"


@dataclass
class CurveConfig:
    """kind: "bezier" or "polychain" (one bend each).  seed: of the host generator the training t are drawn from.  [t_min, t_max]: the range of
    those draws, inside [0, 1]."""
    kind: str = "bezier"
    seed: int = 0
    t_min: float = 0.0
    t_max: float = 1.0

    def __post_init__(self):
        if self.kind not in CURVE_KINDS:
            raise ValueError(f"CurveConfig: kind must be one of {CURVE_KINDS}, got {self.kind!r}")
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or self.seed < 0:
            raise ValueError(f"CurveConfig: seed must be a non-negative integer, got {self.seed!r}")
        for name in ("t_min", "t_max"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not 0.0 <= v <= 1.0:
                raise ValueError(f"CurveConfig: {name} must be a number in [0, 1], got {v!r}")
        if self.t_min > self.t_max:
            raise ValueError(f"CurveConfig: t_min = {self.t_min!r} lies above t_max = {self.t_max!r}")


# ---- the curve's algebra: host code, float64 ---------------------------------------------------------------------------------------------------
def _f32(v: float) -> float:
    return ctypes.c_float(v).value


def coefficients64(kind: str, t: float) -> Tuple[float, float, float]:
    """(ca, cm, cb) of phi(t) = ca A + cm theta + cb B in float64."""
    if kind not in CURVE_KINDS:
        raise ValueError(f"curve kind must be one of {CURVE_KINDS}, got {kind!r}")
    t = float(t)
    if not 0.0 <= t <= 1.0:                             # NaN fails too
        raise ValueError(f"curve: t must lie in [0, 1], got {t!r}")
    if kind == "bezier":
        return (1.0 - t) * (1.0 - t), 2.0 * t * (1.0 - t), t * t
    if t <= 0.5:
        return 1.0 - 2.0 * t, 2.0 * t, 0.0
    return 0.0, 2.0 - 2.0 * t, 2.0 * t - 1.0


def coefficients(kind: str, t: float) -> Tuple[float, float, float]:
    """(ca, cm, cb) computed in float64, each then rounded once to float32: the three values the kernel receives, and the oracle uses."""
    return tuple(_f32(c) for c in coefficients64(kind, t))


_GL = np.polynomial.legendre.leggauss(32)


def bezier_length(sq_a: float, sq_b: float, sq_c: float) -> float:
    """The arc length of the quadratic Bezier curve through (A, theta, B) from the squared sides sq_a = |theta - A|^2, sq_b = |theta - B|^2,
    sq_c = |A - B|^2 alone (the curve lies in the plane of its three points), in float64.

    phi'(t) = 2 (u + t a) with u = theta - A, a = A - 2 theta + B, so |phi'(t)|^2 = 4 (alpha t^2 + 2 beta t + gamma) with
    alpha = |a|^2 = 2 sq_a + 2 sq_b - sq_c, beta = a.u = (sq_c - sq_a - sq_b) / 2 - sq_a, gamma = sq_a.  With t0 = -beta / alpha and
    d^2 = (alpha gamma - beta^2) / alpha^2 the speed is 2 sqrt(alpha) sqrt((t - t0)^2 + d^2), whose antiderivative is
    G(s) = (s sqrt(s^2 + d^2) + d^2 asinh(s / d)) / 2 (d = 0: s |s| / 2).  Where the branch points t0 +- i d lie two or more away from [0, 1]
    (a nearly straight curve: G's two terms would cancel) the smooth speed is integrated by 32-point Gauss-Legendre instead."""
    sq_a, sq_b, sq_c = float(sq_a), float(sq_b), float(sq_c)
    alpha = max(2.0 * sq_a + 2.0 * sq_b - sq_c, 0.0)
    beta = 0.5 * (sq_c - sq_a - sq_b) - sq_a            # (u.v - |u|^2, v = B - theta; exact where the sides make it a power of two times sq_a)
    gamma = max(sq_a, 0.0)
    if alpha == 0.0:                                    # theta on the chord's midpoint (or all three equal): beta^2 <= alpha gamma = 0,
        return 2.0 * math.sqrt(gamma)                   # constant speed
    far = alpha * alpha == 0.0                          # (an alpha whose square underflows: as straight as float64 can tell)
    if not far:
        t0 = -beta / alpha
        d2 = max(alpha * gamma - beta * beta, 0.0) / (alpha * alpha)
        far = math.hypot(max(0.0, -t0, t0 - 1.0), math.sqrt(d2)) >= 2.0
    if far:
        x = 0.5 * (_GL[0] + 1.0)
        return float(np.sum(_GL[1] * np.sqrt(np.maximum((alpha * x + 2.0 * beta) * x + gamma, 0.0))))      # 2 * (1/2) * sum w sqrt(Q)

    def G(s):
        return 0.5 * (s * math.sqrt(s * s + d2) + (d2 * math.asinh(s / math.sqrt(d2)) if d2 > 0.0 else 0.0))

    return 2.0 * math.sqrt(alpha) * (G(1.0 - t0) - G(-t0))


def curve_length(kind: str, sq_a: float, sq_b: float, sq_c: float) -> float:
    """Arc length from the three squared sides: the polychain's is leg_a + leg_b."""
    if kind not in CURVE_KINDS:
        raise ValueError(f"curve kind must be one of {CURVE_KINDS}, got {kind!r}")
    if kind == "polychain":
        return math.sqrt(max(float(sq_a), 0.0)) + math.sqrt(max(float(sq_b), 0.0))
    return bezier_length(sq_a, sq_b, sq_c)


def geometry_of(kind: str, sq_a: float, sq_b: float, sq_c: float) -> Dict[str, float]:
    """The read-out of `Curve.geometry` from the three sums, float64."""
    sq_a, sq_b, sq_c = (max(float(v), 0.0) for v in (sq_a, sq_b, sq_c))
    return {"leg_a": math.sqrt(sq_a), "leg_b": math.sqrt(sq_b), "chord": math.sqrt(sq_c),
            "bend_offset": math.sqrt(max(0.5 * sq_a + 0.5 * sq_b - 0.25 * sq_c, 0.0)), "length": curve_length(kind, sq_a, sq_b, sq_c)}


def draw_t(gen: torch.Generator, cfg: CurveConfig) -> float:
    """One training t: t_min + (t_max - t_min) * u with u one float64 uniform draw of the host generator."""
    return cfg.t_min + (cfg.t_max - cfg.t_min) * torch.rand(1, generator=gen, dtype=torch.float64).item()


# ---- the curve on the device -------------------------------------------------------------------------------------------------------------------
class Curve:
    """The endpoints `wa`, `wb` and the bend `theta` of one curve, flat float32 buffers on the model's device.  theta starts at the chord's
    midpoint (one launch with the coefficients (0.5, 0, 0.5)) unless one is given."""

    def __init__(self, model, end_a: torch.Tensor, end_b: torch.Tensor, cfg: Optional[CurveConfig] = None, theta: Optional[torch.Tensor] = None):
        from . import ops
        cfg = CurveConfig() if cfg is None else cfg
        if not isinstance(cfg, CurveConfig):
            raise TypeError(f"Curve: cfg must be a CurveConfig, got {type(cfg).__name__}")
        n = int(model.flat_numel)
        for what, v in (("end_a", end_a), ("end_b", end_b), ("theta", theta)):
            if v is None and what == "theta":
                continue
            if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != n:
                got = f"{tuple(v.shape)} {v.dtype}" if torch.is_tensor(v) else type(v).__name__
                raise ValueError(f"Curve: {what} must be a flat float32 tensor of the model's {n} floats (model.flat_numel), got {got}")
        self.model, self.cfg = model, cfg
        dev = model.flat_param.device
        self.wa = end_a.detach().to(dev).clone().contiguous()
        self.wb = end_b.detach().to(dev).clone().contiguous()
        self._partial = torch.empty(3 * 1024, device=dev, dtype=torch.float32)
        self._out3 = torch.zeros(3, device=dev, dtype=torch.float32)
        if theta is None:
            self.theta = torch.empty_like(self.wa)
            ops.curve_point(self.theta, self.wa, self.wa, self.wb, 0.5, 0.0, 0.5, weights=False)
        else:
            self.theta = theta.detach().to(dev).clone().contiguous()
        self._prints: Optional[Tuple[int, int]] = None

    @property
    def kind(self) -> str:
        return self.cfg.kind

    def point(self, t: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """phi(t) into `out`, or (out None) into the network's flat_param: one launch.  The latter is a raw write of the weights, so what the
        network derived from them is dropped (`model.weights_changed()`)."""
        from . import ops
        ca, cm, cb = coefficients(self.cfg.kind, t)
        if out is not None:
            return ops.curve_point(out, self.wa, self.theta, self.wb, ca, cm, cb, weights=False)
        ops.curve_point(self.model.flat_param, self.wa, self.theta, self.wb, ca, cm, cb, weights=True)
        self.model.weights_changed()
        return self.model.flat_param

    def sums(self) -> Tuple[float, float, float]:
        """(sum (theta - A)^2, sum (theta - B)^2, sum (A - B)^2): one launch, read back."""
        from . import ops
        ops.curve_geometry(self.wa, self.theta, self.wb, self._partial, self._out3)
        return tuple(float(v) for v in self._out3.cpu())

    def geometry(self) -> Dict[str, float]:
        """leg_a = |theta - A|, leg_b = |theta - B|, chord = |A - B|, bend_offset = the distance of theta from the chord's midpoint, and the
        curve's arc length, all from the three sums of one vd_curve_geometry launch (synchronises)."""
        return geometry_of(self.cfg.kind, *self.sums())

    def fingerprints(self) -> Tuple[int, int]:
        """Of the two endpoints: the float32 bits of vd_l2norm_sq over each, reproducible, one launch each (computed once)."""
        if self._prints is None:
            self._prints = (fingerprint(self.wa), fingerprint(self.wb))
        return self._prints

    def save(self, path: str) -> str:
        """curve.pt: the bend and what it belongs to.  The endpoints themselves are not stored (two more copies of the network; whoever loads
        brings them, and their fingerprints are checked)."""
        path = os.path.join(path, CURVE_FILE) if os.path.isdir(path) else path
        torch.save({"theta": self.theta.detach().to("cpu").clone(), "kind": self.cfg.kind, "numel": int(self.model.flat_numel),
                    "layout_sha256": layout_digest(self.model), "family": family_of(self.model), "fingerprints": list(self.fingerprints())}, path)
        return path


def fingerprint(w: torch.Tensor) -> int:
    """The float32 bits of vd_l2norm_sq over a flat device buffer, as an int."""
    from . import ops
    partial = torch.empty(1024, device=w.device, dtype=torch.float32)
    out = torch.zeros(1, device=w.device, dtype=torch.float32)
    ops.l2norm_sq(w, partial, out)
    return int(out.view(torch.int32).item())


def load_curve(path: str, model, end_a: torch.Tensor, end_b: torch.Tensor, cfg: Optional[CurveConfig] = None) -> Curve:
    """The curve of a curve.pt (`path`: the file, or a directory that holds one) between the given endpoints.  A file written for another size,
    layout or endpoint raises, naming both.  cfg: the seed and range of further training; its kind must be the file's (None: the file's)."""
    path = os.path.join(path, CURVE_FILE) if os.path.isdir(path) else path
    d = torch.load(path, map_location="cpu")
    if not isinstance(d, dict) or not {"theta", "kind", "numel", "layout_sha256", "fingerprints"} <= set(d):
        raise ValueError(f"load_curve: {path} is no curve.pt (Curve.save writes theta / kind / numel / layout_sha256 / fingerprints / ...)")
    if int(d["numel"]) != int(model.flat_numel):
        raise ValueError(f"load_curve: {path} was trained on a {d.get('family', '?')} of {int(d['numel'])} floats; this {family_of(model)} has "
                         f"{int(model.flat_numel)}")
    if d["layout_sha256"] != layout_digest(model):
        raise ValueError(f"load_curve: {path} was trained on a {d.get('family', '?')} whose parameter layout has the digest "
                         f"{d['layout_sha256'][:12]}...; this {family_of(model)} has {layout_digest(model)[:12]}... (other names or offsets)")
    if cfg is None:
        cfg = CurveConfig(kind=d["kind"])
    elif cfg.kind != d["kind"]:
        raise ValueError(f"load_curve: {path} holds a {d['kind']!r} curve; the configuration asks for {cfg.kind!r}")
    curve = Curve(model, end_a, end_b, cfg, theta=d["theta"])
    check_fingerprints(curve, d["fingerprints"], f"load_curve: {path}")
    return curve


def check_fingerprints(curve: Curve, recorded: Sequence[int], who: str):
    got = curve.fingerprints()
    for name, have, want in zip(("end_a", "end_b"), got, recorded):
        if int(have) != int(want):
            raise ValueError(f"{who} was written between other endpoints: its {name} has the fingerprint {int(want):#010x}, the given one "
                             f"{int(have):#010x} (the float32 bits of the endpoint's squared norm; swapped or other checkpoints?)")


# ---- the optimiser -----------------------------------------------------------------------------------------------------------------------------
class CurveAdam:
    """`trainer.FusedAdam`'s interface over the bend only: torch.optim.Adam(betas=(0.9, 0.999), eps=1e-8) on theta with the global-norm clip of
    theta's gradient cm * dL/dphi, as `clip_grad_norm_` would see it.  One `step()`: `vd_l2norm_sq` over flat_grad, `vd_adam_step` on theta with
    inv_scale = grad_inv_scale * cm (exactly the clip and the update of the gradient cm * g), the draw of the next t, and `Curve.point(t)`
    into flat_param.

    The t sequence comes from one host generator seeded with cfg.seed.  The FIRST draw happens here, at construction: the network then holds
    phi(t0), and THE WEIGHTS IT HELD BEFORE ARE OVERWRITTEN.  One further draw follows every optimiser step, so all micro-batches of an
    accumulation window see the same t.  `self.t` is the t of the point the network holds."""
    ema = None
    ema_cfg = None
    ema_step = 0

    def __init__(self, curve: Curve, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: Optional[float] = 1.0):
        self.curve, self.model = curve, curve.model
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.exp_avg = torch.zeros_like(curve.theta)
        self.exp_avg_sq = torch.zeros_like(curve.theta)
        self.step_count = 0
        dev = curve.theta.device
        self._partial = torch.empty(1024, device=dev, dtype=torch.float32)
        self.grad_norm_sq = torch.zeros(1, device=dev, dtype=torch.float32)
        self.skipped = torch.zeros(1, device=dev, dtype=torch.int32)
        self.gen = torch.Generator().manual_seed(int(curve.cfg.seed))
        self._cm_last = 0.0                               # cm of the point the last step's gradient was taken at
        self.hold(draw_t(self.gen, curve.cfg))

    def hold(self, t: float):
        """The network takes phi(t): one launch; `self.t` and the cm of the next step's gradient follow."""
        self.curve.point(t)
        self.t = float(t)
        self.cm = coefficients(self.curve.cfg.kind, t)[1]

    def step(self, lr: Optional[float] = None, grad_inv_scale: float = 1.0, need_norm: bool = False):
        from . import ops
        m = self.model
        self.step_count += 1
        nsq = None
        if self.max_grad_norm is not None or need_norm:
            ops.l2norm_sq(m.flat_grad, self._partial, self.grad_norm_sq)
            nsq = self.grad_norm_sq
        max_norm = float(self.max_grad_norm if self.max_grad_norm is not None else 3.0e38)
        self._cm_last = self.cm
        ops.adam_step(self.curve.theta, m.flat_grad, self.exp_avg, self.exp_avg_sq, nsq, max_norm, grad_inv_scale * self.cm,
                      self.lr if lr is None else lr, self.betas[0], self.betas[1], self.eps, self.step_count,
                      skipped=self.skipped if nsq is not None else None, weights=False)
        self.hold(draw_t(self.gen, self.curve.cfg))       # (bumps WEIGHTS_EPOCH: the network's weights are what changed)

    def grad_norm(self, grad_inv_scale: float = 1.0) -> float:
        """Global L2 norm of the bend's gradient of the last step, sqrt(norm_sq) * grad_inv_scale * cm -- synchronises; for logging/tests."""
        return math.sqrt(float(self.grad_norm_sq)) * grad_inv_scale * self._cm_last

    def state_dict(self) -> Dict:
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count, "lr": self.lr}

    def load_state_dict(self, sd: Dict):
        if "ema" in sd:
            raise ValueError("load_state_dict: the state holds an EMA shadow but this optimiser trains a curve's bend (no EMA with a curve)")
        if sd["exp_avg"].numel() != self.exp_avg.numel():
            raise ValueError(f"load_state_dict: the state's moments hold {sd['exp_avg'].numel()} floats, this bend {self.exp_avg.numel()}")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])
        self.lr = float(sd.get("lr", self.lr))

    # the curve's own part of a training state, beside state_dict(): what a resumed run needs besides the two endpoints
    def curve_state(self) -> Dict:
        cfg = self.curve.cfg
        return {"theta": self.curve.theta, "t": self.t, "generator": self.gen.get_state(), "kind": cfg.kind, "seed": cfg.seed,
                "t_min": cfg.t_min, "t_max": cfg.t_max, "fingerprints": list(self.curve.fingerprints())}

    def load_curve_state(self, sd: Dict):
        """theta, the generator and the current t of a state; the network then holds phi(t) again.  Another kind or other endpoints raise."""
        if sd["kind"] != self.curve.cfg.kind:
            raise ValueError(f"load_curve_state: the state holds a {sd['kind']!r} curve; this optimiser trains a {self.curve.cfg.kind!r} one")
        if sd["theta"].numel() != self.curve.theta.numel():
            raise ValueError(f"load_curve_state: the state's bend holds {sd['theta'].numel()} floats, this model {self.curve.theta.numel()}")
        check_fingerprints(self.curve, sd["fingerprints"], "load_curve_state: the state")
        with torch.no_grad():
            self.curve.theta.copy_(sd["theta"])
        self.gen.set_state(sd["generator"].clone())
        self.hold(float(sd["t"]))


def curve_step(model, opt: CurveAdam, loss_fn, x0: torch.Tensor, R: Optional[torch.Tensor], timesteps: torch.Tensor,
               noise: Optional[torch.Tensor] = None, lr: Optional[float] = None) -> torch.Tensor:
    """One eager optimiser step of the curve's training on one batch: the loss at phi(opt.t) as the trainer forms it (LossFn.p_loss; R None:
    a zero poison residual, clean data), backward into flat_grad, `opt.step(lr)` -- norm, Adam on the bend, the next t and its point -- and
    flat_grad zeroed.  Returns the loss at the point the step was taken at (device, no sync).  The loss function's grad_scale is put back."""
    dev = model.device
    x0 = x0.to(dev).float()
    R = torch.zeros_like(x0) if R is None else R.to(dev).float()
    if getattr(model, "conv_math", None) == "f16":
        raise NotImplementedError("curve_step with conv_math='f16' is not built (flat_grad holds a scaled gradient there)")
    kept, loss_fn.grad_scale = loss_fn.grad_scale, 1.0
    try:
        model.zero_grad()
        kw = {"is_poison": torch.zeros(len(x0), dtype=torch.bool, device=dev)} if getattr(loss_fn, "shaped", False) else {}
        loss = loss_fn.p_loss(model, x0, R, timesteps.to(dev), noise=None if noise is None else noise.to(dev), **kw)
        loss.backward()
        opt.step(lr=lr)
    finally:
        loss_fn.grad_scale = kept
        model.zero_grad()
    return loss.detach()


# ---- the loss along the curve ------------------------------------------------------------------------------------------------------------------
def curve_scan(model, curve: Curve, loss_fn, batches: Iterable, ts: Sequence[float], seed: int = 0, trigger: Optional[torch.Tensor] = None):
    """The loss along the curve, to choose t by: for each t of `ts`, `curve.point(t)` and the no-grad clean loss, the mean over `batches`.

    batches: clean image (or latent) tensors [b, C, H, W], or dicts that hold them under "image".  Batch k uses the timesteps and noise of
    `anchor.fisher_draws(shape, T, seed, k)`, so every t sees the same draws.  With `trigger` (a [C, H, W] tensor, a known or an inverted one)
    every entry also holds the poisoned loss: the poison residual R is the trigger and the sample the batch's "target" key (the backdoor
    target, [C, H, W] or one per image), so the batches are dicts then.  Returns [{"t", "loss_clean", "loss_poison"?}]; afterwards the
    network holds the weights it held before, bit for bit."""
    from . import ops
    batches = list(batches)
    if not batches:
        raise ValueError("curve_scan: no batches")
    ts = [float(t) for t in ts]
    for t in ts:
        coefficients64(curve.cfg.kind, t)                 # every t is checked before the first launch
    if trigger is not None and not all(isinstance(b, dict) and "target" in b and "image" in b for b in batches):
        raise ValueError("curve_scan: with a trigger every batch is a dict with the clean images under 'image' and the backdoor target under 'target'")
    dev = model.device
    T = _timesteps_of(loss_fn)
    shaped = getattr(loss_fn, "shaped", False)
    keep = model.flat_param.detach().clone()
    out = []
    try:
        with torch.no_grad():
            for t in ts:
                curve.point(t)
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
                row = {"t": t, "loss_clean": float(torch.stack(clean).double().mean())}
                if trigger is not None:
                    row["loss_poison"] = float(torch.stack(poison).double().mean())
                out.append(row)
    finally:
        with torch.no_grad():
            model.flat_param.copy_(keep)
        ops.WEIGHTS_EPOCH += 1
        model.weights_changed()
    return out
