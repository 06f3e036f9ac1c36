"""Mode Connectivity Repair restated for the tests (a helper module, not a test file; no GPU needed).

1. The numpy float32 op sequences of the two kernels of vd_curve.hip: `point_ref` (three products, two sums) and `geometry_ref`, which walks the
   three sums the way include/villan_hip.h states it -- items of four, item q in thread q % (grid * block), one partial per position of an item,
   (a0 + a1) + (a2 + a3), the xor tree over the 64 lanes of a wave, the four waves as (r0 + r1) + (r2 + r3), and the second stage over
   partial[t], partial[t + 256], ... -- so the kernel's three floats can be held to it bit for bit.
2. The trainer oracle `FlatOracle`: the CPU oracle network called through `torch.func.functional_call` with the weights
   (ca * A + cm * theta) + cb * B formed from the SAME three float32 coefficients `curve.coefficients` gives, autograd to theta,
   clip_grad_norm_(theta, 1.0), torch.optim.Adam on theta, the cosine schedule, and the t sequence by the rule of curve.py (one host generator
   seeded with the configuration's seed; the first draw at construction, one more after every optimiser step).  Without endpoints it is the
   plain step on the same flat vector, which the plain trainer's figure is measured against.  `forget_cm=True` is the wrong oracle of the
   teeth test: theta's gradient is dL/dphi, the factor cm left out."""
import numpy as np
import torch
from torch.func import functional_call

import oracle.schedulers_ref as R
import sam_ref
from oracle.loss_ref import SDE_VP, LossFnRef
from villandiffusion_amd.curve import CurveConfig, coefficients, draw_t

SMALL = sam_ref.SMALL
batch_of = sam_ref.batch_of
f32 = np.float32

SEED_A, SEED_B = 3, 4          # reset_parameters seeds of the two endpoints of the trajectory tests (A is tests/anchor_ref.py's start)
CURVE_SEED = 0                 # CurveConfig.seed of the trajectory tests
STEPS = 4
# The plain trainer's update L2 error over these batches from this start in bf16x3, as recorded on MI355X in tests/test_anchor_gpu.py; the GPU
# test measures it again and gates on 1.5x what it measures.  The CPU teeth test needs a figure without a GPU: 10 x 1.5 x this one.
BF16X3_PLAIN_RECORDED = 4.09e-4
TEETH = 10 * 1.5 * BF16X3_PLAIN_RECORDED


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------------
def point_ref(wa, wm, wb, ca, cm, cb):
    """p = ca * a; p = p + cm * m; out = p + cb * b, on float32 arrays, every operation rounded on its own."""
    p = f32(ca) * wa + f32(cm) * wm
    return p + f32(cb) * wb


def chain(n, grid, block):
    """vd_curve_geometry's longest chain of additions: ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18 (include/villan_hip.h)."""
    items = (n + 3) // 4
    return -(-items // (grid * block)) + -(-grid // 256) + 18


def _tree_256(v):
    """[..., 256] float32 -> [...]: the xor tree over each wave of 64 lanes (offsets 32 ... 1), then (r0 + r1) + (r2 + r3)."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    r = v[..., 0]
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def two_stage_sum(terms, grid, block=256):
    """The fixed-order sum of vd_sam_norm_sq over float32 `terms` (one per float of the buffer) for the launch shape (grid, block)."""
    assert terms.dtype == f32 and block == 256
    n = terms.size
    T = grid * block
    items = (n + 3) // 4
    rounds = max(1, -(-items // T))
    padded = np.zeros(rounds * T * 4, dtype=f32)      # positions past n add +0.0 to a non-negative partial: its bits do not change
    padded[:n] = terms
    per = padded.reshape(rounds, T, 4)
    acc = np.zeros((T, 4), dtype=f32)
    for r in range(rounds):                            # a thread's items in ascending order
        acc = acc + per[r]
    v = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    partial = _tree_256(v.reshape(grid, 256))
    rows = -(-grid // 256)
    pp = np.zeros(rows * 256, dtype=f32)
    pp[:grid] = partial
    pp = pp.reshape(rows, 256)
    s = np.zeros(256, dtype=f32)
    for r in range(rows):                              # thread t: partial[t], partial[t + 256], ...
        s = s + pp[r]
    return _tree_256(s)


def geometry_ref(wa, wm, wb, grid, block=256):
    """The three floats of vd_curve_geometry: every difference and every square rounded to float32, each sum in the two stages."""
    da, db, dc = wm - wa, wm - wb, wa - wb
    return np.array([two_stage_sum(d * d, grid, block) for d in (da, db, dc)], dtype=f32)


def geometry_f64(wa, wm, wb):
    """(the three sums in float64 from float64 differences, the sum of their terms: the same, the terms being non-negative)."""
    a, m, b = (v.astype(np.float64) for v in (wa, wm, wb))
    return np.array([((m - a) ** 2).sum(), ((m - b) ** 2).sum(), ((a - b) ** 2).sum()])


# ---- 2. the trainer oracle ----------------------------------------------------------------------------------------------------------------------
def named(flat, offs, frozen=()):
    """name -> tensor views of a flat tensor by the network's offsets; the names in `frozen` are cut off the graph."""
    return {k: (flat[off:off + n].detach() if k in frozen else flat[off:off + n]).view(shape) for k, (off, n, shape) in offs.items()}


def t_sequence(cfg, count):
    """The first `count` draws of the rule: t[0] is held at construction, t[k] after the k-th optimiser step."""
    gen = g(cfg.seed)
    return [draw_t(gen, cfg) for _ in range(count)]


class FlatOracle:
    """ends = (A, B): the curve step on theta (flat, float32).  ends None: the plain step on the flat weights `theta0`.
    step(micro_batches) -> (mean loss at the weights the step was taken at, the pre-clip norm of theta's gradient)."""

    def __init__(self, ref, lf, offs, theta0, ends=None, cfg=None, frozen=(), lr=1e-3, total_steps=20, warmup_steps=0, max_grad_norm=1.0,
                 forget_cm=False):
        self.ref, self.lf, self.offs, self.ends, self.frozen, self.forget_cm = ref, lf, offs, ends, tuple(frozen), forget_cm
        self.cfg = cfg if cfg is not None else CurveConfig()
        self.theta = theta0.detach().clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.theta], lr=lr)
        self.sch = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda k: R.cosine_with_warmup_lambda(k, warmup_steps, total_steps))
        self.max_grad_norm = max_grad_norm
        self.gen = g(self.cfg.seed)
        self.t = draw_t(self.gen, self.cfg) if ends is not None else None
        self.ts = [self.t]

    def weights(self):
        if self.ends is None:
            return self.theta
        ca, cm, cb = coefficients(self.cfg.kind, self.t)
        A, B = self.ends
        if self.forget_cm:                                 # the same point, but d phi / d theta = 1
            return ((ca * A + cm * self.theta.detach()) + cb * B) + (self.theta - self.theta.detach())
        return (ca * A + cm * self.theta) + cb * B

    def step(self, micro_batches):
        self.opt.zero_grad()
        w = named(self.weights(), self.offs, self.frozen)
        model = lambda x, tt, return_dict=False: functional_call(self.ref, w, (x, tt))
        loss = sum(self.lf.p_loss(model, x0, Rr, t, noise=eps) for x0, Rr, t, eps in micro_batches) / len(micro_batches)
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_([self.theta], self.max_grad_norm))
        self.opt.step()
        self.sch.step()
        if self.ends is not None:
            self.t = draw_t(self.gen, self.cfg)
            self.ts.append(self.t)
        return float(loss.detach()), norm


def update_error(got, want, start):
    """||theta - theta_ref|| / ||theta_ref - theta_0|| on flat tensors, float64."""
    got, want, start = (v.detach().cpu().double() for v in (got, want, start))
    return float((got - want).norm() / (want - start).norm())


# ---- the trajectory cases on the small UNet, computed once and shared read-only -------------------------------------------------------------------
_SETUP, _RUNS = {}, {}


def flat_of(seed, **cfg):
    from villandiffusion_amd.unet import UNet2DModel
    twin = UNet2DModel(**(cfg or SMALL), device="cpu")
    twin.reset_parameters(seed=seed)
    return twin


def setup():
    """The endpoints of the trajectory tests: the small UNet at SEED_A and at SEED_B, flat host tensors, the layout, the midpoint theta_0."""
    if not _SETUP:
        a, b = flat_of(SEED_A), flat_of(SEED_B)
        A, B = a.flat_param.detach().clone(), b.flat_param.detach().clone()
        mid = torch.from_numpy(point_ref(A.numpy(), A.numpy(), B.numpy(), 0.5, 0.0, 0.5))
        _SETUP.update(offs=dict(a._offs), A=A, B=B, theta0=mid)
    return _SETUP


def oracle_run(mode="curve", accum=1, steps=STEPS, kind="bezier"):
    """mode "curve" / "forget_cm" / "plain" (from A): `steps` optimiser steps; step i takes the micro-batches batch_of(i * accum) ...
    -> dict(losses, norms, ts, end: the flat theta (plain: the flat weights), start)."""
    key = (mode, accum, steps, kind)
    if key not in _RUNS:
        from oracle.unet_ref import UNet2DModelRef
        s = setup()
        ref = UNet2DModelRef(**SMALL)
        lf = LossFnRef(R.DDPMSchedulerRef(), SDE_VP, psi=1)
        if mode == "plain":
            o = FlatOracle(ref, lf, s["offs"], s["A"])
            start = s["A"]
        else:
            o = FlatOracle(ref, lf, s["offs"], s["theta0"], ends=(s["A"], s["B"]), cfg=CurveConfig(kind=kind, seed=CURVE_SEED),
                           forget_cm=mode == "forget_cm")
            start = s["theta0"]
        out = [o.step([batch_of(i * accum + j) for j in range(accum)]) for i in range(steps)]
        _RUNS[key] = dict(losses=[a for a, _ in out], norms=[b for _, b in out], ts=list(o.ts), end=o.theta.detach().clone(), start=start)
    return _RUNS[key]
