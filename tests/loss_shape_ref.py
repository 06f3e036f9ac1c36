"""References, inputs, bounds and the shape table of the shaped loss (vd_loss_sample_fwd_bwd, LossFn snr_gamma / poison_weight / track_split):
a helper module, not a test file; plain torch / numpy, no GPU.  test_loss_shape_cpu.py pins everything here on the CPU, test_loss_shape_gpu.py
compares the kernel with it and test_loss_shape_train_gpu.py the training step.

* `shaped_f64`: the definition in float64 -- l[b] = mean_i norm(pred ps - y), w[b] = weight[b] wtab[clamp(t[b])] (pw where flagged),
  loss = mean_b w[b] l[b], dpred = gscale dloss/dpred, stats = {sum l clean, n clean, sum l poisoned, n poisoned};
* `dpred_f32`: the float32 sequence ((gcoef w) g) ps the kernel promises, operation by operation;
* `shaped_torch`: the same loss in plain torch (any dtype, differentiable): what torch float32 computes, and the oracle loss of the training tests;
* `sample_loss_bound`: the bound on a sample's loss from the kernel's reduction shape (below);
* the shape table, with what the library's own plan query says each shape reaches."""
import numpy as np
import torch

import elem_ref as E

KINDS = E.LOSS_KINDS
TINY_CHW = 3                                     # the many-tiny-samples shapes: one 3-float segment per sample
# the smallest at which each path can go wrong: one element; under one workgroup, ragged; either side of 256; two segments of a vector sample;
# odd chw (misaligned sample bases, many segments); one 256 x 256 image (the largest segment count); a training batch
SHAPES = ((1, 1), (3, 85), (2, 255), (2, 257), (7, 3072), (5, 66603), (1, 196608), (128, 12288))


def plan(B, chw):
    """(segments, blocks, workspace floats) from the library (host only)."""
    from villandiffusion_amd import ops
    return ops.loss_sample_plan(B, chw)


def block_cap():
    """The launcher's block cap and its largest segment count, asked of the plan query: a batch far beyond any cap, a sample far beyond any cut."""
    return plan(1 << 22, TINY_CHW)[1], plan(1, 1 << 40)[0]


def tiny_shapes():
    """((B, 3) with B * segments exactly the block cap, (B, 3) beyond it by a ragged 37 pairs): some workgroups walk two samples."""
    cap, _ = block_cap()
    seg = plan(1, TINY_CHW)[0]
    return (cap // seg, TINY_CHW), (cap // seg + 37, TINY_CHW)


def all_shapes():
    return SHAPES + tiny_shapes()


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def loss_inputs(B, chw, negative_pscale, seed=0):
    """E.loss_inputs for any B: rows in chunks of at most five (its pscale list has five entries), each chunk with its own exact d = 0, +-1 and
    either side of +-1."""
    parts = [E.loss_inputs(min(5, B - b0), chw, negative_pscale, seed=seed + 7 * b0) for b0 in range(0, B, 5)]
    pred, y = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return pred, y, (torch.cat([p[2] for p in parts]) if negative_pscale else None)


def shaping_inputs(B, T=16, seed=0):
    """(weight [B] in [0.25, 2], wtab [T] in (0, 1], t [B] in range, flags [B] bool with both classes where B > 1)."""
    g = E.g(seed + 100)
    weight = 0.25 + 1.75 * torch.rand(B, generator=g)
    wtab = (0.05 + 0.95 * torch.rand(T, generator=g)).float()
    t = torch.randint(0, T, (B,), generator=g)
    flags = (torch.arange(B) % 3 == 1)
    return weight.float(), wtab, t, flags


def integer_inputs(B, chw, seed=0):
    """Everything exact: d in {-3 .. 3}, pscale in {+-1, +-2}, pred a small integer, y = pred ps - d; weights in {1, 2}, table entries in
    {0.5, 1}.  With poison_weight 2 every partial sum of every reduction is a multiple of one power of two and below 2^24 of it."""
    g = E.g(seed)
    d = torch.randint(-3, 4, (B, chw), generator=g).float()
    ps = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (B,), generator=g)]
    pred = torch.randint(-4, 5, (B, chw), generator=g).float()
    y = pred * ps[:, None] - d
    weight = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (B,), generator=g)]
    wtab = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (8,), generator=g)]
    t = torch.randint(0, 8, (B,), generator=g)
    flags = (torch.arange(B) % 2 == 1)
    return pred, y, ps, weight, wtab, t, flags


# -------------------------------------------------------------------------------------------------------------------------- references
def _norm(d, kind):
    """(norm(d), norm'(d)) elementwise, any float dtype: sign(0) = 0 for l1, beta = 1 for huber."""
    if kind == "l2":
        return d * d, 2 * d
    if kind == "l1":
        return d.abs(), torch.sign(d)
    a = d.abs()
    return torch.where(a < 1, 0.5 * d * d, a - 0.5), torch.where(a < 1, d, torch.sign(d))


def weights(B, weight=None, wtab=None, t=None, flags=None, pw=1.0, dtype=torch.float64):
    """w[b] = weight[b] * wtab[clamp(t[b], 0, T - 1)] * (pw where flags[b]), absent factors 1, multiplied in this order in `dtype`."""
    w = torch.ones(B, dtype=dtype) if weight is None else weight.to(dtype).clone()
    if wtab is not None:
        w = w * wtab.to(dtype)[t.clamp(0, wtab.numel() - 1)]
    if flags is not None:
        w = w * torch.where(flags.bool(), torch.tensor(float(pw), dtype=dtype), torch.ones((), dtype=dtype))
    return w


def shaped_f64(pred, y, ps=None, weight=None, wtab=None, t=None, flags=None, pw=1.0, gscale=1.0, kind="l2"):
    """(loss, dpred, sample_loss, stats) in float64."""
    B, chw = pred.shape
    psd = ps.double()[:, None] if ps is not None else torch.ones(B, 1, dtype=torch.float64)
    v, gr = _norm(pred.double() * psd - y.double(), kind)
    l = v.mean(1)
    w = weights(B, weight, wtab, t, flags, pw)
    f = flags.bool() if flags is not None else torch.zeros(B, dtype=torch.bool)
    stats = torch.stack([l[~f].sum(), (~f).sum().double(), l[f].sum(), f.sum().double()])
    return (w * l).sum() / B, gr * psd * w[:, None] * (gscale / (B * chw)), l, stats


def dpred_f32(pred, y, ps=None, weight=None, wtab=None, t=None, flags=None, pw=1.0, gscale=1.0, kind="l2"):
    """The float32 sequence of the kernel: d = pred * ps - y (two roundings), gcoef = (2 or 1) * gscale / float(B chw), ((gcoef * w) * g) * ps with
    g = d (l2; the 2 is in gcoef), sign(d) (l1), d or sign(d) (huber)."""
    B, chw = pred.shape
    psf = ps.float()[:, None] if ps is not None else torch.ones(B, 1)
    d = pred.float() * psf - y.float()
    _, g = _norm(d, kind)
    if kind == "l2":
        g = d
    gcoef = (np.float32(2.0 if kind == "l2" else 1.0) * np.float32(gscale)) / np.float32(B * chw)
    w = weights(B, weight, wtab, t, flags, pw, dtype=torch.float32)
    return ((E.f32(gcoef) * w)[:, None] * g) * psf


def shaped_torch(pred, y, ps=None, w=None, kind="l2"):
    """mean_b w[b] mean_i norm(pred ps - y) in pred's dtype with torch ops (differentiable) -> (loss, sample_loss)."""
    B = pred.shape[0]
    p2, y2 = pred.reshape(B, -1), y.reshape(B, -1)
    if ps is not None:
        p2 = p2 * ps.to(p2.dtype)[:, None]
    l = _norm(p2 - y2.to(p2.dtype), kind)[0].mean(1)
    return ((l * w.to(l.dtype)) if w is not None else l).mean(), l


def shaped_torch_f32(pred, y, ps=None, weight=None, wtab=None, t=None, flags=None, pw=1.0, gscale=1.0, kind="l2"):
    """(loss, dpred, sample_loss) as plain torch float32 computes them on the host."""
    x = pred.clone().float().requires_grad_(True)
    w = weights(pred.shape[0], weight, wtab, t, flags, pw, dtype=torch.float32)
    loss, l = shaped_torch(x, y.float(), ps, w, kind)
    (loss * gscale).backward()
    return loss.detach(), x.grad, l.detach()


# ------------------------------------------------------------------------------------------------------------------------------ bounds
def chain_terms(chw, segments):
    """The longest chain of roundings behind one sample's loss in the kernel: a segment holds seg_len = ceil(chw / segments) rounded up to 4
    floats; a thread adds ceil(seg_len / 256) terms serially on the scalar path and 4 ceil(seg_len / 1024) on the 16-byte one (the larger is
    taken), each term rounded once when it is formed; 6 shuffle steps and the 2 adds of block_sum_256; segments - 1 adds of the second stage;
    the division by chw."""
    seg_len = (-(-chw // segments) + 3) // 4 * 4
    serial = max(-(-seg_len // 256), 4 * -(-seg_len // 1024))
    return 1 + serial + 6 + 2 + (segments - 1) + 1


def sample_loss_bound(pred, y, ps, kind, segments):
    """Per-sample bound [B] on |sample_loss - float64| / float64: chain_terms half-ulps on the sum of non-negative terms, plus what the two
    roundings of d = pred * ps - y (one without pscale) can move the sum by: |d32 - d| <= delta = 2^-24 (|pred ps| + |d|) (2^-24 |d| without
    pscale), and norm moves by at most |norm'(d)| delta + delta^2.  Nothing here is fitted to a result."""
    B, chw = pred.shape
    u = 2.0 ** -24
    prod = pred.double() * (ps.double()[:, None] if ps is not None else 1.0)
    d = prod - y.double()
    delta = u * (d.abs() + (prod.abs() if ps is not None else 0.0))
    v, gr = _norm(d, kind)
    moved = (gr.abs() * delta + delta * delta).sum(1)
    return chain_terms(chw, segments) * u + moved / v.sum(1).clamp_min(1e-300)


def figures(loss, dpred, sample_loss, stats, ref, bound_b):
    """[(name, value, bound)]: the suite's 1e-5 on the loss and on max |dpred|; every sample's loss inside its own bound (the worst ratio
    against 1); the class sums inside the worst sample bound plus one half-ulp per added sample; the counts exact."""
    rl, rd, rs, rst = ref
    figs = E.loss_figures(loss, dpred, rl, rd) if dpred is not None else [("loss", abs(float(loss) - float(rl)) / max(abs(float(rl)), 1e-300), E.TOL_NORM)]
    sl = sample_loss.detach().double().cpu()
    figs.append(("sample_loss / bound", float(((sl - rs).abs() / rs.clamp_min(1e-300) / bound_b).max()), 1.0))
    st = stats.detach().double().cpu()
    cls = float(bound_b.max()) + rs.numel() * 2.0 ** -24
    for i, name in ((0, "clean sum"), (2, "poisoned sum")):
        figs.append((name, abs(float(st[i] - rst[i])) / max(float(rst[i]), 1e-300) if float(rst[i]) > 0 else abs(float(st[i])), cls))
    figs.append(("counts", float((st[[1, 3]] - rst[[1, 3]]).abs().max()), 0.0))
    return figs


# ------------------------------------------------------------------------------------------------------- the oracle's shaped training loss
def min_snr_f64(alphas_cumprod, gamma):
    """min(snr, gamma) / snr with snr = abar / (1 - abar), in float64."""
    ac = alphas_cumprod.double()
    snr = ac / (1 - ac)
    return torch.minimum(snr, torch.tensor(float(gamma), dtype=torch.float64)) / snr


def oracle_weights(loss_ref, t, flags, snr_gamma=None, pw=1.0, weight=None):
    """w[b] of a shaped LossFn, from the oracle loss function's own schedule (float64)."""
    wtab = min_snr_f64(loss_ref.alphas_cumprod, snr_gamma) if snr_gamma is not None else None
    return weights(len(t), weight, wtab, t, flags, pw)


def oracle_shaped_loss(loss_ref, model, x0, R, t, noise, w=None, kind="l2"):
    """The weighted loss through an oracle network (oracle.loss_ref.LossFnRef's inputs and targets, its VP / VE prediction), differentiable:
    mean_b w[b] mean_i norm(prediction - target) -> (loss, unweighted sample losses)."""
    x_noisy, target = loss_ref.inputs_targets(x0, R, t, noise)
    if hasattr(loss_ref, "sigmas"):
        sig = loss_ref.sigmas[t]
        pred, ps = model(x_noisy.contiguous(), sig.contiguous(), return_dict=False)[0], -sig
    else:
        pred, ps = model(x_noisy.contiguous(), t.contiguous(), return_dict=False)[0], None
    return shaped_torch(pred, target, ps, w, kind)
