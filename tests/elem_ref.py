"""References, inputs and case lists for the elementwise hot-path kernels of vd_elem.hip (a helper module, not a test file; plain torch /
numpy, no GPU).  test_elem_ref_cpu.py pins everything here on the CPU; test_elem_edges_gpu.py compares the kernels with it.

Three kinds of reference:

* restatements of device code whose every operation is an exact function of its operands: Philox4x32-10 in integer arithmetic
  (`philox4x32_10`, `randn_ref`), Adam's update operation by operation in float32 (`adam_emulate`, `grad_scale`), and the short float32
  torch sequences of the kernels that promise bit-equality (q-sample, sched_step, lincomb, postprocess, rowscale, add, scale);
* float64 references of the kernels that round differently from the host (SiLU, the losses, the embeddings, the norms), with the bounds the
  tests apply to them: the figure functions below return [(name, value, bound)] and `report` prints and asserts them, for a kernel's result and
  for torch float32's alike;
* the sizes, each with the launch it reaches.  T = 1 048 576 is the thread count of a capped launch: egrid() gives at most 4096 blocks of 256
  threads and the kernels go on in grid-stride loops.

The Fourier embedding is the one place where "the argument as the kernel forms it" cannot be restated: logf is not correctly rounded, on
either side, and at an argument of ~10^3 one ulp of it is ~10^-4 in the sine.  Its reference evaluates the kernel's expression -- float32 inputs,
the float32 constant pi -- in float64 throughout, and the bound is measured from torch float32's error against it (fourier_bound)."""
import math

import numpy as np
import torch

T = 1 << 20                                      # threads of a capped egrid() launch

# ------------------------------------------------------------------------------------------------------------------ the size lists
# one thread; a ragged second block; the cap (4096 blocks) with a ragged wrap: silu fwd / bwd, lincomb, rowscale, add_strided's scalar kernel
SIZES_SCALAR = (1, 257, T + 257)
# the same in f32x4 items (1, 257, T + 257 of them): add_strided's vector kernel, add_flat
SIZES_VEC = (4, 1028, 4 * T + 1028)
# scale_kernel is launched with egrid(n, 4): 1 block; 2 blocks (1027 > 1024); capped at 4096 with every thread wrapping four times and 1027 more
SIZES_SCALE = (1, 1027, 4 * T + 1027)
# randn / sched_step work in quads: every partial last quad (n % 4 = 1, 2, 3, 0), a second block, and T + 301 quads: the cap, the last one partial
SIZES_QUADS = (1, 2, 3, 4, 5, 1023, 4 * T + 1203)
# adam_step egrid(n, 8), l2norm_sq egrid(n, 16) clamped to 1024: the scalar tail alone (n < 4: no f32x4 item at all); one item, no tail; items
# and a 3-float tail; 8T + 2051: 2T + 512 items on T threads (adam: 4097 -> 4096 blocks; l2norm: 2049 -> 1024 blocks, every partial slot
# written) and a 3-float tail that block 0 of the capped grid owns
SIZES_ADAM = (1, 3, 4, 2051, 8 * T + 2051)
# the loss runs on at most 1024 blocks: one element; under one block; exactly 1024 blocks and no wrap; a wrap, pscale changing inside blocks
LOSS_SHAPES = ((1, 1), (3, 85), (4, 65536), (5, 66603))
# q-sample: one element; under one block; beyond T with t[b] changing inside a block
QSAMPLE_SHAPES = ((1, 1), (3, 85), (5, 209767))
# postprocess: the NHWC index arithmetic with C != 3 and H != W; beyond T
POSTPROCESS_SHAPES = ((1, 1, 1, 1), (2, 4, 7, 5), (2, 3, 419, 421))
# batch_l2norm, one block per row: fewer elements than threads, one per thread, a ragged second round, 12 and 768 serial terms per thread
BATCH_NORM_BS = (1, 5)
BATCH_NORM_INNERS = (1, 255, 256, 257, 3072, 196608)
TEMB_SHAPES = ((1, 1), (5, 64), (7, 160))
TEMB_T = (1999.0, 0.0, 1.0, 499.5, 999.0)
FOURIER_SHAPES = ((1, 1), (3, 128), (128, 256))
RANDN_IDENTITY = ((0, 0), (1234, 0), (1234, 2 ** 32 - 1), (1234, 2 ** 32 + 5), (2 ** 32 + 7, 3), (2 ** 64 - 1, 2 ** 40))

TOL_NORM = 1e-5            # the suite's: l2norm_sq (on the norm), the loss
TOL_DPRED = 1e-5           # of max |dpred|
TOL_TEMB = 2e-6            # absolute
TOL_RANDN = 1e-3           # absolute: an identity gate


def rows(n):
    """(B, inner) with B * inner = n for the row-wise kernels: inner = 1 at 257 (row = element), three ragged rows at the cap."""
    return {1: (1, 1), 257: (257, 1), T + 257: (3, (T + 257) // 3)}[n]


def g(seed):
    return torch.Generator().manual_seed(seed)


def f32(c):
    """A float32 scalar as a 0-dim tensor: an operation with it is the float32 operation, whatever torch does with Python numbers."""
    return torch.tensor(float(c), dtype=torch.float32)


def rel(a, b):
    """max |a - b| / max |b| in float64 (the suite's relative error)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def ulp32(x):
    """The spacing of float32 at |x| (float64 tensor)."""
    x = x.detach().float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def report(what, figs):
    """Print every figure (name, value, bound) as a [parity] line with value / bound, then assert them all."""
    for name, val, bound in figs:
        print(f"[parity] {what} {name}: {val:.3e} (bound {bound:.3e}, value/bound {val / bound if bound > 0 else float(val > 0):.3f})")
    bad = [f"{name}: {val:.3e} > {bound:.3e}" for name, val, bound in figs if not val <= bound]
    assert not bad, f"{what}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- Philox
_M0, _M1, _W0, _W1, _MASK = (np.uint64(c) for c in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32_10(counter_words, key_words):
    """Philox4x32-10 (Salmon et al., Random123) in 64-bit integer arithmetic: four counter words and two key words (scalars or arrays of equal
    shape, each < 2^32) -> the four output words as uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK for w in counter_words]
    k = [np.asarray(w, dtype=np.uint64) & _MASK for w in key_words]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return tuple(w.astype(np.uint32) for w in c)


def randn_uniforms(n, seed, offset):
    """The uniforms behind elements 0 .. n-1 of vd_randn(seed, offset): quad q uses counter (lo32(offset + q), hi32(offset + q), 0, 0) and key
    (lo32(seed), hi32(seed)); u = (float32(r) + 0.5f) * 2^-32 in float32, as randn4 forms it -> float32 [quads, 4]."""
    nq = (n + 3) // 4
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset % 2 ** 64) + np.arange(nq, dtype=np.uint64)          # wraps at 2^64 as the kernel's uint64_t does
    zero = np.zeros(nq, dtype=np.uint64)
    seed = seed % 2 ** 64
    r = philox4x32_10((ctr & _MASK, ctr >> _S32, zero, zero), (np.full(nq, seed & 0xFFFFFFFF, dtype=np.uint64), np.full(nq, seed >> 32, dtype=np.uint64)))
    return np.stack([(w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32) for w in r], axis=1)


_TWO_PI_F32 = float(np.float32(6.283185307179586))


def box_muller(u, dtype):
    """randn4's Box-Muller on the float32 uniforms u [quads, 4], evaluated in `dtype`: (u0, u1) -> elements 0, 1; (u2, u3) -> elements 2, 3."""
    u = u.astype(dtype)
    one = dtype(0.99999994) if dtype is np.float64 else np.float32(0.99999994)
    ra, rb = (np.sqrt(dtype(-2.0) * np.log(np.minimum(u[:, i], one) + dtype(1e-12))) for i in (0, 2))
    a1, a3 = dtype(_TWO_PI_F32) * u[:, 1], dtype(_TWO_PI_F32) * u[:, 3]
    return np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3), rb * np.sin(a3)], axis=1).reshape(-1)


def randn_ref(n, seed, offset):
    """Elements 0 .. n-1 of vd_randn(seed, offset) with log, sqrt, sin and cos in float64 -> float64 tensor [n]."""
    return torch.from_numpy(box_muller(randn_uniforms(n, seed, offset), np.float64)[:n].copy())


def randn_torch_f32(n, seed, offset):
    """The same from the same uniforms with everything in float32 on the host (what the identity gate must leave room for)."""
    return torch.from_numpy(box_muller(randn_uniforms(n, seed, offset), np.float32)[:n].copy())


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def grad_scale(norm_sq, max_norm, inv_scale):
    """adam_grad_scale in float32: the gradient scale of the step (np.float32), or None when the step is skipped (norm_sq not <= 3e38).
    norm_sq None: no clipping."""
    gs = np.float32(inv_scale)
    if norm_sq is None:
        return gs
    with np.errstate(over="ignore"):
        nsq = np.float32(norm_sq)
    if not nsq <= np.float32(3.0e38):
        return None
    norm = np.sqrt(nsq) * np.float32(inv_scale)
    return gs * np.minimum(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6)))


def adam_consts(lr, beta1, beta2, step):
    """(step_size, bc2_sqrt, 1 - beta1, 1 - beta2) as the launcher and the kernel form them: bc1 and sqrt(bc2) from double pow of the float32
    betas, then cast to float; step_size = lr / bc1 and 1 - beta in float32."""
    b1, b2 = np.float32(beta1), np.float32(beta2)
    bc1 = np.float32(1.0 - math.pow(float(b1), float(step)))
    bc2_sqrt = np.float32(math.sqrt(1.0 - math.pow(float(b2), float(step))))
    return np.float32(lr) / bc1, bc2_sqrt, np.float32(1.0) - b1, np.float32(1.0) - b2


def adam_emulate(p, g_, m, v, gs, lr, beta1, beta2, eps, step):
    """adam_update operation by operation in float32 (vd_elem.o is built with -ffp-contract=off; (1.f - beta2) * gr * gr associates left) ->
    new (p, m, v); float32 tensors in, nothing modified.  The square root is taken in float64 and rounded: that is the correctly rounded float32
    root (53 >= 2 * 24 + 2 bits), which the device's sqrtf is; torch.sqrt of a float32 CPU tensor is not (a vector math library, off by one ulp
    on ~0.6 % of the elements)."""
    step_size, bc2_sqrt, omb1, omb2 = (f32(c) for c in adam_consts(lr, beta1, beta2, step))
    gr = g_ * f32(gs)
    m = m + (gr - m) * omb1
    v = v * f32(beta2) + (omb2 * gr) * gr
    denom = v.double().sqrt().float() / bc2_sqrt + f32(eps)
    upd = step_size * (m / denom)
    return p - upd, m, v


def adam_update_size(m, v, lr, beta1, beta2, eps, step):
    """|step_size * m / denom| in float64 of the NEW m, v: the size of the update, for the fallback gate on p."""
    step_size, bc2_sqrt, _, _ = adam_consts(lr, beta1, beta2, step)
    return (float(step_size) * m.double() / (v.double().sqrt() / float(bc2_sqrt) + float(np.float32(eps)))).abs()


def adam_f64(p, g_, m, v, clip, lr, beta1, beta2, eps, step):
    """torch.optim.Adam's step in float64 on the gradient g * clip (float64 tensors)."""
    gr = g_ * clip
    m = beta1 * m + (1 - beta1) * gr
    v = beta2 * v + (1 - beta2) * gr * gr
    denom = v.sqrt() / math.sqrt(1 - beta2 ** step) + eps
    return p - lr / (1 - beta1 ** step) * m / denom, m, v


# ------------------------------------------------------------------------------------------------------------------------------ SiLU
SILU_GRID = tuple(s * a for a in (0.0, 1e-30, 0.5, 1.0, 10.0, 20.0, 40.0, 80.0) for s in (1.0, -1.0)) + (-100.0, -1e4, 100.0)


def silu_inputs(n, seed):
    """(z, dy, dx0): randn with the fixed grid (both signs of 0 .. 80, -100, -1e4, +100) in its first elements and again in its last ones where n
    allows; dy and the preloaded dx of the accumulating backward are randn."""
    z = torch.randn(n, generator=g(seed))
    grid = torch.tensor(SILU_GRID, dtype=torch.float32)
    if n >= 2 * grid.numel():
        z[:grid.numel()] = grid
        z[-grid.numel():] = grid
    return z, torch.randn(n, generator=g(seed + 1)), torch.randn(n, generator=g(seed + 2))


def silu_f64(z):
    z = z.double()
    return z * torch.sigmoid(z)


def silu_grad_f64(z):
    """(d silu / dz, the same with both terms of 1 + z (1 - s) taken positive) in float64."""
    z = z.double()
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s)), s * (1 + z.abs() * (1 - s))


def _silu_ratio(err, mag, z, extra=0.0):
    """max over |z| <= 80 of err / ((|z| + 4) 2^-23 mag + 1e-30 + extra)."""
    z = z.double()
    bound = (z.abs() + 4) * 2.0 ** -23 * mag + 1e-30 + extra
    keep = z.abs() <= 80
    return float((err / bound)[keep].max()) if bool(keep.any()) else 0.0


def _silu_outside(got, z, ref):
    """Beyond |z| = 80: below -88 a finite value of magnitude <= 1e-30; above +80 within one ulp of the reference -> worst value / bound."""
    got, zd = got.detach().double().cpu(), z.double()
    lo, hi = zd < -88, zd > 80
    assert bool(torch.isfinite(got).all()), "a non-finite value"
    worst = 0.0
    if bool(lo.any()):
        worst = max(worst, float(got[lo].abs().max()) / 1e-30)
    if bool(hi.any()):
        worst = max(worst, float(((got - ref).abs() / ulp32(ref))[hi].max()))
    return worst


def silu_fwd_figures(got, z):
    """Elementwise, not relative to the largest output.  |z| <= 80: |got - ref| <= (|z| + 4) 2^-23 |ref| + 1e-30: __expf rounds z log2(e) once
    (|z| 2^-24 relative in e^-z); v_exp, the add, v_rcp and the final product cost an ulp each."""
    ref = silu_f64(z)
    err = (got.detach().double().cpu() - ref).abs()
    return [("silu fwd elem (|z| <= 80)", _silu_ratio(err, ref.abs(), z), 1.0), ("silu fwd beyond", _silu_outside(got, z, ref), 1.0)]


def silu_bwd_figures(got, z, dy, dx0=None):
    """The same bound on the gradient term dy s (1 + z (1 - s)), its magnitude taken as |dy| s (1 + |z| (1 - s)): equal to |ref| for z >= 0;
    for z < 0 the two terms of the sum cancel (silu' has a root at z = -1.2785) and no bound relative to the cancelled value can hold for
    float32 arithmetic, torch's included.  dx0: the preloaded dx of an accumulating launch, whose sum costs one more ulp."""
    d, mag = silu_grad_f64(z)
    term = dy.double() * d
    ref = term if dx0 is None else dx0.double() + term
    err = (got.detach().double().cpu() - ref).abs()
    extra = 0.0 if dx0 is None else ulp32(ref)
    name = "silu bwd" + (" accumulate" if dx0 is not None else "")
    figs = [(name + " elem (|z| <= 80)", _silu_ratio(err, dy.double().abs() * mag, z, extra), 1.0)]
    if dx0 is None:
        figs.append((name + " beyond", _silu_outside(got, z, ref), 1.0))
    else:                                                    # beyond |z| = 80 the term is 0 (or dy): the sum is dx0 (+ dy) to one ulp
        far = z.double().abs() > 80
        figs.append((name + " beyond", float((err / ulp32(ref))[far].max()) if bool(far.any()) else 0.0, 1.0))
    return figs


def silu_torch_f32(z, dy, dx0=None):
    """(fwd, bwd or dx0 + bwd) as torch float32 computes them on the host."""
    x = z.clone().requires_grad_(True)
    y = torch.nn.functional.silu(x)
    y.backward(dy)
    return y.detach(), x.grad if dx0 is None else dx0 + x.grad


# ---------------------------------------------------------------------------------------------------------------------------- losses
LOSS_KINDS = ("l2", "l1", "huber")
LOSS_D = (1 - 2.0 ** -20, 0.0, 1.0, -1.0, 1 + 2.0 ** -19, -(1 - 2.0 ** -20), -(1 + 2.0 ** -19))
LOSS_PSCALES = (-0.5, -1.25, -3.0, -0.375, -2.0)


def loss_inputs(B, chw, negative_pscale, seed=0):
    """(pred, y, pscale or None): randn * 1.5, and at up to seven places spread from the first element to the last a difference d = pred * ps - y
    of exactly 0, +-1 and just either side of +-1 (LOSS_D).  There pred has 8 significant bits and pscale at most 3, so that the product, y and
    the difference are exact in float32: the kernel's d and the float64 reference's are the same number, on the right side of every branch."""
    n = B * chw
    pred, y = torch.randn(n, generator=g(seed)) * 1.5, torch.randn(n, generator=g(seed + 1)) * 1.5
    ps = torch.tensor(LOSS_PSCALES[:B], dtype=torch.float32) if negative_pscale else None
    k = min(n, len(LOSS_D))
    for j in range(k):
        i = (j * (n - 1)) // max(k - 1, 1)
        q = float(torch.round(pred[i].clamp(-2, 2) * 64) / 64)
        prod = q * (float(ps[i // chw]) if ps is not None else 1.0)
        pred[i], y[i] = q, prod - LOSS_D[j]
        assert float(pred[i]) == q and float(y[i]) == prod - LOSS_D[j]
    return pred.view(B, chw), y.view(B, chw), ps


def loss_f64(pred, y, ps, gscale, kind):
    """(mean(norm(pred * ps - y)), gscale * d/dpred of it) in float64; sign(0) = 0 for l1, beta = 1 for huber."""
    d = pred.double() * (ps.double()[:, None] if ps is not None else 1.0) - y.double()
    n = d.numel()
    if kind == "l2":
        v, gr = d * d, 2 * d
    elif kind == "l1":
        v, gr = d.abs(), torch.sign(d)
    else:
        a = d.abs()
        v, gr = torch.where(a < 1, 0.5 * d * d, a - 0.5), torch.where(a < 1, d, torch.sign(d))
    if ps is not None:
        gr = gr * ps.double()[:, None]
    return v.mean(), gr * (gscale / n)


def loss_torch_f32(pred, y, ps, gscale, kind):
    x = pred.clone().requires_grad_(True)
    fn = {"l2": torch.nn.functional.mse_loss, "l1": torch.nn.functional.l1_loss, "huber": torch.nn.functional.smooth_l1_loss}[kind]
    loss = fn(x * ps[:, None] if ps is not None else x, y)
    (loss * gscale).backward()
    return loss.detach(), x.grad


def loss_figures(loss, dpred, ref_loss, ref_dpred):
    """The suite's: 1e-5 relative on the loss, 1e-5 of max |dpred| on the gradient."""
    rl, scale = float(ref_loss), float(ref_dpred.abs().max())
    lerr = abs(float(loss) - rl)
    derr = float((dpred.detach().double().cpu() - ref_dpred).abs().max())
    return [("loss", lerr / abs(rl) if rl != 0 else lerr, TOL_NORM), ("dpred", derr / scale if scale != 0 else derr, TOL_DPRED)]


# ----------------------------------------------------------------------------------------------------------------------------- norms
def l2norm_input(n, kind, seed=0):
    """'randn', or 'ill': 99 % of the elements at +-1e-4 and every hundredth (the first one included) at +-1e+2."""
    if kind == "randn":
        return torch.randn(n, generator=g(seed))
    x = torch.full((n,), 1e-4)
    x[::100] = 1e2
    return x * (torch.randint(0, 2, (n,), generator=g(seed)) * 2 - 1).float()


def sumsq_f64(x):
    return float((x.double() ** 2).sum())


def l2norm_figures(nsq, x):
    ref = math.sqrt(sumsq_f64(x))
    return [("norm", abs(math.sqrt(float(nsq)) - ref) / ref, TOL_NORM)]


def batch_l2norm_bound(inner):
    """Relative error of a row norm: the longest chain of float additions -- ceil(inner / 256) serial terms per thread, 6 shuffle steps and the
    2 + 1 adds of block_sum_256, the product's own rounding: ceil(inner / 256) + 10 half-ulps on the sum at most --, halved by the square root,
    plus the rounding of the root: <= (ceil(inner / 256) + 10) 2^-24."""
    return (-(-inner // 256) + 10) * 2.0 ** -24


def batch_l2norm_figures(got, x):
    ref = x.double().pow(2).sum(1).sqrt()
    return [("row norm", float(((got.detach().double().cpu() - ref).abs() / ref).max()), batch_l2norm_bound(x.shape[1]))]


# ------------------------------------------------------------------------------------------------------------------------ embeddings
def temb_inputs(B, half):
    """(t, freqs): t cycles through TEMB_T; freqs = exp(-ln(10000) k / half) (diffusers get_timestep_embedding, freq_shift = 0)."""
    t = torch.tensor([TEMB_T[i % len(TEMB_T)] for i in range(B)], dtype=torch.float32)
    return t, torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)


def temb_f64(t, freqs, flip):
    """float64 sin / cos of the float32 product t f (the argument exactly as the kernel forms it): [sin | cos], or [cos | sin] with flip."""
    a = (t.float()[:, None] * freqs.float()[None, :]).double()
    return torch.cat([torch.cos(a), torch.sin(a)] if flip else [torch.sin(a), torch.cos(a)], dim=1)


def temb_torch_f32(t, freqs, flip):
    a = t.float()[:, None] * freqs.float()[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)] if flip else [torch.sin(a), torch.cos(a)], dim=1)


def temb_figures(got, t, freqs, flip):
    """2e-6 absolute on the whole row (so a half in the wrong place fails), and each half against its own reference by name."""
    ref, half = temb_f64(t, freqs, flip), freqs.numel()
    err = (got.detach().double().cpu() - ref).abs()
    s, c = (slice(half, None), slice(0, half)) if flip else (slice(0, half), slice(half, None))
    return [("sin half", float(err[:, s].max()), TOL_TEMB), ("cos half", float(err[:, c].max()), TOL_TEMB)]


_PI_F32 = float(np.float32(math.pi))


def fourier_inputs(B, half, seed=0):
    """t log-spaced from 0.01 to 380 (one row: 380), W = 16 randn (GaussianFourierProjection, scale 16)."""
    t = torch.exp(torch.linspace(math.log(0.01), math.log(380.0), B)) if B > 1 else torch.tensor([380.0])
    return t.float(), (16 * torch.randn(half, generator=g(seed))).float()


def fourier_f64(t, W):
    """[sin(a) | cos(a)], a = ((log(t) W) 2) pi_f32: the kernel's expression on its float32 inputs and constant, in float64 throughout."""
    a = torch.log(t.double())[:, None] * W.double()[None, :] * 2.0 * _PI_F32
    return torch.cat([torch.sin(a), torch.cos(a)], dim=1)


def fourier_torch_f32(t, W):
    a = ((torch.log(t.float())[:, None] * W.float()[None, :]) * f32(2.0)) * f32(_PI_F32)
    return torch.cat([torch.sin(a), torch.cos(a)], dim=1)


def fourier_bound(t, W):
    """(4 x torch float32's worst absolute error on this case, that error): device logf / sinf may be a couple of ulps where the host's are
    under one."""
    terr = float((fourier_torch_f32(t, W).double() - fourier_f64(t, W)).abs().max())
    return 4 * terr, terr


def fourier_figures(got, t, W):
    bound, _ = fourier_bound(t, W)
    return [("sin | cos", float((got.detach().double().cpu() - fourier_f64(t, W)).abs().max()), bound)]


# ---------------------------------------------------------------------------------------- the float32 sequences that promise bit-equality
def qsample_f32(x0, R, eps, t, tab_a, tab_s, tab_step, tab_coef):
    """x_t = (a[t] x0 + s[t] eps) + step[t] R  (tab_a None, the VE form: x0 + s[t] eps), y = coef[t] R + eps; rows [B, chw]."""
    col = lambda tab: tab.float()[t][:, None]                                                 # noqa: E731
    noisy = (col(tab_a) * x0 + col(tab_s) * eps) if tab_a is not None else (x0 + col(tab_s) * eps)
    return noisy + col(tab_step) * R, col(tab_coef) * R + eps


def sched_step_f32(x, eps, z, c_eps, c_div, clip, c_x0, c_x, c_e, c_z):
    """(out, x0): x0 = (x - c_eps eps) / c_div, clamped to +-clip where clip > 0; out = c_x0 x0 + c_x x (+ c_e eps) (+ c_z z), terms with a zero
    coefficient left out as the kernel leaves them out."""
    x0 = (x - f32(c_eps) * eps) / f32(c_div)
    if clip > 0:
        x0 = torch.minimum(torch.maximum(x0, f32(-clip)), f32(clip))
    out = f32(c_x0) * x0 + f32(c_x) * x
    if float(np.float32(c_e)) != 0:
        out = out + f32(c_e) * eps
    if float(np.float32(c_z)) != 0:
        out = out + f32(c_z) * z
    return out, x0


def lincomb_f32(srcs, coefs):
    """c0 s0, then + ck sk in source order: multiply, then add."""
    acc = f32(coefs[0]) * srcs[0]
    for c, s in zip(coefs[1:], srcs[1:]):
        acc = acc + f32(c) * s
    return acc


def postprocess_f32(x, mul, add, lo, hi, to_nhwc):
    v = torch.minimum(torch.maximum(x * f32(mul) + f32(add), f32(lo)), f32(hi))
    return v.permute(0, 2, 3, 1).contiguous() if to_nhwc else v


def rowscale_f32(x, s, divide):
    return x / s[:, None] if divide else x * s[:, None]


def add_f32(dst, src, accumulate):
    return dst + src if accumulate else src.clone()


def scale_f32(x, alpha):
    return torch.zeros_like(x) if float(np.float32(alpha)) == 0 else x * f32(alpha)
