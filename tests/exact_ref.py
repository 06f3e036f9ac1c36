"""Exact references and memory guards for the split-precision kernel tests (a helper module, not a test file).

Each arithmetic of the persistent 16x16x32 kernels is an exact function of its operands:

* "bf16x3" (math 0 / 1, the default): hi = bf16(x), lo = bf16(x - hi) for both operands, three products per term,
  hi*hi + hi*lo + lo*hi;
* "f16" (math 2): one product of the f16-rounded operands;
* "bf16" (math 3): one product of the bf16-rounded operands (the hi parts);
* "f32": the plain product.

The references below contract those operands in float64 on the GPU (im2col + f64 matmul), so what is left between a kernel and
its reference is the f32 accumulation order alone.  The guard helpers place operands inside NaN and outputs inside a fixed bit
pattern, so a kernel that reads past its operand or writes past its output fails instead of adding zeros."""
import ctypes as C

import torch
import torch.nn.functional as F

from villandiffusion_amd import lib as L
from villandiffusion_amd import ops
from villandiffusion_amd.lib import B_CONV3, B_CONV3_S2, B_CONV3_T, B_CONV3_UP

DEV = "cuda"
ARITHS = ("bf16x3", "f16", "bf16", "f32")
SENTINEL = 0x5A3C96E1                   # an int32 bit pattern no kernel writes (a finite f32 of no special meaning)
NAN_PAIR = 0x7FC07FC0                   # two bf16 NaNs (and two f16 NaNs): the tail of a packed operand


def rel(a, b):
    """max |a - b| / max |b| (the suite's max-abs / max-abs relative error)."""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def split_bf16(x):
    """(hi, lo) as the split-precision format defines them: hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even."""
    x = x.float()
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def operands(t, arith):
    """The float64 parts of t that a product term multiplies, such that the term is sum_i sum_j P_i(a) P_j(b) over (i, j) in
    `pairs(arith)`."""
    if arith == "bf16x3":
        hi, lo = split_bf16(t)
        return hi.double(), lo.double()
    if arith == "f16":
        return (t.float().half().double(),)
    if arith == "bf16":
        return (t.float().bfloat16().double(),)
    return (t.double(),)


def contract(f, a, b, arith):
    """The bilinear f64 contraction f(a, b) in the given arithmetic: bf16x3 = f(a_hi, b_hi) + f(a_hi, b_lo) + f(a_lo, b_hi)."""
    pa, pb = operands(a, arith), operands(b, arith)
    if arith == "bf16x3":
        return f(pa[0], pb[0] + pb[1]) + f(pa[1], pb[0])
    return f(pa[0], pb[0])


# ---------------------------------------------------------------------------------------------------------- f64 contractions
def conv_f64(x, w, mode, chunk=16):
    """float64 3x3 convolution (padding 1) on the GPU: im2col + matmul; mode B_CONV3_UP upsamples x by nearest 2x first."""
    x, w = x.to(DEV).double(), w.to(DEV).double()
    if mode == B_CONV3_UP:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    B, _, H, W = x.shape
    wm = w.reshape(w.shape[0], -1)
    out = torch.empty(B, w.shape[0], H, W, device=DEV, dtype=torch.float64)
    for b0 in range(0, B, chunk):
        cols = F.unfold(x[b0:b0 + chunk], 3, padding=1)                      # [b, C*9, HW]
        out[b0:b0 + chunk] = torch.matmul(wm, cols).view(-1, w.shape[0], H, W)
    return out


def wgrad_cols(x, mode, taps=9, pad=0):
    """im2col of x [b, C, H, W] (float64) as the weight gradient contracts it: [b, C * taps, output pixels].  B_CONV3_S2 is the stride-2
    Downsample2D convolution: pad = 0 pads one zero column on the right and one zero row below (F.pad(x, (0, 1, 0, 1)), no further padding),
    pad = 1 is padding = 1 on every side.  Images need not be square."""
    if taps != 9:
        return x.flatten(2)
    if mode == B_CONV3_S2:
        assert pad in (0, 1), pad
        return F.unfold(F.pad(x, (0, 1, 0, 1)), 3, stride=2) if pad == 0 else F.unfold(x, 3, padding=1, stride=2)
    if mode == B_CONV3_UP:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.unfold(x, 3, padding=1)


def wgrad_f64(dy, x, mode, taps=9, chunk=16, pad=0):
    """dW[m, c*9 + t] = sum_{b,p} dy[b,m,p] * im2col(x)[b, c*9 + t, p] in float64 on the GPU (im2col: wgrad_cols)."""
    dy, x = dy.to(DEV).double(), x.to(DEV).double()
    B, M = dy.shape[:2]
    chunk = max(1, min(chunk, (1 << 25) // max(1, x.shape[1] * taps * dy.shape[2] * dy.shape[3])))      # <= 256 MB of columns at a time
    acc = 0
    for b0 in range(0, B, chunk):
        cols = wgrad_cols(x[b0:b0 + chunk], mode, taps, pad)
        acc = acc + torch.einsum("bmp,bkp->mk", dy[b0:b0 + chunk].flatten(2), cols)
    return acc


def conv3_f64(x, w, mode, arith, bias=None, rowadd=None, residual=None, acc=None, pool2=False):
    """What vd_gemm computes for a 3x3 convolution of x [B, C, H, W] with the FORWARD weights w [M_fwd, C_fwd, 3, 3]:
    mode B_CONV3 / B_CONV3_UP: conv(x, w); B_CONV3_T (flipped taps, the input gradient): conv(x, flip(w)^T).  Folded GroupNorm
    (mode 3 of the kernel) is B_CONV3 of the loader's activation: pass that activation as x.  pool2: the 2x2 block sums of the
    result.  The epilogue adds bias [M], rowadd [B, M], residual [B, M, OH, OW] and the accumulated output `acc`."""
    w = w.to(DEV)
    if mode == B_CONV3_T:
        w = w.transpose(0, 1).flip(2, 3)
    y = contract(lambda a, b: conv_f64(b, a, B_CONV3_UP if mode == B_CONV3_UP else B_CONV3), w, x.to(DEV), arith)
    if pool2:
        y = y.view(y.shape[0], y.shape[1], y.shape[2] // 2, 2, y.shape[3] // 2, 2).sum((3, 5))
    return _epilogue(y, bias, rowadd, residual, acc)


def gemm1x1_f64(x, w, arith, bias=None, residual=None, acc=None):
    """1x1 convolution of x [B, C, H, W] with w [M, C]."""
    y = contract(lambda a, b: torch.einsum("mc,bcp->bmp", a, b.flatten(2)), w.to(DEV), x.to(DEV), arith)
    return _epilogue(y.view(x.shape[0], w.shape[0], x.shape[2], x.shape[3]), bias, None, residual, acc)


def wgrad_arith_f64(dy, x, mode, arith, taps=9, acc=None, pad=0):
    """Weight gradient dW [M, C*taps] of a 3x3 (mode B_CONV3 / B_CONV3_UP / B_CONV3_S2 with its `pad`) or 1x1 (taps = 1) convolution in the
    given arithmetic."""
    y = contract(lambda a, b: wgrad_f64(a, b, mode, taps, pad=pad), dy.to(DEV), x.to(DEV), arith)
    return y if acc is None else y + acc.to(DEV).double()


def _epilogue(y, bias, rowadd, residual, acc):
    if bias is not None:
        y = y + bias.to(DEV).double().view(1, -1, 1, 1)
    if rowadd is not None:
        y = y + rowadd.to(DEV).double().view(y.shape[0], y.shape[1], 1, 1)
    if residual is not None:
        y = y + residual.to(DEV).double()
    if acc is not None:
        y = y + acc.to(DEV).double()
    return y


def gn_part_f64(out, TW):
    """Per 256-pixel tile (TR = 256 / TW rows x TW columns, tiles in row-major order) and channel: (sum, sum of squares) in float64
    of the kernel's own output out [B, M, OH, OW] -> [B, tiles, M, 2] (vd_gemm_desc.gn_part)."""
    B, M, OH, OW = out.shape
    TR = 256 // TW
    v = out.double().view(B, M, OH // TR, TR, OW // TW, TW)
    s, s2 = v.sum((3, 5)), (v * v).sum((3, 5))                                       # [B, M, ty, tx]
    return torch.stack([s, s2], -1).flatten(2, 3).permute(0, 2, 1, 3)               # [B, tiles, M, 2]


def gn_silu_operand(x, ss):
    """The folded GroupNorm loader's f32 operand as torch computes it: (z, silu(z)) with z = x * scale + shift rounded once, as the
    kernel's FMA does (the f64 product of two f32 values is exact).  ss: [B, C, 2] (scale, shift) from ops.groupnorm_stats."""
    z = (x.double() * ss[:, :, 0, None, None].double() + ss[:, :, 1, None, None].double()).float()
    return z, z * torch.sigmoid(z)


def rounding_ambiguity(a, z, arith):
    """The kernel computes silu with a hardware exp and reciprocal, so its f32 operand lies a few f32 ulps from torch's `a`: about
    |z| ulps from the rounded exp argument plus a handful from exp, reciprocal and product.  Within a window of 16 + 4|z| ulps of
    `a`, a value may round to the other neighbour in the arithmetic's format.  Returns, per operand, the distance between the two
    possible rounded values (float64; 0 where both ends of the window round alike, and everywhere for bf16x3 / f32, whose lo part or
    full precision absorbs the difference)."""
    if arith not in ("f16", "bf16"):
        return torch.zeros_like(a, dtype=torch.float64)
    rnd = (lambda t: t.half().double()) if arith == "f16" else (lambda t: t.bfloat16().double())
    mag = a.abs()
    d = (16 + 4 * z.abs().double()) * (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
    r0 = rnd(a)
    return torch.maximum((rnd((a.double() - d).float()) - r0).abs(), (rnd((a.double() + d).float()) - r0).abs())


def rel_bounded(got, ref, bound):
    """rel() of what exceeds a per-element bound: max(|got - ref| - bound, 0) / max |ref|."""
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    return float(((got - ref).abs() - bound.to(got.device)).clamp(min=0).max() / (ref.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------ guards
def _nan_buffer(numel):
    return torch.full((numel,), float("nan"), device=DEV)


def nan_slice(x, pre=8, post=8, tail=4096):
    """A copy of x [B, C, H, W] placed as channels [pre, pre + C) of a NaN-filled [B, pre + C + post, H, W] buffer followed by
    `tail` more NaN floats: NaN channels on both sides, in the batch-stride gap and after the last image.  pre / post are whole
    channel octets, so the slice keeps the 16-byte alignment (and the octet offsets of a pre-split image)."""
    B, Cc, H, W = x.shape
    Ct = pre + Cc + post
    buf = _nan_buffer(B * Ct * H * W + tail)
    v = buf[:B * Ct * H * W].view(B, Ct, H, W)[:, pre:pre + Cc]
    v.copy_(x)
    return v


def nan_presplit(x, pre=8, post=8, tail=4096):
    """The pre-split image of x written into the channel slice of a NaN-filled buffer (as nan_slice): every unit outside the slice
    reads as (bf16 NaN, 0)."""
    v = nan_slice(torch.zeros_like(x), pre, post, tail)
    return ops.presplit_pack(x.to(DEV), out=ops.PreSplit(v))


def nan_vector(v, tail=64):
    """v (1-D or [B, n] rows) with NaN after it (rows: NaN between rows and after the last one) -> (view, row stride)."""
    v = v.to(DEV)
    if v.dim() == 1:
        buf = _nan_buffer(v.numel() + tail)
        buf[:v.numel()].copy_(v)
        return buf[:v.numel()], v.numel()
    B, n = v.shape
    ld = n + tail
    buf = _nan_buffer(B * ld + tail)
    out = buf[:B * ld].view(B, ld)[:, :n]
    out.copy_(v)
    return out, ld


def packed_guarded(w2d, M, Cc, transposed=False, taps=9, f16=False, tail=1024):
    """Split-precision (or f16) operand of w2d in a buffer of exactly vd_conv3_packed_bytes (half of it for f16) plus a tail of
    NaN pairs -> (operand view, whole buffer, operand int32 count)."""
    nbytes = L.load().vd_conv3_packed_bytes(M, Cc, taps) // (2 if f16 else 1)
    assert nbytes > 0 and nbytes % 16 == 0
    n = nbytes // 4
    buf = torch.full((n + tail,), NAN_PAIR, device=DEV, dtype=torch.int32)
    if not f16:
        ops.conv3_pack_weights(w2d, M, Cc, transposed=transposed, out=buf[:n], taps=taps)
    else:
        rs, cs = (taps, M * taps) if transposed else (Cc * taps, taps)
        mpad = (M + 127) // 128 * 128
        tab = torch.tensor([[w2d.data_ptr(), buf.data_ptr(), M, Cc, rs, cs, 0, taps]], dtype=torch.int64).to(DEV)
        ops.conv3_pack_weights_f16_multi(tab, 1, (mpad * (Cc // 16) * 2 + 255) // 256)
        torch.cuda.synchronize()
    assert bool((buf[n:] == NAN_PAIR).all()), "the packer wrote past vd_conv3_packed_bytes"
    return buf[:n], buf, n


class GuardedOut:
    """An output [B, M, H, W] as channels [pre, pre + M) of a [B, pre + M + post, H, W] buffer (+ tail) whose every other word holds
    SENTINEL.  `fresh(init)` refills the slice -- with NaN, or with `init` for an accumulating case -- and re-arms the sentinel;
    `intact()` checks the surroundings through an int32 view."""

    def __init__(self, B, M, H, W, pre=4, post=4, tail=4096):
        self.shape, self.pre = (B, M, H, W), pre
        Ct = pre + M + post
        self.n = B * Ct * H * W
        self.buf = torch.empty(self.n + tail, device=DEV)
        self.view = self.buf[:self.n].view(B, Ct, H, W)[:, pre:pre + M]
        self.mask = torch.ones(self.n + tail, dtype=torch.bool, device=DEV)
        self.mask[:self.n].view(B, Ct, H, W)[:, pre:pre + M] = False

    def fresh(self, init=None):
        self.buf.view(torch.int32).fill_(SENTINEL)
        if init is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(init)
        return self.view

    def intact(self):
        return bool((self.buf.view(torch.int32)[self.mask] == SENTINEL).all())


class GuardedFlat:
    """A flat float buffer `view` of exactly n floats between a SENTINEL head of `pre` floats (16-byte aligned) and a SENTINEL tail
    (split-K / group workspaces, weight gradients, gn_part): a store before the first or after the last element shows in intact()."""

    def __init__(self, n, pre=64, tail=4096, fill=float("nan")):
        self.n, self.pre, self.fill = n, pre, fill
        self.buf = torch.empty(pre + n + tail, device=DEV)
        self.view = self.buf[pre:pre + n]
        self.arm()

    def arm(self):
        self.buf.view(torch.int32).fill_(SENTINEL)
        self.view.fill_(self.fill)
        return self.view

    def intact(self):
        raw = self.buf.view(torch.int32)
        return bool((raw[:self.pre] == SENTINEL).all()) and bool((raw[self.pre + self.n:] == SENTINEL).all())


def wgrad_group_ws_floats(descs):
    """The workspace floats vd_conv_wgrad_group_plan asks for this job list (what ops.conv_wgrad_group allocates at least)."""
    lib = L.load()
    n = len(descs)
    arr = (L.WgradDesc * n)(*descs)
    host = (C.c_uint8 * (n * int(lib.vd_conv_wgrad_group_job_bytes())))()
    wsf, blocks, rblocks = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    cls = lib.vd_conv_wgrad_group_plan(arr, n, host, C.byref(wsf), C.byref(blocks), C.byref(rblocks))
    assert cls > 0, L.last_error()
    return int(wsf.value), int(blocks.value)
