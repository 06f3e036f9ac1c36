"""Tensor-level wrappers over the C ABI (include/villan_hip.h).

torch is plumbing here: it owns device memory and the current HIP stream; every computation below is one of
the hand-written gfx950 kernels.  Image tensors are [B, C, H, W] views whose (C, H, W) part is contiguous and
whose batch stride may be larger than C*H*W (channel slices of a concat buffer).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from typing import Optional, Sequence

import torch

from . import lib as L
from .lib import (A_COL, A_ROW, B_CONV3, B_CONV3_DIL, B_CONVG, B_CONV3_S2, B_CONV3_T, B_CONV3_UP, B_KCONTIG, B_PLAIN,
                  GemmDesc, WgradDesc)


def _lib():
    L.require_device()
    return L.load()


# ---- optional per-launch timing of the MFMA kernels (bench.py roofline leg): HIP events on the launch stream ----
_PROF = None          # list of (kernel_symbol, algorithmic_flops, start_event, end_event) while enabled


def _kernel_name(query, what) -> str:
    """The recorded name of a launch: the library writes the instantiation its own launch branch names (vd_*_kernel_name, host only)."""
    buf = C.create_string_buffer(128)
    L.check(min(query(what, buf, len(buf)), 0), "kernel name query")
    return buf.value.decode()


def profile_start():
    global _PROF
    _PROF = []


def profile_stop():
    global _PROF
    rec, _PROF = _PROF, None
    return rec


def _s() -> int:
    return torch.cuda.current_stream().cuda_stream


def _timed(name, amount, kind, call, nbytes=None):
    """Run `call()`; while profiling is on, bracket it with HIP events on the launch stream and record a dict
    {name, flops, bytes, e0, e1, kind}: kind "mfma" -> amount = algorithmic FLOPs (nbytes = algorithmic bytes, optional),
    kind "hbm" -> amount = algorithmic bytes (every operand read once / written once)."""
    if _PROF is None:
        return call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = call()
    e1.record()
    _PROF.append({"name": name, "flops": float(amount) if kind == "mfma" else 0.0, "bytes": float(nbytes if nbytes is not None else (amount if kind == "hbm" else 0.0)),
                  "e0": e0, "e1": e1, "kind": kind})
    return r


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _img(t: torch.Tensor):
    """(B, C, H, W, bstride) of an image view; inner CHW must be contiguous."""
    assert t.dtype == torch.float32 and t.dim() == 4, (t.dtype, t.shape)
    B, Cc, H, W = t.shape
    st = t.stride()
    assert (st[1], st[2], st[3]) == (H * W, W, 1) or Cc * H * W == 0, f"inner CHW not contiguous: {t.shape} {st}"
    return B, Cc, H, W, (st[0] if B > 1 else Cc * H * W)


# --------------------------------------------------------------------------------------------- pre-split activation images
class PreSplit:
    """A [B, C, H, W] activation held as its PRE-SPLIT image (include/villan_hip.h "PRE-SPLIT activation images": per pixel and channel octet the
    bf16 hi / lo halves the split-precision kernels contract, written once by the producer).  `t` is the float32 tensor whose storage carries the
    image: same shape, bytes, batch stride and channel-octet offsets as the f32 tensor it replaces -- only the meaning of the bytes differs, so
    nothing but a kernel that declares a pre-split operand may read it."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        assert t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] % 8 == 0, (t.dtype, t.shape)
        self.t = t

    shape = property(lambda self: self.t.shape)
    device = property(lambda self: self.t.device)

    def stride(self, *a):
        return self.t.stride(*a)

    def data_ptr(self):
        return self.t.data_ptr()

    def channels(self, lo: int, hi: int) -> "PreSplit":
        """The channel slice [lo, hi) (whole octets): an O8 image of a channel range is the same bytes as the f32 slice."""
        assert lo % 8 == 0 and hi % 8 == 0
        return PreSplit(self.t[:, lo:hi])


def _unwrap(x):
    """(tensor, is_presplit)"""
    return (x.t, True) if isinstance(x, PreSplit) else (x, False)


def presplit_empty(shape, device) -> PreSplit:
    return PreSplit(torch.empty(shape, device=device, dtype=torch.float32))


def presplit_pack(x: torch.Tensor, out: Optional[PreSplit] = None) -> PreSplit:
    Bn, Cc, H, W, xbs = _img(x)
    out = presplit_empty(x.shape, x.device) if out is None else out
    assert tuple(out.shape) == tuple(x.shape)
    _timed("presplit_pack (presplit_pack_kernel)", 8.0 * x.numel(), "hbm", lambda: L.check(
        _lib().vd_presplit_pack(_p(x), _p(out.t), Bn, Cc, H * W, xbs, _img(out.t)[4], _s()), "vd_presplit_pack"))
    return out


def presplit_unpack(y: PreSplit, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    Bn, Cc, H, W, ybs = _img(y.t)
    out = torch.empty(y.shape, device=y.device, dtype=torch.float32) if out is None else out
    L.check(_lib().vd_presplit_unpack(_p(y.t), _p(out), Bn, Cc, H * W, ybs, _img(out)[4], _s()), "vd_presplit_unpack")
    return out


def groupnorm_presplit_ok(Cc: int, HW: int, G: int) -> bool:
    return bool(_lib().vd_groupnorm_fwd_presplit_ok(Cc, HW, G))


def groupnorm_fwd_presplit(x, gamma, beta, y: PreSplit, mean, rstd, G, eps, silu) -> PreSplit:
    """y = the pre-split image of silu?(GroupNorm(x)); mean / rstd as groupnorm_fwd."""
    Bn, Cc, H, W, xbs = _img(x)
    assert tuple(y.shape) == tuple(x.shape) and mean.numel() >= Bn * G and rstd.numel() >= Bn * G
    _timed("groupnorm_fwd_presplit (gn_fwd_ps_kernel<*>)", 8.0 * x.numel(), "hbm", lambda: L.check(
        _lib().vd_groupnorm_fwd_presplit(_p(x), _p(gamma), _p(beta), _p(y.t), _p(mean), _p(rstd), Bn, Cc, H * W, G, eps, int(silu), xbs,
                                         _img(y.t)[4], _s()), "vd_groupnorm_fwd_presplit"))
    return y


# ---- shape-only questions to the library's planners (vd_gemm_tile, vd_conv_wgrad_plan, vd_conv_wgrad_group_class: host functions, no device): the one
# place that picks a kernel.  The predicates build a placeholder descriptor -- contiguous NCHW at 16-byte aligned dummy addresses -- and ask once per shape.
_FAKE_PTR = 0x10000
_BX3_TILES = (8, 12, 15, 16, 18, 20)           # vd_gemm_tile() of the split-precision 3x3 convolutions; 9 / 11 / 13 / 19: 1x1 and plain products; 10: activations


def _src_side(mode, s):
    """Side of the gather's source under an output side."""
    return s // 2 if mode == B_CONV3_UP else (2 * s if mode == B_CONV3_S2 else s)


def conv_query_desc(M, Cc, OH, OW, mode, nb=1, **flags) -> GemmDesc:
    """vd_gemm_desc of a 3x3 convolution Cc -> M with OH x OW outputs and a packed weight operand; flags: further fields (math, pool2, b_presplit, ...)."""
    H, W = _src_side(mode, OH), _src_side(mode, OW)
    d = GemmDesc()
    d.A = d.B = d.D = d.a_packed = _FAKE_PTR
    d.a_packed_mpad = (M + 127) // 128 * 128
    d.M, d.N, d.K, d.NP = M, nb * OH * OW, Cc * 9, OH * OW
    d.a_mode, d.b_mode, d.alpha = A_ROW, mode, 1.0
    d.C, d.H, d.W, d.OH, d.OW = Cc, H, W, OH, OW
    d.lda, d.b_bstride = Cc * 9, Cc * H * W
    d.ldd = (OH // 2) * (OW // 2) if flags.get("pool2") else OH * OW          # (pool2 writes D at half resolution)
    d.d_bstride = M * d.ldd
    for k, v in flags.items():
        setattr(d, k, v)
    return d


def product_query_desc(M, K, NP, nb=1, a_mode=A_ROW, b_mode=B_PLAIN, act=False) -> GemmDesc:
    """vd_gemm_desc of D[b] = A @ B[b] ([M, K] x [K, NP]).  act=False: shared A with a packed operand (1x1 convolutions, projections);
    act=True: a product of two activation matrices -- per-batch A, math = 1, nothing packed."""
    d = GemmDesc()
    d.A = d.B = d.D = _FAKE_PTR
    d.M, d.N, d.K, d.NP = M, nb * NP, K, NP
    d.a_mode, d.b_mode, d.alpha = a_mode, b_mode, 1.0
    d.lda = K if a_mode == A_ROW else M
    d.ldb = K if b_mode == B_KCONTIG else NP
    d.b_bstride, d.ldd, d.d_bstride = K * NP, NP, M * NP
    if act:
        d.math, d.a_bstride = 1, M * K
    else:
        d.a_packed, d.a_packed_mpad = _FAKE_PTR, (M + 127) // 128 * 128
    return d


def wgrad_query_desc(M, Cc, OH, OW, mode, nb=1, math_mode=1, **flags) -> WgradDesc:
    """vd_wgrad_desc of the weight gradient of a convolution Cc -> M with OH x OW outputs (mode B_PLAIN: 1x1, else 3x3)."""
    d = WgradDesc()
    d.dY = d.X = d.dW = _FAKE_PTR
    d.M, d.C, d.T, d.nb, d.NP = M, Cc, 1 if mode == B_PLAIN else 9, nb, OH * OW
    d.H, d.W, d.OH, d.OW = _src_side(mode, OH), _src_side(mode, OW), OH, OW
    d.mode, d.math = mode, math_mode
    d.dy_bstride, d.x_bstride = M * OH * OW, Cc * d.H * d.W
    for k, v in flags.items():
        setattr(d, k, v)
    return d


def _gemm_tile(d: GemmDesc) -> int:
    return int(L.load().vd_gemm_tile(C.byref(d)))


def _wgrad_tile(d: WgradDesc) -> int:
    tile, splits = C.c_int32(0), C.c_int32(0)
    L.load().vd_conv_wgrad_plan(C.byref(d), C.byref(tile), C.byref(splits))
    return tile.value


@functools.lru_cache(maxsize=None)
def conv_presplit_ok(Bn: int, Cin: int, Cout: int, OH: int, OW: int, mode: int) -> bool:
    """Would conv3x3(PreSplit input [Bn, Cin, ..] -> [Bn, Cout, OH, OW], mode, a_packed=...) be taken by the persistent 16x16x32 kernel, the only
    reader of pre-split images?  (vd_gemm_tile() == 18 with b_presplit = 1.)"""
    return _gemm_tile(conv_query_desc(Cout, Cin, OH, OW, mode, Bn, b_presplit=1)) == 18


@functools.lru_cache(maxsize=None)
def wgrad_presplit_ok(Bn: int, Cin: int, Cout: int, S: int, mode: int = B_CONV3) -> bool:
    """Is there a grouped pre-split weight-gradient kernel for a 3x3 convolution Cin -> Cout with S x S OUTPUTS (mode B_CONV3 or B_CONV3_UP)?"""
    d = wgrad_query_desc(Cout, Cin, S, S, mode, Bn, accumulate=1, presplit=3)
    return int(L.load().vd_conv_wgrad_group_class(C.byref(d))) >= 3000


def groupnorm_bwd_presplit(dy, x, mean, rstd, gamma, beta, dx, dx_ps, dgamma_ws, dbeta_ws, G, silu, extra=None, extra2=None, rowsum=None,
                           rowsum_ld=None):
    """groupnorm_bwd whose dx goes out as f32 (`dx`, may be None), as a pre-split image (`dx_ps`: PreSplit, may be None) or both."""
    Bn, Cc, H, W, xbs = _img(x)
    dbs = _img(dy)[4]
    assert dx is not None or dx_ps is not None
    dxbs = _img(dx)[4] if dx is not None else 0
    psbs = _img(dx_ps.t)[4] if dx_ps is not None else 0
    assert dx is None or dx.shape == x.shape
    assert dx_ps is None or tuple(dx_ps.shape) == tuple(x.shape)
    ebs = _img(extra)[4] if extra is not None else 0
    e2bs = _img(extra2)[4] if extra2 is not None else 0
    assert dgamma_ws.numel() >= Bn * Cc and dbeta_ws.numel() >= Bn * Cc
    assert (extra is None or extra.shape == x.shape) and (extra2 is None or extra2.shape == x.shape)
    rld = 0
    if rowsum is not None:
        rld = Cc if rowsum_ld is None else rowsum_ld
        assert rld >= Cc
    nbytes = (8.0 + (4.0 if dx is not None else 0.0) + (4.0 if dx_ps is not None else 0.0) + (4.0 if extra is not None else 0.0)
              + (4.0 if extra2 is not None else 0.0)) * x.numel()
    _timed("groupnorm_bwd_presplit (gn_bwd_ps_kernel<*>)", nbytes, "hbm", lambda: L.check(
        _lib().vd_groupnorm_bwd_presplit(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(extra), _p(extra2), _p(dx),
                                         _p(dx_ps.t) if dx_ps is not None else None, _p(dgamma_ws), _p(dbeta_ws), _p(rowsum), Bn, Cc, H * W, G,
                                         int(silu), dbs, xbs, ebs, e2bs, dxbs, psbs, rld, _s()), "vd_groupnorm_bwd_presplit"))
    return dx_ps if dx_ps is not None else dx


# --------------------------------------------------------------------------------------------- GEMM family
_GEMM_WS = {}
_WS_SLOT = 0
AUX_WS_SLOT = -1       # the UNet's auxiliary stream (unet.aux_scope): outside the non-negative slots pipelines.sample_concurrent hands to its streams


class ws_slot:
    """Launch sequences that run CONCURRENTLY on different streams (the sampler's interleaved chunks, pipelines.sample_concurrent) must not share
    the split-K workspace: each takes its own slot.  `with ops.ws_slot(k): ...` around everything that launches (or captures) on that stream."""

    def __init__(self, slot: int):
        self.slot, self.prev = int(slot), 0

    def __enter__(self):
        global _WS_SLOT
        self.prev, _WS_SLOT = _WS_SLOT, self.slot
        return self

    def __exit__(self, *exc):
        global _WS_SLOT
        _WS_SLOT = self.prev
        return False


def gemm_ws_buffer(device, slot: int = None):
    """The current split-K workspace tensor of (device, slot), or None (graph owners compare it by identity to know their capture is still valid)."""
    return _GEMM_WS.get((device, _WS_SLOT if slot is None else slot))


def _gemm_ws(n_floats: int, device):
    """Per-(device, slot) split-K workspace, grown on demand (launches on one stream are ordered, so one stream's launches share it)."""
    key = (device, _WS_SLOT)
    t = _GEMM_WS.get(key)
    if t is None or t.numel() < n_floats:
        t = torch.empty(max(n_floats, 1 << 22), device=device, dtype=torch.float32)
        _GEMM_WS[key] = t
    return t


def gemm(A, B, D, *, M, N, K, a_mode=A_ROW, b_mode=B_PLAIN, NP=None, lda=0, a_bstride=0, ldb=0, b_bstride=0,
         ldd=0, d_bstride=0, bias=None, bias_on_n=False, rowadd=None, rowadd_bstride=0, residual=None,
         res_bstride=0, conv=None, alpha=1.0, d_trans=False, accumulate=False, tile=0, debug=0, pad=0, nb2=0, a_b2stride=0,
         b_b2stride=0, d_b2stride=0, gn_ss=None, a_packed=None, math_mode=0, pool2=False, convg=None, act=0, gn_part=None, b_presplit=False):
    """gn_part: optional [B, NP // 256, M, 2] buffer for the per-tile channel sums of the result (vd_gemm_desc.gn_part); it is filled only when the
    launch goes to the persistent 16x16x32 split-precision convolution -- ops.GN_PART_WRITTEN tells the caller right after the call."""
    global GN_PART_WRITTEN
    d = GemmDesc()
    d.act = act
    d.b_presplit = int(b_presplit)
    if convg is not None:
        d.kh, d.kw, d.conv_stride, d.pad_h, d.pad_w = convg
    d.pad = pad
    d.pool2 = int(pool2)
    d.math = math_mode
    a_packed16, alt_math = None, 2
    if isinstance(a_packed, tuple):            # (split-precision operand, single-product operand[, math]): opt-in mixed precision, decided per problem below
        a_packed, a_packed16, *rest = a_packed # (f16: the f16 operand, math 2; bf16: the split-precision operand again, math 3)
        alt_math = rest[0] if rest else 2
    if a_packed is not None:
        d.a_packed, d.a_packed_mpad = a_packed.data_ptr(), (M + 127) // 128 * 128
    d.gn_ss = _p(gn_ss)
    d.nb2, d.a_b2stride, d.b_b2stride, d.d_b2stride = nb2, a_b2stride, b_b2stride, d_b2stride
    d.A, d.B, d.D = _p(A), _p(B), _p(D)
    d.bias, d.rowadd, d.residual = _p(bias), _p(rowadd), _p(residual)
    d.M, d.N, d.K = M, N, K
    d.a_mode, d.b_mode = a_mode, b_mode
    d.NP = N if NP is None else NP
    if conv is not None:
        d.C, d.H, d.W, d.OH, d.OW = conv
    d.bias_on_n, d.d_trans, d.accumulate, d.tile = int(bias_on_n), int(d_trans), int(accumulate), tile
    d.alpha = alpha
    d.debug = debug
    d.lda, d.a_bstride, d.ldb, d.b_bstride = lda, a_bstride, ldb, b_bstride
    d.ldd, d.d_bstride, d.res_bstride, d.rowadd_bstride = ldd, d_bstride, res_bstride, rowadd_bstride
    lib = _lib()
    need = lib.vd_gemm_ws_floats(C.byref(d))
    if need > 0:
        d.ws = _gemm_ws(need, D.device).data_ptr()
    elif FORCE_WS is not None:                 # diagnostic builds only (tools/k32p_stamps.py: the stamp buffer travels in the unused ws pointer)
        d.ws = FORCE_WS.data_ptr()
    global LAST_GEMM_TILE, LAST_GEMM_MATH
    if a_packed16 is not None and (gn_part is None or alt_math == 3):
        # single-product operands are read by the persistent 16x16x32 kernels only (vd_gemm_tile 18 / 19 with math = 2; 18 / 19 / 20 with
        # math = 3), the library answers -1 for every other problem: that keeps the split-precision operand
        d.a_packed, d.math = a_packed16.data_ptr(), alt_math
        if lib.vd_gemm_tile(C.byref(d)) not in ((18, 19) if alt_math == 2 else (18, 19, 20)):
            d.a_packed, d.math = a_packed.data_ptr(), math_mode
    LAST_GEMM_MATH = d.math
    LAST_GEMM_TILE = lib.vd_gemm_tile(C.byref(d))            # kernel family the library picks for this problem (tests assert on it)
    GN_PART_WRITTEN = gn_part is not None and not pool2 and LAST_GEMM_TILE == 18
    if GN_PART_WRITTEN:
        assert gn_part.is_contiguous() and gn_part.numel() >= (N // 256) * M * 2
        d.gn_part = gn_part.data_ptr()
    if _PROF is None:
        L.check(lib.vd_gemm(C.byref(d), _s()), "vd_gemm")
        return D
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.check(lib.vd_gemm(C.byref(d), _s()), "vd_gemm")
    e1.record()
    flops = 2.0 * M * N * K * (0.25 if b_mode == B_CONV3_DIL else 1.0)     # DIL: 3/4 of the taps are structural zeros
    # algorithmic bytes: B (the activation operand) read once, D written once (+ residual read), A read once
    if conv is not None:
        nb_ = N // d.NP
        b_elems = nb_ * d.C * d.H * d.W
        a_elems = M * K
    else:
        b_elems = K * N
        a_elems = M * K * (N // d.NP if a_bstride else 1)
    d_elems = M * N // (4 if pool2 else 1)
    nbytes = 4.0 * (b_elems + d_elems * (2 if residual is not None else 1) + a_elems)
    name = _kernel_name(lib.vd_gemm_kernel_name, C.byref(d))
    _PROF.append({"name": name, "flops": flops, "bytes": nbytes, "e0": e0, "e1": e1, "kind": "mfma", "shape": (M, K, d.NP, N // d.NP, d.OH, d.OW)})
    return D


_CONV_OUT = {B_CONV3: lambda h, w: (h, w), B_CONV3_T: lambda h, w: (h, w), B_CONV3_S2: lambda h, w: (h // 2, w // 2),
             B_CONV3_UP: lambda h, w: (2 * h, 2 * w), B_CONV3_DIL: lambda h, w: (2 * h, 2 * w)}


def conv3_pack_weights(w2d, M, Cc, transposed=False, out=None, taps=9):
    """Split-precision operand of conv3x3 / conv1x1 (a_packed=...): the [M, Cc*taps] weights as bf16 (hi, lo) pairs in MFMA
    fragment order.  transposed=True packs the dgrad operand A'[c_in][m_out] straight from the forward weights w2d
    [m_out, c_in*taps] (then M = c_in, Cc = m_out)."""
    lib = _lib()
    nbytes = lib.vd_conv3_packed_bytes(M, Cc, taps)
    assert nbytes > 0, (M, Cc, taps)
    if out is None:
        out = torch.empty(nbytes // 4, device=w2d.device, dtype=torch.int32)
    assert out.numel() * out.element_size() >= nbytes and w2d.is_contiguous()
    rs, cs = (taps, M * taps) if transposed else (Cc * taps, taps)
    L.check(lib.vd_conv3_pack_weights(_p(w2d), _p(out), M, Cc, taps, rs, cs, _s()), "vd_conv3_pack_weights")
    return out


def conv3_pack_weights_f16(w2d, M, Cc, transposed=False, taps=9):
    """f16 operand (vd_gemm_desc.math = 2) of ONE convolution -- tests and tools; the network packs all of them in one launch
    (unet._PackedConvWeights(f16=True)).  Pass it to conv3x3 / conv1x1 / gemm as a_packed=(split-precision operand, this)."""
    nbytes = _lib().vd_conv3_packed_bytes(M, Cc, taps) // 2
    assert nbytes > 0 and w2d.is_contiguous(), (M, Cc, taps)
    out = torch.empty(nbytes // 4, device=w2d.device, dtype=torch.int32)
    rs, cs = (taps, M * taps) if transposed else (Cc * taps, taps)
    mpad = (M + 127) // 128 * 128
    tab = torch.tensor([[w2d.data_ptr(), out.data_ptr(), M, Cc, rs, cs, 0, taps]], dtype=torch.int64).to(w2d.device)
    conv3_pack_weights_f16_multi(tab, 1, (mpad * (Cc // 16) * 2 + 255) // 256)
    torch.cuda.current_stream(w2d.device).synchronize()       # the one-row table is a temporary
    return out


def conv3_pack_weights_f16_multi(table, n_jobs, total_blocks):
    """The same job table, f16 operands (vd_gemm_desc.math = 2): half the bytes per job."""
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= 8 * n_jobs
    L.check(_lib().vd_conv3_pack_weights_f16_multi(_p(table), n_jobs, total_blocks, _s()), "vd_conv3_pack_weights_f16_multi")


def conv3_pack_weights_multi(table, n_jobs, total_blocks):
    """table: device int64 [n_jobs, 8] = (W address, packed address, M, C, row_stride, chan_stride, first workgroup, 0)."""
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= 8 * n_jobs
    L.check(_lib().vd_conv3_pack_weights_multi(_p(table), n_jobs, total_blocks, _s()), "vd_conv3_pack_weights_multi")


# Bumped by every raw-pointer parameter update (vd_adam_step writes behind torch's version counters): caches derived from the
# weights (packed split-precision operands) key on (flat_param._version, WEIGHTS_EPOCH).
WEIGHTS_EPOCH = 0


@functools.lru_cache(maxsize=None)
def bx3_eligible(M, Cc, OH, OW, mode) -> bool:
    """Problems the split-precision convolution kernels take (vd_gemm_desc.a_packed; OH, OW: the OUTPUT)."""
    return _gemm_tile(conv_query_desc(M, Cc, OH, OW, mode)) in _BX3_TILES


@functools.lru_cache(maxsize=None)
def bx3_pool2_eligible(M, Cc, OH, OW, nb) -> bool:
    """The split-precision stride-1 dgrad can add the 2x2 blocks of its output in the epilogue (vd_gemm_desc.pool2): 16x16 / 32x32 outputs
    on an unsplit grid (>= 256 tiles of 128 channels x 128 pixels; below that the kernel splits the channel loop over workgroups).  The persistent
    kernel would also take it on the wider images it walks; the network keeps its separate 2x2 sum there, as it always has (OW <= 32)."""
    return _gemm_tile(conv_query_desc(M, Cc, OH, OW, B_CONV3_T, nb, pool2=1)) in _BX3_TILES and OW <= 32


GN_PART_WRITTEN = False
LAST_GEMM_TILE = 0
LAST_GEMM_MATH = 0
FORCE_WS = None


def conv3x3(x, w2d, bias, out, mode=B_CONV3, rowadd=None, rowadd_bstride=0, residual=None, accumulate=False, tile=0, debug=0,
            pad=0, gn_ss=None, a_packed=None, pool2=False, gn_part=None):
    """out[b] = W (*) gather_mode(x[b]) + bias (+ rowadd[b,:,None,None]) (+ residual).  w2d: [M, C*9].
    pad: stride-2 mode only (0: zero pad (0,1,0,1); 1: symmetric padding 1).
    pool2 (B_CONV3_T with a_packed only): `out` has HALF the resolution and receives the 2x2 block sums of the result."""
    x, ps = _unwrap(x)                          # a PreSplit input: the persistent 16x16x32 kernel copies its (hi, lo) units (vd_gemm_desc.b_presplit)
    Bn, Cc, H, W, xbs = _img(x)
    M = w2d.shape[0]
    assert w2d.shape[1] == Cc * 9 and w2d.is_contiguous()
    OH, OW = _CONV_OUT[mode](H, W)
    Bo, Mo, OHo, OWo, obs = _img(out)
    if pool2:
        assert (Bo, Mo, OHo, OWo) == (Bn, M, OH // 2, OW // 2) and mode == B_CONV3_T and a_packed is not None, (out.shape, (Bn, M, OH, OW))
        assert bias is None and rowadd is None and residual is None and not accumulate
    else:
        assert (Bo, Mo, OHo, OWo) == (Bn, M, OH, OW), (out.shape, (Bn, M, OH, OW))
    rbs = 0
    if residual is not None:
        rbs = _img(residual)[4]
        assert residual.shape == out.shape
    return gemm(w2d, x, out, M=M, N=Bn * OH * OW, K=Cc * 9, b_mode=mode, NP=OH * OW, lda=Cc * 9, b_bstride=xbs,
                ldd=OHo * OWo, d_bstride=obs, bias=bias, rowadd=rowadd, rowadd_bstride=rowadd_bstride,
                residual=residual, res_bstride=rbs, conv=(Cc, H, W, OH, OW), accumulate=accumulate, tile=tile, debug=debug,
                pad=pad, gn_ss=gn_ss, a_packed=a_packed, pool2=pool2, gn_part=gn_part, b_presplit=ps)


def conv2d_general(x, w2d, bias, out, kh, kw, stride=1, pad_h=0, pad_w=0, relu=False):
    """out[b] = act(W (*) x[b] + bias) for a kh x kw convolution with zero padding (pad_h, pad_w) and stride 1 | 2 -- the InceptionV3
    convolutions of the FID measure (w2d: [M, C*kh*kw] with BatchNorm folded in).  1x1 / stride 1 goes to the plain GEMM."""
    Bn, Cc, H, W, xbs = _img(x)
    M = w2d.shape[0]
    assert w2d.shape[1] == Cc * kh * kw and w2d.is_contiguous()
    OH, OW = (H + 2 * pad_h - kh) // stride + 1, (W + 2 * pad_w - kw) // stride + 1
    Bo, Mo, OHo, OWo, obs = _img(out)
    assert (Bo, Mo, OHo, OWo) == (Bn, M, OH, OW), (out.shape, (Bn, M, OH, OW))
    if kh == 1 and kw == 1 and stride == 1 and pad_h == 0 and pad_w == 0:
        return gemm(w2d, x, out, M=M, N=Bn * OH * OW, K=Cc, b_mode=B_PLAIN, NP=OH * OW, lda=Cc, ldb=H * W, b_bstride=xbs, ldd=OH * OW,
                    d_bstride=obs, bias=bias, act=int(relu))
    return gemm(w2d, x, out, M=M, N=Bn * OH * OW, K=Cc * kh * kw, b_mode=B_CONVG, NP=OH * OW, lda=Cc * kh * kw, b_bstride=xbs, ldd=OH * OW,
                d_bstride=obs, bias=bias, conv=(Cc, H, W, OH, OW), convg=(kh, kw, stride, pad_h, pad_w), act=int(relu))


def pool3(x, out, stride=1, pad=0, mode="max"):
    """3x3 max pooling / average pooling that excludes the zero padding from the divisor (count_include_pad=False)."""
    Bn, Cc, H, W, xbs = _img(x)
    OH, OW = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    Bo, Co, OHo, OWo, obs = _img(out)
    assert (Bo, Co, OHo, OWo) == (Bn, Cc, OH, OW), (out.shape, (Bn, Cc, OH, OW))
    return _timed("pool3_kernel", 4.0 * (x.numel() + out.numel()), "hbm",
                  lambda: L.check(_lib().vd_pool3(_p(x), _p(out), Bn, Cc, H, W, stride, pad, 0 if mode == "max" else 1, xbs, obs, _s()), "vd_pool3"))


def resize_bilinear(x, out, mul=1.0, add=0.0):
    """out = mul * F.interpolate(x, out.shape[-2:], mode="bilinear", align_corners=False) + add  (x, out contiguous NCHW)."""
    assert x.is_contiguous() and out.is_contiguous() and x.shape[:2] == out.shape[:2] and x.dtype == out.dtype == torch.float32
    L.check(_lib().vd_resize_bilinear(_p(x), _p(out), x.shape[0] * x.shape[1], x.shape[2], x.shape[3], out.shape[2], out.shape[3], mul, add, _s()),
            "vd_resize_bilinear")
    return out


def channel_affine(x, mul, add, out):
    """out[b, c] = x[b, c] * mul[c] + add[c]  (contiguous NCHW)."""
    B, C, H, W = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and mul.numel() == C and add.numel() == C
    L.check(_lib().vd_channel_affine(_p(x), _p(mul), _p(add), _p(out), B, C, H * W, _s()), "vd_channel_affine")
    return out


def lpips_layer(f0, f1, w, out, accumulate=False):
    """out[n] (+)= mean_p sum_c w[c] (unit(f0) - unit(f1))^2 for one tap of the LPIPS metric (contiguous [N, C, H, W] feature maps)."""
    N, C, H, W = f0.shape
    assert f0.is_contiguous() and f1.is_contiguous() and f1.shape == f0.shape and w.numel() == C and out.numel() == N
    L.check(_lib().vd_lpips_layer(_p(f0), _p(f1), _p(w), _p(out), N, C, H * W, int(accumulate), _s()), "vd_lpips_layer")
    return out


def attn_core_eligible(heads, head_dim, N) -> bool:
    """Shapes the fused attention core takes (vd_attn_core_fwd / _bwd): 256 tokens, head_dim 32 / 64 / 128 or a multiple of 256."""
    return N == 256 and heads >= 1 and (head_dim in (32, 64, 128) or (head_dim > 0 and head_dim % 256 == 0))


@functools.lru_cache(maxsize=None)
def gemm_bx3_act_eligible(M, K, NP) -> bool:
    """Products of two activation matrices (attention) the split-precision kernel takes (vd_gemm_desc.math = 1).  The callers do not say which
    way A lies, so the question is asked for column-major A, the layout with the stricter rule (M % 4 == 0)."""
    return _gemm_tile(product_query_desc(M, K, NP, a_mode=A_COL, act=True)) == 10


@functools.lru_cache(maxsize=None)
def gemm_bx3_eligible(M, K, NP, nb=None) -> bool:
    """1x1 convolutions / plain products the split-precision GEMM kernels take (vd_gemm_desc.a_packed, shared A); nb = batch items (None: one)."""
    return _gemm_tile(product_query_desc(M, K, NP, nb or 1)) in (9, 11, 13, 19)


def conv1x1(x, w2d, bias, out, residual=None, accumulate=False, tile=0, a_packed=None):
    """1x1 convolution on NCHW = batched GEMM W[M,C] @ x[b][C, HW]."""
    Bn, Cc, H, W, xbs = _img(x)
    M = w2d.shape[0]
    assert w2d.shape[1] == Cc and w2d.is_contiguous()
    Bo, Mo, Ho, Wo, obs = _img(out)
    assert (Bo, Mo, Ho, Wo) == (Bn, M, H, W)
    rbs = _img(residual)[4] if residual is not None else 0
    HW = H * W
    return gemm(w2d, x, out, M=M, N=Bn * HW, K=Cc, b_mode=B_PLAIN, NP=HW, lda=Cc, ldb=HW, b_bstride=xbs, ldd=HW,
                d_bstride=obs, bias=bias, residual=residual, res_bstride=rbs, accumulate=accumulate, tile=tile, a_packed=a_packed)


def linear(x, w, bias, out, accumulate=False):
    """out[b, o] = sum_i x[b, i] w[o, i] + bias[o]   (x: [B, I], w: [O, I])."""
    Bn, I = x.shape
    O = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and out.shape == (Bn, O)
    return gemm(x, w, out, M=Bn, N=O, K=I, a_mode=A_ROW, b_mode=B_KCONTIG, lda=I, ldb=w.stride(0), ldd=O,
                bias=bias, bias_on_n=True, accumulate=accumulate)


def linear_dgrad(dy, w, dx, accumulate=False):
    """dx[b, i] = sum_o dy[b, o] w[o, i]."""
    Bn, O = dy.shape
    I = w.shape[1]
    assert dy.is_contiguous() and dx.is_contiguous()
    S = _long_k_slices(Bn, I, O)
    if S > 1:
        # a long reduction over few output tiles (the time-embedding projections of all ResNet blocks at once: K = 4992, 16 tiles):
        # K slices run as the GEMM's batch dimension into [S][Bn][I] partials, summed in slice order by colsum (deterministic)
        Kc = O // S
        ws = _gemm_ws(S * Bn * I, dx.device)
        gemm(dy, w, ws, M=Bn, N=S * I, K=Kc, NP=I, a_mode=A_ROW, b_mode=B_PLAIN, lda=O, a_bstride=Kc, ldb=w.stride(0),
             b_bstride=Kc * w.stride(0), ldd=I, d_bstride=Bn * I)
        return colsum(ws, dx, S, Bn * I, accumulate=accumulate)
    return gemm(dy, w, dx, M=Bn, N=I, K=O, a_mode=A_ROW, b_mode=B_PLAIN, lda=O, ldb=w.stride(0), ldd=I,
                accumulate=accumulate)


def _long_k_slices(M, N, K) -> int:
    """Number of K slices for a plain product whose tile grid cannot fill the chip by itself (0/1 = do not slice)."""
    if K < 2048 or N % 128 != 0 or ((M + 63) // 64) * (N // 64) >= 128:
        return 1
    for S in range(32, 1, -1):
        if K % S == 0 and (K // S) % 4 == 0 and K // S >= 256:
            return S
    return 1


def linear_wgrad(dy, x, dw, accumulate=False):
    """dw[o, i] (+)= sum_b dy[b, o] x[b, i]."""
    Bn, O = dy.shape
    I = x.shape[1]
    assert dy.is_contiguous() and x.is_contiguous()
    return gemm(dy, x, dw, M=O, N=I, K=Bn, a_mode=A_COL, b_mode=B_PLAIN, lda=O, ldb=I, ldd=dw.stride(0),
                accumulate=accumulate)


def wgrad_desc(dy, x, dw2d, mode, ws=None, accumulate=False, splits=0, tile=0, pad=0, math_mode=0) -> WgradDesc:
    dy, dy_ps = _unwrap(dy)                     # PreSplit operands: vd_wgrad_desc.presplit (bit 0: x, bit 1: dy)
    x, x_ps = _unwrap(x)
    Bn, M, OH, OW, dbs = _img(dy)
    Bx, Cc, H, W, xbs = _img(x)
    assert Bx == Bn
    T = 1 if mode == B_PLAIN else 9
    assert dw2d.shape == (M, Cc * T) and dw2d.is_contiguous()
    d = WgradDesc()
    d.dY, d.X, d.dW, d.ws = _p(dy), _p(x), _p(dw2d), _p(ws)
    d.M, d.C, d.T, d.nb, d.NP = M, Cc, T, Bn, OH * OW
    d.H, d.W, d.OH, d.OW = H, W, OH, OW
    d.mode, d.splits, d.accumulate, d.tile = mode, splits, int(accumulate), tile
    d.dy_bstride, d.x_bstride = dbs, xbs
    d.pad = pad
    d.math = math_mode
    d.presplit = int(x_ps) | (int(dy_ps) << 1)
    return d


WGRAD_ONE = 10000       # class offset of the one-product (math = 3) grouped weight gradients (vd_conv_wgrad_group_class)


def wgrad_group_class(d: WgradDesc) -> int:
    """Kernel class of a split-precision weight gradient for the grouped launch (0: not groupable -> conv_wgrad)."""
    return int(L.load().vd_conv_wgrad_group_class(C.byref(d)))


_WG_CACHE, _WG_WS = {}, {}

# Device job tables (grouped weight gradients, segmented column sums) are built on the host from operand ADDRESSES and uploaded once per
# distinct set.  Inside a HIP-graph capture the activations live at new addresses (the graph's private pool), so new tables appear -- and
# a pageable host -> device copy cannot be captured.  While a capture is open the device tensor is only ALLOCATED (from the graph's pool:
# its address is what the captured launches read) and the copy (+ any one-time fix-up kernel) runs right after the capture ends; the
# graph never writes these tables, so one upload serves every replay.
_CAPTURE_DEFER = None
_CAPTURE_TABLES = None
_CAPTURE_ARENA = None      # [uint8 device buffer, bytes used]


def capture_begin(device, arena_bytes: int = 1 << 20):
    """Open a graph capture for table uploads.  The tables must NOT come from the graph's private memory pool: a block the capture hands to
    a table may have belonged to an activation EARLIER in capture order, and every replay would then overwrite the uploaded table with that
    activation before the launches that read it run.  They are carved out of an arena allocated here, before the capture starts."""
    global _CAPTURE_DEFER, _CAPTURE_TABLES, _CAPTURE_ARENA
    _CAPTURE_DEFER, _CAPTURE_TABLES = [], []
    _CAPTURE_ARENA = [torch.empty(arena_bytes, dtype=torch.uint8, device=device), 0]


def capture_end():
    """Runs the deferred uploads; returns the device tables (and their arena) the captured launches read -- the graph's owner must keep them
    alive (the look-up caches that also hold them are bounded and may drop them)."""
    global _CAPTURE_DEFER, _CAPTURE_TABLES, _CAPTURE_ARENA
    todo, _CAPTURE_DEFER = _CAPTURE_DEFER or [], None
    tables, _CAPTURE_TABLES = _CAPTURE_TABLES or [], None
    arena, _CAPTURE_ARENA = _CAPTURE_ARENA, None
    for fin in todo:
        fin()
    return tables + ([arena[0]] if arena else [])


def upload_table(host: torch.Tensor, device, after=None) -> torch.Tensor:
    """host (CPU tensor) -> device, now or -- during a graph capture -- right after it; `after(dev_tensor)` runs once the data is there."""
    if _CAPTURE_DEFER is None:
        t = host.to(device)
        if after is not None:
            after(t)
        return t
    nbytes = host.numel() * host.element_size()
    arena, used = _CAPTURE_ARENA
    start = (used + 255) // 256 * 256
    if start + nbytes > arena.numel():
        raise L.VillanHipError(f"graph capture: job-table arena exhausted ({start + nbytes} > {arena.numel()} bytes)")
    _CAPTURE_ARENA[1] = start + nbytes
    t = arena[start:start + nbytes].view(host.dtype).view(host.shape)
    _CAPTURE_TABLES.append(t)

    def fin():
        t.copy_(host)
        if after is not None:
            after(t)
    _CAPTURE_DEFER.append(fin)
    return t


def conv_wgrad_group(descs: Sequence[WgradDesc], device):
    """All `descs` (one kernel class, see wgrad_group_class) in ONE compute launch + ONE fixed-order slab reduction.  The device job
    table is planned by the library and uploaded once per distinct set of operand addresses (steady-state training repeats them).
    One-product (math = 3) jobs have classes of their own: a launch never mixes arithmetics (UNet2DModel.wgrad queues per class)."""
    lib = _lib()
    n = len(descs)
    key = tuple((d.dY, d.X, d.dW, d.M, d.C, d.T, d.nb, d.NP, d.H, d.W, d.OH, d.OW, d.mode, d.accumulate, d.dy_bstride, d.x_bstride, d.presplit, d.math)
                for d in descs)
    ent = _WG_CACHE.get(key)
    ws = _WG_WS.get(device)
    if ent is None or ws is None or ent["ws_ptr"] != ws.data_ptr() or ent["ws_floats"] > ws.numel():
        arr = (WgradDesc * n)(*descs)
        jb = int(lib.vd_conv_wgrad_group_job_bytes())
        host = (C.c_uint8 * (n * jb))()
        wsf, blocks, rblocks = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        cls = lib.vd_conv_wgrad_group_plan(arr, n, host, C.byref(wsf), C.byref(blocks), C.byref(rblocks))
        if cls <= 0:
            raise L.VillanHipError(f"vd_conv_wgrad_group_plan: {lib.vd_last_error().decode()}")
        if ws is None or ws.numel() < wsf.value:
            ws = torch.empty(max(int(wsf.value), 1 << 22), device=device, dtype=torch.float32)
            _WG_WS[device] = ws
        ws_ptr = ws.data_ptr()
        table = upload_table(torch.frombuffer(bytearray(host), dtype=torch.uint8), device,
                             after=lambda t: L.check(lib.vd_conv_wgrad_group_rebase(t.data_ptr(), n, ws_ptr, _s()), "vd_conv_wgrad_group_rebase"))
        if len(_WG_CACHE) > 256:
            _WG_CACHE.clear()
        ent = _WG_CACHE[key] = {"table": table, "cls": cls, "blocks": blocks.value, "rblocks": rblocks.value, "ws_ptr": ws.data_ptr(),
                                "ws_floats": int(wsf.value)}
    if _CAPTURE_TABLES is not None:
        _CAPTURE_TABLES.append(ent["table"])              # a cache hit inside a capture: the graph reads this table too
    flops = sum(2.0 * d.M * d.C * d.T * d.nb * d.NP for d in descs)
    nbytes = sum(4.0 * (d.nb * d.M * d.NP + d.nb * d.C * d.H * d.W + d.M * d.C * d.T) for d in descs)
    name = _kernel_name(lib.vd_conv_wgrad_group_kernel_name, ent["cls"]) if _PROF is not None else None
    _timed(name, flops, "mfma", lambda: L.check(
        lib.vd_conv_wgrad_group_launch(ent["table"].data_ptr(), n, ent["cls"], ent["blocks"], ent["rblocks"], _s()), "vd_conv_wgrad_group_launch"),
        nbytes=nbytes)


def conv_wgrad(dy, x, dw2d, mode, ws: Optional[torch.Tensor], accumulate=False, splits=0, tile=0, pad=0, math_mode=0):
    """dw2d[M, C*T] (+)= sum_{b,p} dy[b,m,p] * gather_mode(x)[b, c, p(+)t]."""
    d = wgrad_desc(dy, x, dw2d, mode, ws, accumulate, splits, tile, pad, math_mode)
    Bn, M, OH, OW = dy.shape
    Cc, T = x.shape[1], d.T
    lib = _lib()
    need = lib.vd_conv_wgrad_ws_floats(C.byref(d))
    if need > 0:
        assert ws is not None and ws.numel() >= need, f"wgrad workspace too small: need {need}"
    if _PROF is None:
        L.check(lib.vd_conv_wgrad(C.byref(d), _s()), "vd_conv_wgrad")
        return dw2d
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.check(lib.vd_conv_wgrad(C.byref(d), _s()), "vd_conv_wgrad")
    e1.record()
    name = _kernel_name(lib.vd_conv_wgrad_kernel_name, C.byref(d))
    _PROF.append({"name": name, "flops": 2.0 * M * Cc * T * Bn * OH * OW, "bytes": 4.0 * (dy.numel() + x.numel() + M * Cc * T),
                  "e0": e0, "e1": e1, "kind": "mfma"})
    return dw2d


def _wgrad_s2_split(OW) -> bool:
    """Stride-2 weight gradients on the split-precision kernel (wgrad_bx3 MODE 4).  VILLAN_WGRAD_S2=none: the exact-f32 kernel; wide: only 32x32 outputs and
    wider.  (The first version of the kernel measured neutral -- profiles/r04_wgrad_s2_ab.txt -- because a conditional store pattern kept its loader state in
    scratch memory; fixed, it is 0.28 ms against 0.99 on config #4's two large layers and -0.03 ms per config-#2 step: profiles/r04_wgrad_s2_wide_ab.txt.)"""
    sel = os.environ.get("VILLAN_WGRAD_S2", "all")
    return sel == "all" or (sel != "none" and OW >= 32)


@functools.lru_cache(maxsize=None)
def _wgrad_split_kernel(M, Cc, OH, OW, mode) -> bool:
    return _wgrad_tile(wgrad_query_desc(M, Cc, OH, OW, mode)) == (5 if mode == B_PLAIN else 4)


def wgrad_bx3_eligible(M, Cc, OH, OW, mode) -> bool:
    """Problems the split-precision weight-gradient kernels take (vd_wgrad_desc.math = 1; tile 4 / 5 of vd_conv_wgrad_plan), less the stride-2 ones
    VILLAN_WGRAD_S2 switches off."""
    return _wgrad_split_kernel(M, Cc, OH, OW, mode) and (mode != B_CONV3_S2 or _wgrad_s2_split(OW))


def wgrad_ws_floats(M, Cc, T, nb, NP, OH=None, OW=None, mode=None, math_mode=0) -> int:
    """Workspace floats vd_conv_wgrad needs (square outputs assumed when OH/OW are omitted)."""
    if OH is None:
        OH = OW = int(round(math.sqrt(NP)))
    d = wgrad_query_desc(M, Cc, OH, OW, (B_PLAIN if T == 1 else B_CONV3) if mode is None else mode, nb, math_mode, NP=NP)
    return int(L.load().vd_conv_wgrad_ws_floats(C.byref(d)))


def weight_transpose(w2d, wt, M, Cc, T):
    L.check(_lib().vd_weight_transpose(_p(w2d), _p(wt), M, Cc, T, _s()), "vd_weight_transpose")
    return wt


def sumpool2x2(dU, dX, accumulate=False):
    Bn, Cc, H, W, xbs = _img(dX)
    ubs = _img(dU)[4]
    assert dU.shape == (Bn, Cc, 2 * H, 2 * W)
    L.check(_lib().vd_sumpool2x2(_p(dU), _p(dX), Bn, Cc, H, W, ubs, xbs, int(accumulate), _s()), "vd_sumpool2x2")
    return dX


def conv3x3_s2_dgrad(dy, w2d, dx, pad=0, a_packed=None):
    """Input gradient of the stride-2 (pad (0,1,0,1)) conv: plain GEMM G[b] = w2d^T @ dy[b] (no structural zeros, unlike
    the dilated-gather GEMM), then the col2im gather.  a_packed: the [C*9, M] transpose packed as a one-tap split-precision operand."""
    Bn, M, OH, OW, dbs = _img(dy)
    Bx, Cc, H, W, xbs = _img(dx)
    assert Bx == Bn and w2d.shape == (M, Cc * 9) and w2d.is_contiguous()
    OHW = OH * OW
    G = torch.empty((Bn, Cc * 9, OHW), device=dy.device, dtype=torch.float32)
    gemm(w2d, dy, G, M=Cc * 9, N=Bn * OHW, K=M, a_mode=A_COL, b_mode=B_PLAIN, NP=OHW, lda=Cc * 9, ldb=OHW, b_bstride=dbs,
         ldd=OHW, d_bstride=Cc * 9 * OHW, a_packed=a_packed)
    L.check(_lib().vd_col2im_s2(_p(G), _p(dx), Bn, Cc, H, W, OH, OW, pad, Cc * 9 * OHW, xbs, _s()), "vd_col2im_s2")
    return dx


def rowsum(x, ws, ws_ld=None):
    """ws[b, m] = sum_p x[b, m, :, :]   (ws may be a column slice of a wider [B, ld] matrix)."""
    Bn, M, H, W, xbs = _img(x)
    ld = M if ws_ld is None else ws_ld
    L.check(_lib().vd_rowsum(_p(x), _p(ws), Bn, M, H * W, xbs, ld, _s()), "vd_rowsum")
    return ws


def colsum(ws, out, Bn, Cc, ld=None, accumulate=False):
    L.check(_lib().vd_colsum(_p(ws), _p(out), Bn, Cc, Cc if ld is None else ld, int(accumulate), _s()), "vd_colsum")
    return out


def colsum_segmented(table, n_jobs, Bn):
    """table: device int64 [n_jobs, 4] = (ws address, out address, columns <= 64, ld); out += column sums (one launch)."""
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= 4 * n_jobs
    L.check(_lib().vd_colsum_segmented(_p(table), n_jobs, Bn, _s()), "vd_colsum_segmented")


# --------------------------------------------------------------------------------------------- GroupNorm
def _gn_ws(Bn, Cc, HW, G, device):
    """Scratch for the multi-workgroup GroupNorm of large groups (None when the single-workgroup kernels apply)."""
    need = _lib().vd_groupnorm_ws_floats(Bn, Cc, HW, G)
    return _gemm_ws(need, device) if need > 0 else None


GN_FWD, GN_BWD, GN_STATS = 0, 1, 2


def groupnorm_plan(which, Bn, Cc, HW, G, aligned=True, has_ws=None, stream=None):
    """(kernel names, chunks per group) that groupnorm_fwd / groupnorm_bwd / groupnorm_stats (which = GN_FWD / GN_BWD / GN_STATS) take for
    these dimensions: a host-only query of the library's own dispatch (vd_groupnorm_plan), nothing is launched.  has_ws None: as the
    wrappers call it (a workspace whenever vd_groupnorm_ws_floats asks for one); stream None: no stream (never capturing)."""
    lib = L.load()                      # no device needed
    if has_ws is None:
        has_ws = lib.vd_groupnorm_ws_floats(Bn, Cc, HW, G) > 0
    buf = C.create_string_buffer(128)
    S = lib.vd_groupnorm_plan(which, Bn, Cc, HW, G, int(aligned), int(has_ws), stream, buf, len(buf))
    L.check(min(S, 0), "vd_groupnorm_plan")
    return buf.value.decode(), S


def groupnorm_fwd(x, gamma, beta, y, mean, rstd, G, eps, silu):
    Bn, Cc, H, W, xbs = _img(x)
    ybs = _img(y)[4]
    assert y.shape == x.shape and mean.numel() >= Bn * G and rstd.numel() >= Bn * G
    _timed("groupnorm_fwd (gn_fwd_reg_kernel<*> / gn_chunk_*)", 8.0 * x.numel(), "hbm", lambda: L.check(
        _lib().vd_groupnorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), Bn, Cc, H * W, G, eps,
                                int(silu), xbs, ybs, _p(_gn_ws(Bn, Cc, H * W, G, x.device)), _s()), "vd_groupnorm_fwd"))
    return y


def groupnorm_stats(x, gamma, beta, ss, mean, rstd, G, eps):
    """ss[b, c] = (gamma_c * rstd, beta_c - mean * gamma_c * rstd): the operand of conv3x3(gn_ss=...)."""
    Bn, Cc, H, W, xbs = _img(x)
    assert ss.shape == (Bn, Cc, 2) and ss.is_contiguous()
    L.check(_lib().vd_groupnorm_stats(_p(x), _p(gamma), _p(beta), _p(ss), _p(mean), _p(rstd), Bn, Cc, H * W, G, eps, xbs, _s()),
            "vd_groupnorm_stats")
    return ss


def groupnorm_stats_from_partials(part, tiles, gamma, beta, ss, mean, rstd, HW, G, eps):
    """groupnorm_stats() from the per-tile channel sums a convolution wrote (conv3x3(gn_part=...)): no pass over the tensor."""
    Bn, Cc = ss.shape[0], ss.shape[1]
    assert ss.is_contiguous() and part.is_contiguous() and part.numel() >= Bn * tiles * Cc * 2
    L.check(_lib().vd_groupnorm_stats_from_partials(_p(part), tiles, _p(gamma), _p(beta), _p(ss), _p(mean), _p(rstd), Bn, Cc, HW, G, eps, _s()),
            "vd_groupnorm_stats_from_partials")
    return ss


def gn_fusable(x, cout) -> bool:
    """conv3x3(gn_ss=...) applies: patch-staged kernel with one image per tile and a register-resident statistics pass."""
    Bn, Cc, H, W = x.shape
    return W in (16, 32) and H == W and Cc % 8 == 0 and Cc <= 1024 and cout >= 64


def groupnorm_bwd(dy, x, mean, rstd, gamma, beta, dx, dgamma_ws, dbeta_ws, G, silu, extra=None, extra2=None, rowsum=None, rowsum_ld=None):
    """dx = GN(+SiLU) backward (+ extra + extra2); rowsum (optional, [B, >= C] rows of stride rowsum_ld): sum_p dx[b, c, p], written by the
    same pass (vd_groupnorm_bwd_fused)."""
    Bn, Cc, H, W, xbs = _img(x)
    dbs, dxbs = _img(dy)[4], _img(dx)[4]
    ebs = _img(extra)[4] if extra is not None else 0
    e2bs = _img(extra2)[4] if extra2 is not None else 0
    assert dgamma_ws.numel() >= Bn * Cc and dbeta_ws.numel() >= Bn * Cc
    assert extra2 is None or extra2.shape == x.shape
    rld = 0
    if rowsum is not None:
        rld = Cc if rowsum_ld is None else rowsum_ld
        assert rld >= Cc
    nbytes = (12.0 + (4.0 if extra is not None else 0.0) + (4.0 if extra2 is not None else 0.0)) * x.numel()   # dy, x (+ extras) read once, dx written once
    _timed("groupnorm_bwd (gn_bwd_reg_kernel<*> / gn_chunk_*)", nbytes, "hbm", lambda: L.check(
        _lib().vd_groupnorm_bwd_fused(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(extra), _p(extra2), _p(dx),
                                      _p(dgamma_ws), _p(dbeta_ws), _p(rowsum), Bn, Cc, H * W, G, int(silu), dbs, xbs, ebs, e2bs, dxbs, rld,
                                      _p(_gn_ws(Bn, Cc, H * W, G, x.device)), _s()), "vd_groupnorm_bwd"))
    return dx


# --------------------------------------------------------------------------------------------- attention
def softmax_col_fwd(S, nb, N):
    L.check(_lib().vd_softmax_col_fwd(_p(S), nb, N, _s()), "vd_softmax_col_fwd")
    return S


def softmax_col_bwd(P, dP, nb, N, scale):
    L.check(_lib().vd_softmax_col_bwd(_p(P), _p(dP), nb, N, scale, _s()), "vd_softmax_col_bwd")
    return dP


def attn_core_fwd(qkv, out, P, heads, head_dim, N, scale):
    """Fused attention core (qkv [B, 3C, H, W] contiguous); P = None in the no-grad path, else the [B, heads, N, N] probabilities."""
    Bn = qkv.shape[0]
    assert qkv.is_contiguous() and out.is_contiguous() and (P is None or P.is_contiguous())
    dt = 8 if head_dim % 256 == 0 else head_dim // 32
    _timed(f"attn_core_kernel<{dt}, false>", 4.0 * Bn * heads * N * N * head_dim, "mfma", lambda: L.check(
        _lib().vd_attn_core_fwd(_p(qkv), _p(out), _p(P), Bn, heads, head_dim, N, scale, _s()), "vd_attn_core_fwd"),
        nbytes=4.0 * (qkv.numel() + out.numel() + (P.numel() if P is not None else 0)))
    return out


def attn_core_bwd(qkv, P, out, dout, dS, dqkv, heads, head_dim, N, scale):
    """dS (into `dS`, [B, heads, N, N]) and dq (into dqkv[:, :C]) of the fused attention core; `out` = the saved forward output."""
    Bn = qkv.shape[0]
    assert qkv.is_contiguous() and P.is_contiguous() and dout.is_contiguous() and dS.is_contiguous() and dqkv.is_contiguous() and out.is_contiguous()
    dt = 8 if head_dim % 256 == 0 else head_dim // 32
    _timed(f"attn_core_kernel<{dt}, true>", 4.0 * Bn * heads * N * N * head_dim, "mfma", lambda: L.check(
        _lib().vd_attn_core_bwd(_p(qkv), _p(P), _p(out), _p(dout), _p(dS), _p(dqkv), Bn, heads, head_dim, N, scale, _s()), "vd_attn_core_bwd"),
        nbytes=4.0 * (qkv.numel() * 2 // 3 + 2 * dout.numel() + P.numel() + dS.numel() + qkv.numel() // 3))
    return dqkv


def attn_flash_eligible(heads, head_dim, N) -> bool:
    """Shapes the flash attention takes (vd_attn_flash_fwd / _bwd): heads of 32 channels and a multiple of 256 tokens (at 256 tokens it
    replaces attn_core + the dk / dv products: no probability matrix is saved)."""
    return head_dim == 32 and heads >= 1 and N >= 256 and N % 256 == 0


def attn_flash_fwd(qkv, out, lse, heads, head_dim, N, scale):
    """Attention of qkv [B, 3C, H, W] without the score matrix in HBM; lse [B, heads, N] (None in the no-grad path) for the backward pass."""
    Bn = qkv.shape[0]
    assert qkv.is_contiguous() and out.is_contiguous() and (lse is None or lse.is_contiguous())
    _timed("attn_flash_kernel<0>", 4.0 * Bn * heads * N * N * head_dim, "mfma", lambda: L.check(
        _lib().vd_attn_flash_fwd(_p(qkv), _p(out), _p(lse), Bn, heads, head_dim, N, scale, qkv.stride(0), out.stride(0), _s()), "vd_attn_flash_fwd"),
        nbytes=4.0 * (qkv.numel() + out.numel()))
    return out


def attn_flash_bwd(qkv, out, dout, lse, dqkv, heads, head_dim, N, scale):
    """dq, dk, dv (all of dqkv [B, 3C, H, W]) from the saved forward output and lse; P is recomputed block by block."""
    Bn = qkv.shape[0]
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and lse.is_contiguous() and dqkv.is_contiguous()
    delta = torch.empty_like(lse)
    _timed("attn_flash_kernel<1>+<2>", 10.0 * Bn * heads * N * N * head_dim, "mfma", lambda: L.check(
        _lib().vd_attn_flash_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), Bn, heads, head_dim, N, scale, qkv.stride(0),
                                 out.stride(0), dout.stride(0), dqkv.stride(0), _s()), "vd_attn_flash_bwd"),
        nbytes=4.0 * (2 * qkv.numel() + 2 * dout.numel()))
    return dqkv


def attn_small_fwd(qkv, out, P, Cc, N, scale):
    Bn = qkv.shape[0]
    L.check(_lib().vd_attn_small_fwd(_p(qkv), _p(out), _p(P), Bn, Cc, N, scale, qkv.stride(0), out.stride(0), _s()),
            "vd_attn_small_fwd")
    return out


def attn_small_bwd(qkv, P, dout, dqkv, Cc, N, scale):
    Bn = qkv.shape[0]
    L.check(_lib().vd_attn_small_bwd(_p(qkv), _p(P), _p(dout), _p(dqkv), Bn, Cc, N, scale, qkv.stride(0),
                                     dout.stride(0), dqkv.stride(0), _s()), "vd_attn_small_bwd")
    return dqkv


# --------------------------------------------------------------------------------------------- elementwise
def timestep_embedding(t_f32, freqs, emb, flip):
    Bn, half = t_f32.numel(), freqs.numel()
    assert emb.shape == (Bn, 2 * half) and emb.is_contiguous()
    L.check(_lib().vd_timestep_embedding(_p(t_f32), _p(freqs), _p(emb), Bn, half, int(flip), _s()),
            "vd_timestep_embedding")
    return emb


def silu_fwd(x, y):
    L.check(_lib().vd_silu_fwd(_p(x), _p(y), x.numel(), _s()), "vd_silu_fwd")
    return y


def silu_bwd(dy, x, dx, accumulate=False):
    L.check(_lib().vd_silu_bwd(_p(dy), _p(x), _p(dx), x.numel(), int(accumulate), _s()), "vd_silu_bwd")
    return dx


def add_strided(dst, src, accumulate=True):
    """dst (+)= src for image views with (possibly different) batch strides."""
    Bn, Cc, H, W, dbs = _img(dst)
    sbs = _img(src)[4]
    assert src.shape == dst.shape
    L.check(_lib().vd_add_strided(_p(dst), _p(src), Bn, Cc * H * W, dbs, sbs, int(accumulate), _s()), "vd_add_strided")
    return dst


def add_flat(dst, src, accumulate=True):
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    L.check(_lib().vd_add_strided(_p(dst), _p(src), 1, dst.numel(), dst.numel(), src.numel(), int(accumulate), _s()),
            "vd_add_strided")
    return dst


def scale_(x, alpha: float):
    assert x.is_contiguous()
    L.check(_lib().vd_scale(_p(x), x.numel(), alpha, _s()), "vd_scale")
    return x


def lincomb(out, srcs: Sequence[torch.Tensor], coefs: Sequence[float]):
    n = len(srcs)
    assert 1 <= n <= 6 and len(coefs) == n
    for t in srcs:
        assert t.is_contiguous() and t.numel() == out.numel()
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    cf = (C.c_float * n)(*[float(c) for c in coefs])
    L.check(_lib().vd_lincomb(_p(out), ptrs, cf, n, out.numel(), _s()), "vd_lincomb")
    return out


# --------------------------------------------------------------------------------------------- loss / optimiser
def qsample_backdoor(x0, R, eps, t, tab_a, tab_s, tab_step, tab_coef, x_t, y):
    Bn = x0.shape[0]
    chw = x0.numel() // Bn
    for z in (x0, R, eps, x_t, y):
        assert z.is_contiguous() and z.dtype == torch.float32
    assert t.dtype == torch.int64 and t.is_contiguous()
    L.check(_lib().vd_qsample_backdoor(_p(x0), _p(R), _p(eps), _p(t), _p(tab_a), _p(tab_s), _p(tab_step), _p(tab_coef),
                                       _p(x_t), _p(y), Bn, chw, _s()), "vd_qsample_backdoor")
    return x_t, y


LOSS_KINDS = {"l2": 0, "l1": 1, "huber": 2}


def mse_fwd_bwd(pred, y, dpred, loss, partial, pscale=None, gscale=1.0, kind="l2"):
    """loss = mean(norm(pred * pscale[b] - y)) and its gradient in one pass; kind = the reference's loss_type (loss.py:849-858)."""
    Bn = pred.shape[0]
    chw = pred.numel() // Bn
    assert pred.is_contiguous() and y.is_contiguous() and partial.numel() >= 1024
    L.check(_lib().vd_loss_fwd_bwd(_p(pred), _p(y), _p(pscale), _p(dpred), _p(loss), _p(partial), Bn, chw, gscale,
                                   LOSS_KINDS[kind], _s()), "vd_loss_fwd_bwd")
    return loss


def loss_sample_plan(Bn: int, chw: int):
    """(segments, blocks, workspace floats) vd_loss_sample_fwd_bwd uses for [Bn, chw]: asked of the library on the host, no device needed."""
    seg, blk = C.c_int32(0), C.c_int32(0)
    lib = L.load()
    L.check(lib.vd_loss_sample_plan(int(Bn), int(chw), C.byref(seg), C.byref(blk)), "vd_loss_sample_plan")
    return seg.value, blk.value, int(lib.vd_loss_sample_ws_floats(int(Bn), int(chw)))


def loss_sample_fwd_bwd(pred, y, dpred, loss, ws, *, pscale=None, weight=None, wtab=None, t=None, flags=None, poison_weight=1.0,
                        sample_loss=None, stats=None, gscale=1.0, kind="l2"):
    """The shaped loss (vd_loss_sample_fwd_bwd): loss = mean_b w[b] l[b] with l[b] = mean_i norm(pred[b] * pscale[b] - y[b]) and
    w[b] = weight[b] * wtab[clamp(t[b])] * (poison_weight where flags[b]), absent factors 1; dpred (None: forward only) its gradient times
    gscale; sample_loss [B] the unweighted l[b]; stats [4] = {sum l over clean, n clean, sum l over poisoned, n poisoned}.  flags: bool or
    uint8 [B].  ws: at least loss_sample_plan(B, chw)[2] floats.  Bit-reproducible; all weights 1 gives mse_fwd_bwd's dpred bits."""
    Bn = pred.shape[0]
    chw = pred.numel() // Bn
    assert pred.is_contiguous() and y.is_contiguous() and pred.dtype == y.dtype == torch.float32 and y.numel() == pred.numel()
    assert dpred is None or (dpred.is_contiguous() and dpred.dtype == torch.float32 and dpred.numel() == pred.numel())
    for v in (pscale, weight, sample_loss):
        assert v is None or (v.is_contiguous() and v.dtype == torch.float32 and v.numel() == Bn)
    assert stats is None or (stats.is_contiguous() and stats.dtype == torch.float32 and stats.numel() == 4)
    assert loss.dtype == torch.float32 and loss.numel() >= 1
    Tn = 0
    if wtab is not None:
        assert wtab.is_contiguous() and wtab.dtype == torch.float32 and wtab.numel() > 0
        assert t is not None and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == Bn
        Tn = wtab.numel()
    if flags is not None:
        assert flags.dtype in (torch.bool, torch.uint8) and flags.is_contiguous() and flags.numel() == Bn      # one byte each, nonzero: poisoned
    assert ws.is_contiguous() and ws.dtype == torch.float32 and ws.numel() >= L.load().vd_loss_sample_ws_floats(Bn, chw)
    _timed("loss_sample_fwd_bwd (loss_sample_kernel + loss_sample_finish_kernel)", 4.0 * (2 if dpred is None else 3) * Bn * chw, "hbm", lambda: L.check(
        _lib().vd_loss_sample_fwd_bwd(_p(pred), _p(y), _p(pscale), _p(weight), _p(wtab), _p(t if wtab is not None else None), Tn, _p(flags),
                                      float(poison_weight), _p(dpred), _p(loss), _p(sample_loss), _p(stats), _p(ws), Bn, chw, gscale,
                                      LOSS_KINDS[kind], _s()), "vd_loss_sample_fwd_bwd"))
    return loss


def trigger_inv_objective(e, tau, lam, loss, dout, dtau, partial):
    """loss = || mean_b e[b] - lam * tau ||_2, dout[b] = dloss/de[b] (every b) and dtau = the direct term -lam * r / loss, in one call
    (vd_trigger_inv_objective: fixed-order two-phase sum, bit-reproducible; loss == 0 gives zero gradients)."""
    Bn, Cc, H, W, ebs = _img(e)
    chw = Cc * H * W
    assert tau.is_contiguous() and tau.numel() == chw and dtau.is_contiguous() and dtau.numel() == chw and tau.dtype == dtau.dtype == torch.float32
    assert dout.is_contiguous() and dout.shape == e.shape and dout.dtype == torch.float32 and partial.numel() >= 1024 and loss.numel() >= 1
    _timed("trigger_inv_objective (trigger_inv_residual_kernel + trigger_inv_grad_kernel)", 4.0 * (2 * e.numel() + 3 * chw), "hbm", lambda: L.check(
        _lib().vd_trigger_inv_objective(_p(e), _p(tau), float(lam), _p(loss), _p(dout), _p(dtau), _p(partial), Bn, chw, ebs, _s()),
        "vd_trigger_inv_objective"))
    return loss


def score_inv_objective(s, tau, sigma, lam, loss, dout, dtau, partial):
    """The VE form of trigger_inv_objective, in noise-prediction units n[b] = -sigma * s[b]: loss = || mean_b n[b] - lam * tau ||_2,
    dout[b] = sigma * dloss/ds[b] (every b) and dtau = the direct term -lam * r / loss (vd_score_inv_objective: fixed-order two-phase sum,
    bit-reproducible; loss == 0 gives zero gradients).  s: [B, C, H, W], may have a batch stride of its own."""
    Bn, Cc, H, W, sbs = _img(s)
    chw = Cc * H * W
    assert tau.is_contiguous() and tau.numel() == chw and dtau.is_contiguous() and dtau.numel() == chw and tau.dtype == dtau.dtype == torch.float32
    assert dout.is_contiguous() and dout.shape == s.shape and dout.dtype == torch.float32 and partial.numel() >= 1024 and loss.numel() >= 1
    _timed("score_inv_objective (score_inv_residual_kernel + score_inv_grad_kernel)", 4.0 * (2 * s.numel() + 3 * chw), "hbm", lambda: L.check(
        _lib().vd_score_inv_objective(_p(s), _p(tau), float(sigma), float(lam), _p(loss), _p(dout), _p(dtau), _p(partial), Bn, chw, sbs, _s()),
        "vd_score_inv_objective"))
    return loss


def removal_loss(pred, ref, w_clean, w_shift, dpred, terms, partial, gscale=1.0):
    """terms = {w_clean*clean + w_shift*shift, clean, shift} with clean = mse(pred[:B], ref), shift = mse(pred[B:], ref), and dpred = the
    gradient of gscale * terms[0] with respect to pred, in one call (vd_removal_loss: fixed-order two-phase sum, bit-reproducible).
    pred: [2B, C, H, W], may be a channel slice of a wider buffer; ref: [B, C, H, W] and dpred: [2B, C, H, W], contiguous."""
    B2, Cc, H, W, pbs = _img(pred)
    Bn, chw = B2 // 2, Cc * H * W
    assert B2 == 2 * Bn and Bn >= 1 and tuple(ref.shape) == (Bn, Cc, H, W) and ref.is_contiguous() and ref.dtype == torch.float32
    assert dpred.is_contiguous() and dpred.shape == pred.shape and dpred.dtype == torch.float32 and partial.numel() >= 2048 and terms.numel() >= 3
    _timed("removal_loss (removal_loss_kernel + removal_loss_finish_kernel)", 4.0 * 5 * Bn * chw, "hbm", lambda: L.check(   # pred 2B, ref B read; dpred 2B written
        _lib().vd_removal_loss(_p(pred), _p(ref), float(w_clean), float(w_shift), float(gscale), _p(dpred), _p(terms), _p(partial), Bn, chw, pbs,
                               _s()), "vd_removal_loss"))
    return terms


def image_set_stats(x, mean_img, stats, partial, mul=0.5, add=0.5, lo=0.0, hi=1.0):
    """mean_img = mean over N of y = clamp(x*mul + add, lo, hi) (ops.postprocess's values), stats = {sum_i ||y_i - mean_img||^2, sum_i TV(y_i)}
    (vd_image_set_stats: two passes, fixed-order sums, bit-reproducible).  x: [N, C, H, W], may have a batch stride of its own."""
    N, Cc, H, W, xbs = _img(x)
    assert mean_img.is_contiguous() and tuple(mean_img.shape) == (Cc, H, W) and mean_img.dtype == torch.float32
    assert stats.numel() >= 2 and stats.dtype == torch.float32 and partial.numel() >= 2048
    _timed("image_set_stats (image_set_mean_kernel + image_set_dev_tv_kernel)", 4.0 * (2 * x.numel() + 2 * Cc * H * W), "hbm", lambda: L.check(   # x read by both passes
        _lib().vd_image_set_stats(_p(x), N, Cc, H, W, xbs, float(mul), float(add), float(lo), float(hi), _p(mean_img), _p(stats), _p(partial),
                                  _s()), "vd_image_set_stats"))
    return stats


def image_set_merge(mean_a, stats_a, n_a, mean_b, stats_b, n_b, partial):
    """Merge a chunk's image_set_stats result (mean_b, stats_b; n_b images) into the running one (mean_a, stats_a; n_a images), in place, by the
    pairwise update of Chan et al. (vd_image_set_merge: fixed-order double sum, bit-reproducible).  n_a == 0 copies b into a."""
    chw = mean_a.numel()
    assert mean_a.is_contiguous() and mean_b.is_contiguous() and mean_b.numel() == chw and mean_a.dtype == mean_b.dtype == torch.float32
    assert stats_a.numel() >= 2 and stats_b.numel() >= 2 and stats_a.dtype == stats_b.dtype == torch.float32 and partial.numel() >= 2048
    assert mean_a.data_ptr() != mean_b.data_ptr() and stats_a.data_ptr() != stats_b.data_ptr() and int(n_a) >= 0 and int(n_b) >= 1
    _timed("image_set_merge (image_set_merge_kernel)", 4.0 * 3 * chw, "hbm", lambda: L.check(                  # both means read, mean_a written
        _lib().vd_image_set_merge(_p(mean_a), _p(stats_a), int(n_a), _p(mean_b), _p(stats_b), int(n_b), chw, _p(partial), _s()),
        "vd_image_set_merge"))
    return stats_a


def _neuron_args(tab, flat, *per_neuron):
    """tab: anp.NeuronTable, resident on flat's device.  Every offset of its jobs is checked against the flat buffer here, on the host: the kernels
    trust the table."""
    assert flat.is_contiguous() and flat.dtype == torch.float32 and flat.numel() >= tab.extent, (flat.numel(), tab.extent)
    for v in per_neuron:
        assert v is None or (v.is_contiguous() and v.dtype == torch.float32 and v.numel() == tab.n_neurons), "one f32 per neuron"
    return tab.device_table(flat.device)


def neuron_scale(w0, w, tab, mask, delta=None, xi=None):
    """w[row j] = (mask[j] + delta[j]) * w0[row j] for every row of every job of `tab`, and w[bias j] = (1 + xi[j]) * w0[bias j] where the job
    has a bias (vd_neuron_scale: one launch for the whole table; delta / xi None: mask alone / the bias copied).  A raw-pointer write: whoever
    scales network weights bumps WEIGHTS_EPOCH and calls the network's weights_changed() afterwards (as with `swap`)."""
    table = _neuron_args(tab, w, mask, delta, xi)
    assert w0.is_contiguous() and w0.dtype == torch.float32 and w0.numel() >= tab.extent and w0.data_ptr() != w.data_ptr()
    nbytes = 8.0 * (tab.weight_floats + tab.n_bias) + 4.0 * tab.n_neurons * (1 + (delta is not None) + (xi is not None))
    _timed("neuron_scale (neuron_scale_kernel)", nbytes, "hbm", lambda: L.check(           # w0 read, w written; one mask / delta / xi per row
        _lib().vd_neuron_scale(_p(w0), _p(w), _p(table), tab.n_jobs, tab.total_blocks, _p(mask), _p(delta), _p(xi), _s()), "vd_neuron_scale"))
    return w


def neuron_grad(g, w0, tab, gmask, gxi=None, scale=1.0, accumulate=False):
    """gmask[j] (+)= scale * <g[row j], w0[row j]> and gxi[j] (+)= scale * g[bias j] * w0[bias j] (vd_neuron_grad: one wave per row, fixed
    order, bit-reproducible; a job without a bias leaves its gxi slots alone)."""
    table = _neuron_args(tab, g, gmask, gxi)
    assert w0.is_contiguous() and w0.dtype == torch.float32 and w0.numel() >= tab.extent
    nbytes = 8.0 * (tab.weight_floats + tab.n_bias) + 4.0 * tab.n_neurons * (1 + bool(accumulate)) * (1 + (gxi is not None))
    _timed("neuron_grad (neuron_grad_kernel)", nbytes, "hbm", lambda: L.check(             # g and w0 read; one gmask / gxi per row
        _lib().vd_neuron_grad(_p(g), _p(w0), _p(table), tab.n_jobs, tab.total_blocks, _p(gmask), _p(gxi), float(scale), int(bool(accumulate)), _s()),
        "vd_neuron_grad"))
    return gmask


def neuron_step(x, g, buf=None, *, lr, momentum=0.0, lo, hi, use_sign=False):
    """x = clamp(x - lr * d, lo, hi) in place with d = buf <- momentum * buf + g (buf given), else sign(g) (use_sign) or g (vd_neuron_step, every
    f32 operation rounded on its own; a negative lr ascends)."""
    n = x.numel()
    assert x.is_contiguous() and g.is_contiguous() and x.dtype == g.dtype == torch.float32 and g.numel() == n and float(lo) <= float(hi)
    assert buf is None or (buf.is_contiguous() and buf.dtype == torch.float32 and buf.numel() == n)
    _timed("neuron_step (neuron_step_kernel)", 4.0 * n * (5 if buf is not None else 3), "hbm", lambda: L.check(
        _lib().vd_neuron_step(_p(x), _p(g), _p(buf), n, float(lr), float(momentum), float(lo), float(hi), int(bool(use_sign)), _s()),
        "vd_neuron_step"))
    return x


def _lora_args(tab, flat, *adapter):
    """tab: lora.AdapterTable, resident on flat's device.  Every offset of its jobs is checked against the buffers here, on the host: the kernels
    trust the table."""
    assert flat.is_contiguous() and flat.dtype == torch.float32 and flat.numel() >= tab.extent, (flat.numel(), tab.extent)
    for v in adapter:
        assert v.is_contiguous() and v.dtype == torch.float32 and v.numel() >= tab.numel and v.device == flat.device, "adapter buffer"
    return tab.device_table(flat.device)


def lora_merge(w0, w, tab, ab):
    """w[layer] = w0[layer] + s * B A for every job of `tab` (vd_lora_merge: one launch for the whole table; rank and s are the table's).  A
    raw-pointer write: whoever merges into network weights bumps WEIGHTS_EPOCH and calls the network's weights_changed() afterwards."""
    table = _lora_args(tab, w, ab)
    assert w0.is_contiguous() and w0.dtype == torch.float32 and w0.numel() >= tab.extent and w0.data_ptr() != w.data_ptr()
    _timed("lora_merge (lora_merge_kernel)", 8.0 * tab.weight_floats, "hbm", lambda: L.check(            # w0 read, w written; A, B from cache
        _lib().vd_lora_merge(_p(w0), _p(w), _p(table), tab.n_jobs, tab.row_blocks, _p(ab), tab.r, float(tab.s), _s()), "vd_lora_merge"))
    return w


def lora_grad(g, tab, ab, gab, accumulate=False):
    """gab.B (+)= s * G A^T and gab.A (+)= s * B^T G for every job of `tab`, G the layer's slice of the flat weight gradient `g` (vd_lora_grad:
    one launch, fixed order, bit-reproducible; the padding of gab is left alone)."""
    table = _lora_args(tab, g, ab, gab)
    assert ab.data_ptr() != gab.data_ptr()
    _timed("lora_grad (lora_grad_kernel)", 8.0 * tab.weight_floats, "hbm", lambda: L.check(              # g read twice: rows -> B, columns -> A
        _lib().vd_lora_grad(_p(g), _p(table), tab.n_jobs, tab.row_blocks + tab.col_blocks, _p(ab), _p(gab), tab.r, float(tab.s),
                            int(bool(accumulate)), _s()), "vd_lora_grad"))
    return gab


ACT_TILE, ACT_CHUNK, ACT_COLS = 32, 768, 16      # pixels of a tile, accumulator rows of a table row, int64 of a table row (vd_lora_act_grad)


class ActPlan:
    """An ACTIVATION JOB TABLE of vd_lora_act_grad laid out on the host (`host`, [n_rows, 16] int64), its workspace floats and algorithmic bytes;
    `table(device)` is the device copy, uploaded once (after the capture when one is open)."""

    def __init__(self, rows, r, nbytes):
        self.host = torch.tensor(rows, dtype=torch.int64).view(-1, ACT_COLS).contiguous()
        self.n_rows, self.r, self.nbytes = self.host.shape[0], int(r), float(nbytes)
        self.ws_floats = int(L.load().vd_lora_act_grad_ws_floats(self.host.data_ptr(), self.n_rows, self.r))
        if self.ws_floats < 0:
            raise L.VillanHipError(f"lora_act_plan: the library refuses the table (rank {r}, {self.n_rows} rows)")
        self.workgroups = int(self.host[:, 11].sum())
        self._dev = None

    def table(self, device):
        if self._dev is None:
            self._dev = upload_table(self.host, device)
        elif _CAPTURE_TABLES is not None:
            _CAPTURE_TABLES.append(self._dev)
        return self._dev


def lora_act_plan(jobs, r, workgroups=512) -> ActPlan:
    """jobs: (dy address, dy batch stride, x address, x batch stride, B, M, L, N, offset of A, offset of B) per layer, dy [B, M, N] and x [B, L, N]
    f32 with channel stride N.  A layer of more than 768 accumulator rows (L + M) becomes several table rows.  `workgroups` are shared out in
    proportion to the bytes a table row reads (at least one, at most one per 32-pixel tile), so that one launch fills the chip."""
    rows = []
    for dy, dbs, x, xbs, Bn, M, Ln, N, aoff, boff in jobs:
        for row0 in range(0, Ln + M, ACT_CHUNK):
            rows.append([dy, dbs, x, xbs, Bn, M, Ln, N, aoff, boff, 0, 0, row0, min(ACT_CHUNK, Ln + M - row0), 0, 0])
    if not rows:
        raise ValueError("lora_act_plan: no jobs")
    cost = [float(t[4] * t[7] * (t[5] + t[6])) for t in rows]
    total = sum(cost) or 1.0
    wg = ws = rb = 0
    for t, c in zip(rows, cost):
        tiles = t[4] * ((t[7] + ACT_TILE - 1) // ACT_TILE)
        t[11] = max(1, min(tiles, int(round(workgroups * c / total))))
        t[10], t[14], t[15] = wg, ws, rb
        wg += t[11]
        ws += t[11] * t[13] * r
        rb += (t[13] * r + 255) // 256
    return ActPlan(rows, r, 4.0 * sum(j[4] * j[7] * (j[5] + j[6]) for j in jobs))


def lora_act_grad(plan: ActPlan, ab, gab, s, ws, accumulate=False):
    """gab.A (+)= s (B^T dy) x^T and gab.B (+)= s dy (A x)^T for every job of `plan`, straight from the activations (vd_lora_act_grad: one compute
    launch and one fixed-order reduce launch; bit-reproducible; slots of gab outside the plan's jobs and its padding are left alone)."""
    assert ab.is_contiguous() and gab.is_contiguous() and ws.is_contiguous() and ab.dtype == gab.dtype == ws.dtype == torch.float32
    assert ab.data_ptr() != gab.data_ptr() and ab.device == gab.device == ws.device
    need = int(torch.maximum(plan.host[:, 8] + plan.r * plan.host[:, 6], plan.host[:, 9] + plan.host[:, 5] * plan.r).max())
    assert ab.numel() >= need and gab.numel() >= need, (ab.numel(), gab.numel(), need)
    lib = _lib()
    table = plan.table(ab.device)
    _timed("lora_act_grad (lora_act_grad_kernel+lora_act_reduce_kernel)", plan.nbytes, "hbm", lambda: L.check(
        lib.vd_lora_act_grad(plan.host.data_ptr(), _p(table), plan.n_rows, _p(ab), _p(gab), plan.r, float(s), int(bool(accumulate)), _p(ws),
                             ws.numel(), _s()), "vd_lora_act_grad"))
    return gab


def l2norm_sq(g, partial, out_sq):
    assert g.is_contiguous() and partial.numel() >= 1024
    _timed("l2norm_sq (sumsq_kernel)", 4.0 * g.numel(), "hbm",
           lambda: L.check(_lib().vd_l2norm_sq(_p(g), g.numel(), _p(partial), _p(out_sq), _s()), "vd_l2norm_sq"))
    return out_sq


def adam_step(p, g, m, v, norm_sq, max_norm, inv_scale, lr, beta1, beta2, eps, step, skipped=None, weights=True):
    """weights=False: `p` is no network parameter (an inverted trigger): caches derived from the weights stay valid."""
    global WEIGHTS_EPOCH
    if weights:
        WEIGHTS_EPOCH += 1
    _timed("adam_step (adam_kernel)", 28.0 * p.numel(), "hbm", lambda: L.check(      # p, g, m, v read; p, m, v written
        _lib().vd_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(norm_sq), max_norm, inv_scale, lr, beta1, beta2,
                            eps, step, _p(skipped), _s()), "vd_adam_step"))


def adam_ema_step(p, g, m, v, ema, norm_sq, max_norm, inv_scale, lr, beta1, beta2, eps, step, one_minus_decay, skipped=None, weights=True):
    """adam_step and, in the same launch, ema += (p_new - ema) * one_minus_decay (every operation rounded on its own); a step the kernel skips
    leaves `ema` alone too.  p / m / v get the bits adam_step gives them."""
    global WEIGHTS_EPOCH
    assert ema.is_contiguous() and ema.dtype == torch.float32 and ema.numel() == p.numel()
    if weights:
        WEIGHTS_EPOCH += 1
    _timed("adam_ema_step (adam_ema_kernel)", 36.0 * p.numel(), "hbm", lambda: L.check(      # p, g, m, v, ema read; p, m, v, ema written
        _lib().vd_adam_ema_step(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(norm_sq), max_norm, inv_scale, lr, beta1, beta2,
                                eps, step, one_minus_decay, _p(skipped), _s()), "vd_adam_ema_step"))


def swap(a, b):
    """a <-> b in place, bit for bit (vd_swap).  A raw-pointer write: it bumps neither a tensor's version counter nor WEIGHTS_EPOCH -- whoever swaps
    network weights calls the network's weights_changed() afterwards."""
    assert a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32 and a.numel() == b.numel()
    _timed("swap (swap_kernel)", 16.0 * a.numel(), "hbm", lambda: L.check(                   # both read, both written
        _lib().vd_swap(_p(a), _p(b), a.numel(), _s()), "vd_swap"))


SAM_MODES = {"sam": 0, "asam": 1}


def sam_plan(n: int):
    """(grid, block, floats per thread) of vd_sam_norm_sq's first stage and of vd_sam_perturb for n floats: asked of the library on the host."""
    g, b, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.load().vd_sam_plan(int(n), C.byref(g), C.byref(b), C.byref(f)), "vd_sam_plan")
    return g.value, b.value, f.value


def _sam_flat(*ts):
    n = ts[0].numel()
    for t in ts:
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == n and t.device == ts[0].device), "flat f32 buffers"
    return n


def sam_norm_sq(g, w, partial, out_sq, mode="asam", eta=0.01):
    """out_sq = sum (T g)^2 with T = 1 ("sam"; w may be None) or |w| + eta ("asam") (vd_sam_norm_sq: two stages in a fixed order)."""
    n = _sam_flat(g, w)
    assert partial.numel() >= 1024 and partial.dtype == torch.float32
    m = SAM_MODES[mode]
    _timed("sam_norm_sq (sam_norm_kernel)", 4.0 * n * (1 + m), "hbm", lambda: L.check(                   # g read, and w in "asam"
        _lib().vd_sam_norm_sq(_p(g), _p(w), n, m, float(eta), _p(partial), _p(out_sq), _s()), "vd_sam_norm_sq"))
    return out_sq


def sam_perturb(w, g, backup, norm_sq, rho, mode="sam", eta=0.01):
    """backup = w (bit for bit; None: no copy), then w += a g with c = rho / (sqrt(norm_sq) + 1e-12) and a = c ("sam") or (c T) T with
    T = |w| + eta ("asam") (vd_sam_perturb: one pass; a norm that is 0 or not finite leaves w alone).  A raw-pointer write: whoever perturbs
    network weights bumps WEIGHTS_EPOCH and calls the network's weights_changed() afterwards (as with `swap`)."""
    n = _sam_flat(w, g, backup)
    _timed("sam_perturb (sam_perturb_kernel)", 4.0 * n * (3 + (backup is not None)), "hbm", lambda: L.check(    # w, g read; w, backup written
        _lib().vd_sam_perturb(_p(w), _p(g), _p(backup), n, SAM_MODES[mode], float(eta), float(rho), _p(norm_sq), _s()), "vd_sam_perturb"))
    return w


def sam_neuron_coef(wsq, gsq, tab, coef, norm_sq, rho, eta=0.01):
    """norm_sq = sum_j T_j^2 gsq_j and coef[j] = rho / (sqrt(norm_sq) + 1e-12) * T_j * T_j with T_j = sqrt(wsq_j / len_j) + eta, one value per
    neuron of `tab` (vd_sam_neuron_coef: one workgroup, fixed order; a norm that is 0 or not finite gives coef = 0)."""
    for v in (wsq, gsq, coef):
        assert v.is_contiguous() and v.dtype == torch.float32 and v.numel() == tab.n_neurons and v.device == wsq.device, "one f32 per neuron"
    table = tab.device_table(wsq.device)
    _timed("sam_neuron_coef (sam_neuron_coef_kernel)", 20.0 * tab.n_neurons, "hbm", lambda: L.check(     # wsq, gsq read twice; coef written
        _lib().vd_sam_neuron_coef(_p(wsq), _p(gsq), _p(table), tab.n_jobs, tab.n_neurons, float(rho), float(eta), _p(coef), _p(norm_sq), _s()),
        "vd_sam_neuron_coef"))
    return coef


def neuron_axpy(w, g, tab, coef):
    """w[row j] += coef[j] * g[row j] for every weight row of `tab`; biases and every float outside the table keep their bits (vd_neuron_axpy: one
    launch, vd_neuron_scale's layout).  A raw-pointer write: the caller bumps WEIGHTS_EPOCH and calls weights_changed() (as with `swap`)."""
    table = _neuron_args(tab, w, coef)
    assert g.is_contiguous() and g.dtype == torch.float32 and g.numel() >= tab.extent and g.data_ptr() != w.data_ptr()
    _timed("neuron_axpy (neuron_axpy_kernel)", 12.0 * tab.weight_floats + 4.0 * tab.n_neurons, "hbm", lambda: L.check(   # w, g read; w written
        _lib().vd_neuron_axpy(_p(w), _p(g), _p(table), tab.n_jobs, tab.total_blocks, _p(coef), _s()), "vd_neuron_axpy"))
    return w


def anchor_plan(n: int):
    """(grid, block, floats per thread) of vd_fisher_accum and vd_anchor_grad for n floats: asked of the library on the host."""
    g, b, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.load().vd_anchor_plan(int(n), C.byref(g), C.byref(b), C.byref(f)), "vd_anchor_plan")
    return g.value, b.value, f.value


def fisher_accum(F, g, s: float):
    """F += s * (g * g), every operation rounded on its own (vd_fisher_accum: one pass).  s >= 0: the 1 / K of a mean over K batches."""
    n = _sam_flat(F, g)
    _timed("fisher_accum (fisher_accum_kernel)", 12.0 * n, "hbm", lambda: L.check(                       # F, g read; F written
        _lib().vd_fisher_accum(_p(F), _p(g), n, float(s), _s()), "vd_fisher_accum"))
    return F


def anchor_grad(g, w, w0, F, coef: float, partial=None, pen=None):
    """g += coef * t with d = w - w0 and t = F * d (F None: t = d, L2-SP), and in the same pass pen = sum t * d, the unscaled penalty, in
    vd_sam_norm_sq's fixed order (pen None: no sum; vd_anchor_grad).  w, w0 and F are read only."""
    n = _sam_flat(g, w, w0, F)
    if pen is not None:
        assert partial is not None and partial.numel() >= 1024 and partial.dtype == torch.float32 and pen.dtype == torch.float32
    _timed("anchor_grad (anchor_grad_kernel)", 4.0 * n * (4 + (F is not None)), "hbm", lambda: L.check(  # g, w, w0 (, F) read; g written
        _lib().vd_anchor_grad(_p(g), _p(w), _p(w0), _p(F), n, float(coef), _p(partial if pen is not None else None), _p(pen), _s()),
        "vd_anchor_grad"))
    return g


def curve_plan(n: int):
    """(grid, block, floats per thread) of vd_curve_point and vd_curve_geometry for n floats: asked of the library on the host."""
    g, b, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.load().vd_curve_plan(int(n), C.byref(g), C.byref(b), C.byref(f)), "vd_curve_plan")
    return g.value, b.value, f.value


def curve_point(out, wa, wm, wb, ca: float, cm: float, cb: float, weights=True):
    """out = (ca * wa + cm * wm) + cb * wb, every operation rounded on its own (vd_curve_point: one pass, no temporary).  The inputs may be one
    another; out is none of them.  weights=False: `out` is no network parameter (the bend, a scratch buffer): caches derived from the weights
    stay valid.  Otherwise a raw-pointer write of weights: WEIGHTS_EPOCH is bumped here and the caller calls the network's weights_changed()."""
    global WEIGHTS_EPOCH
    n = _sam_flat(out, wa, wm, wb)
    if weights:
        WEIGHTS_EPOCH += 1
    _timed("curve_point (curve_point_kernel)", 16.0 * n, "hbm", lambda: L.check(                         # wa, wm, wb read; out written
        _lib().vd_curve_point(_p(out), _p(wa), _p(wm), _p(wb), n, float(ca), float(cm), float(cb), _s()), "vd_curve_point"))
    return out


def curve_geometry(wa, wm, wb, partial, out3):
    """out3 = [sum (wm - wa)^2, sum (wm - wb)^2, sum (wa - wb)^2] in vd_sam_norm_sq's fixed order (vd_curve_geometry: one read of the three)."""
    n = _sam_flat(wa, wm, wb)
    assert partial.numel() >= 3 * 1024 and partial.dtype == torch.float32 and out3.numel() >= 3 and out3.dtype == torch.float32
    _timed("curve_geometry (curve_geometry_kernel)", 12.0 * n, "hbm", lambda: L.check(
        _lib().vd_curve_geometry(_p(wa), _p(wm), _p(wb), n, _p(partial), _p(out3), _s()), "vd_curve_geometry"))
    return out3


MERGE_MODES = {"linear": 0, "ties": 1}
MERGE_MAX_TASKS = 8
MERGE_SELECT_PASSES = 4          # vd_merge_select: four passes of 8 bits
MERGE_PARTIAL = 18 * 1024        # uint32 of vd_merge_apply's scratch: (2 K + 2) * 1024 at K = 8


def merge_plan(n: int):
    """(grid, block, floats per thread, scratch bytes of merge_select) of vd_merge_select and vd_merge_apply for n floats: asked of the library
    on the host."""
    g, b, f, w = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    L.check(L.load().vd_merge_plan(int(n), C.byref(g), C.byref(b), C.byref(f), C.byref(w)), "vd_merge_plan")
    return g.value, b.value, f.value, w.value


def merge_select(w, base, k: int, ws, thr_out, rec):
    """thr_out[0] = the k-th largest |w - base| exactly (k = 0: +inf), rec = [keys above it, keys equal to it, non-finite keys] (vd_merge_select:
    radix selection over the float bits, four passes of 8 bits, no read-back).  ws: >= merge_plan(n)[3] bytes (uint8), rec: 3 int64."""
    n = _sam_flat(w, base)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= merge_plan(n)[3], "ws: merge_plan(n)[3] bytes of uint8"
    assert thr_out.dtype == torch.float32 and thr_out.numel() >= 1 and rec.dtype == torch.int64 and rec.numel() >= 3 and rec.is_contiguous()
    passes = MERGE_SELECT_PASSES if k else 1
    _timed("merge_select (merge_hist_kernel)", 8.0 * n * passes, "hbm", lambda: L.check(                 # w, base read once per pass
        _lib().vd_merge_select(_p(w), _p(base), n, int(k), _p(ws), _p(thr_out), _p(rec), _s()), "vd_merge_select"))
    return thr_out


def merge_apply(out, base, tasks: Sequence[torch.Tensor], lam: Optional[Sequence[float]], thr, mode: str, lam_out: float, partial, stats,
                weights=True):
    """The merge of K task checkpoints into `out` in one pass (vd_merge_apply): with t_i = tasks[i] - base trimmed at thr[i], "linear" is
    out = base + sum_i lam[i] t_i (added in ascending i), "ties" out = base + lam_out * (the mean of the t_i that carry the elected sign).
    out may be `base` or one of the tasks.  stats (2 K + 2 int64): kept[K], won[K], support, conflict.  weights=False: `out` is no network
    parameter.  Otherwise a raw-pointer write of weights: WEIGHTS_EPOCH is bumped here and the caller calls the network's weights_changed()."""
    global WEIGHTS_EPOCH
    K = len(tasks)
    n = _sam_flat(out, base, *tasks)
    assert thr.dtype == torch.float32 and thr.numel() >= K and thr.is_contiguous()
    assert partial.dtype == torch.int32 and partial.numel() >= (2 * K + 2) * 1024 and stats.dtype == torch.int64 and stats.numel() >= 2 * K + 2
    ptrs = (C.c_void_p * max(K, 1))(*[t.data_ptr() for t in tasks])
    lams = None if lam is None else (C.c_float * max(K, 1))(*[float(v) for v in lam])
    assert lam is None or len(lam) == K, f"merge_apply: {len(lam)} coefficients for {K} tasks"
    if weights:
        WEIGHTS_EPOCH += 1
    _timed("merge_apply (merge_apply_kernel)", 4.0 * (K + 2) * n, "hbm", lambda: L.check(                # base and K tasks read; out written
        _lib().vd_merge_apply(_p(out), _p(base), ptrs, lams, _p(thr), K, n, MERGE_MODES[mode], float(lam_out), _p(partial), _p(stats), _s()),
        "vd_merge_apply"))
    return out


MERGE_DROP_FLAGS = {"rescale": 1, "copy": 2}
MERGE_DROP_PARTIAL = 26 * 1024   # uint32 of vd_merge_apply_drop's scratch: (3 K + 2) * 1024 at K = 8


def merge_apply_drop(out, base, tasks: Sequence[torch.Tensor], lam: Optional[Sequence[float]], thr, mode: str, lam_out: float,
                     drop_thr: Sequence[int], rescale: Optional[Sequence[float]], streams: Sequence[int], seed: int, partial, stats, copy=False,
                     weights=True):
    """merge_apply with a seeded drop of every task vector (vd_merge_apply_drop): element j of task i is kept where word j & 3 of
    philox4x32_10((lo32(j >> 2), hi32(j >> 2), streams[i], 1), (lo32(seed), hi32(seed))) is >= drop_thr[i] (0 .. 2^32), and the kept entries
    are multiplied by rescale[i] (None: not at all).  copy=True (K = 1, "linear"; lam, thr, rescale and lam_out are not read): out = where(keep,
    tasks[0], base), bits copied.  stats (3 K + 2 int64): drawn[K], kept[K], won[K], support, conflict.  `weights` as in merge_apply."""
    global WEIGHTS_EPOCH
    K = len(tasks)
    n = _sam_flat(out, base, *tasks)
    assert copy or (thr is not None and thr.dtype == torch.float32 and thr.numel() >= K and thr.is_contiguous())
    assert partial.dtype == torch.int32 and partial.numel() >= (3 * K + 2) * 1024 and stats.dtype == torch.int64 and stats.numel() >= 3 * K + 2
    assert len(drop_thr) == K and len(streams) == K, f"merge_apply_drop: {len(drop_thr)} thresholds and {len(streams)} streams for {K} tasks"
    assert lam is None or len(lam) == K, f"merge_apply_drop: {len(lam)} coefficients for {K} tasks"
    assert rescale is None or len(rescale) == K, f"merge_apply_drop: {len(rescale)} rescale factors for {K} tasks"
    ptrs = (C.c_void_p * max(K, 1))(*[t.data_ptr() for t in tasks])
    lams = None if lam is None else (C.c_float * max(K, 1))(*[float(v) for v in lam])
    thrs = (C.c_uint64 * max(K, 1))(*[int(v) for v in drop_thr])
    resc = None if rescale is None else (C.c_float * max(K, 1))(*[float(v) for v in rescale])
    strs = (C.c_uint32 * max(K, 1))(*[int(v) for v in streams])
    flags = (MERGE_DROP_FLAGS["copy"] if copy else 0) | (MERGE_DROP_FLAGS["rescale"] if rescale is not None else 0)
    if weights:
        WEIGHTS_EPOCH += 1
    name = "merge_mix_kernel" if copy else "merge_apply_drop_kernel"
    _timed(f"merge_apply_drop ({name})", 4.0 * (K + 2) * n, "hbm", lambda: L.check(                      # base and K tasks read; out written
        _lib().vd_merge_apply_drop(_p(out), _p(base), ptrs, lams, None if thr is None else _p(thr), thrs, resc, strs, K, n, MERGE_MODES[mode],
                                   float(lam_out), int(seed), flags, _p(partial), _p(stats), _s()), "vd_merge_apply_drop"))
    return out


CHANNEL_ACTS = {"raw": 0, "silu_gn": 1}
CHANNEL_JOB_INTS = 11     # x, mean, rstd, gamma, beta, B, C, HW, G, first channel, first workgroup


def channel_stats_plan(Bn: int, Cc: int, HW: int):
    """(workgroups of a [B, C, HW] job, segments a channel is cut into, longest chain of additions of a sum) of vd_channel_stats: asked of the
    library on the host."""
    wg, seg, chain = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    L.check(L.load().vd_channel_stats_plan(int(Bn), int(Cc), int(HW), C.byref(wg), C.byref(seg), C.byref(chain)), "vd_channel_stats_plan")
    return wg.value, seg.value, chain.value


def channel_stats_table(taps):
    """The host job table of vd_channel_stats ([n_jobs, 11] int64) for taps = [(x [B, C, ...] contiguous f32, mean, rstd, gamma, beta, G,
    first channel)] (the four statistics tensors None: address 0, for act "raw").  -> (table, n_channels written up to)."""
    rows, block, top = [], 0, 0
    for x, mean, rstd, gamma, beta, G, c0 in taps:
        assert x.is_contiguous() and x.dtype == torch.float32 and x.dim() >= 2, "a tapped tensor is contiguous f32 [B, C, ...]"
        Bn, Cc = int(x.shape[0]), int(x.shape[1])
        HW = x.numel() // (Bn * Cc)
        for v, n in ((mean, Bn * G), (rstd, Bn * G), (gamma, Cc), (beta, Cc)):
            assert v is None or (v.is_contiguous() and v.dtype == torch.float32 and v.numel() == n and v.device == x.device), "statistics shape"
        ad = lambda v: 0 if v is None else v.data_ptr()
        rows.append((x.data_ptr(), ad(mean), ad(rstd), ad(gamma), ad(beta), Bn, Cc, HW, int(G), int(c0), block))
        block += channel_stats_plan(Bn, Cc, HW)[0]
        top = max(top, int(c0) + Cc)
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, CHANNEL_JOB_INTS), top


def channel_stats(taps, out, act="silu_gn", keep=None):
    """out[first channel + c] = (sum a, sum a^2) over the batch and the pixels of channel c of every tap, a = x ("raw") or silu(groupnorm(x))
    from the given mean / rstd / gamma / beta ("silu_gn") (vd_channel_stats: one launch for the table, a second one where a channel is long
    enough to be cut; fixed order, bit-reproducible).  out: [n_channels, 2] f32, written where the taps point.  The tapped tensors must stay
    alive until the launch has run; `keep` (a list) receives the table and the workspace, which must live as long."""
    dev = out.device
    assert out.is_contiguous() and out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == 2
    host, top = channel_stats_table(taps)
    assert top <= out.shape[0], (top, tuple(out.shape))
    n_jobs = host.shape[0]
    ws_n = int(L.load().vd_channel_stats_ws_floats(host.data_ptr(), n_jobs))
    if ws_n < 0:
        raise L.VillanHipError(f"vd_channel_stats: {L.last_error()}")
    ws = torch.empty(ws_n, device=dev, dtype=torch.float32) if ws_n else None
    table = upload_table(host, dev)
    if keep is not None:
        keep += [table, ws]
    nbytes = 4.0 * sum(t[0].numel() for t in taps) + 8.0 * top
    _timed("channel_stats (channel_stats_kernel)", nbytes, "hbm", lambda: L.check(          # every x read once; one pair per channel written
        _lib().vd_channel_stats(host.data_ptr(), _p(table), n_jobs, CHANNEL_ACTS[act], _p(out), int(out.shape[0]), _p(ws), ws_n, _s()),
        "vd_channel_stats"))
    return out


def neuron_keep_rows(buf, tab, keep):
    """buf[row j] = +0.0 for every weight row of `tab` with keep[j] == 0, in place; kept rows, biases and every float outside the table keep
    their bits (vd_neuron_keep_rows: one launch, vd_neuron_scale's layout).  On network weights a raw-pointer write: the caller bumps
    WEIGHTS_EPOCH and calls weights_changed() (as with `swap`)."""
    table = _neuron_args(tab, buf, keep)
    assert keep.device == buf.device
    _timed("neuron_keep_rows (neuron_keep_rows_kernel)", 4.0 * tab.n_neurons, "hbm", lambda: L.check(    # the mask read; only dropped rows written
        _lib().vd_neuron_keep_rows(_p(buf), _p(table), tab.n_jobs, tab.total_blocks, _p(keep), _s()), "vd_neuron_keep_rows"))
    return buf


LIPSCHITZ_JOB_INTS = 6    # weight offset, rows, Cin, T, first neuron, first workgroup
LIPSCHITZ_GRAM = 45       # gram slots per neuron: the upper triangle of a 9 x 9 Gram matrix, row by row
LIPSCHITZ_SWEEPS = 8
LIPSCHITZ_EIGEN_BOUND = 5760.5 * 2.0 ** -24     # relative error of lambda_max the header of vd_channel_lipschitz derives


def channel_lipschitz_plan(Cin: int, T: int) -> int:
    """The longest chain of additions of a Gram entry of a [Cin, T] row of vd_channel_lipschitz: asked of the library on the host."""
    chain = C.c_int64(0)
    L.check(L.load().vd_channel_lipschitz_plan(int(Cin), int(T), C.byref(chain)), "vd_channel_lipschitz_plan")
    return chain.value


def channel_lipschitz(w, host_table, out, scale=None, gram=None, table=None):
    """out[first neuron + j] = sigma_max of row j of every job of the Lipschitz table, the row seen as [Cin, T], times |scale[.]| where given
    (vd_channel_lipschitz: one launch for the table, w read once, fixed order, bit-reproducible).  host_table: [n_jobs, 6] int64 on the host,
    {weight offset, rows, Cin, T, first neuron, first workgroup}; table: the same on w's device (uploaded here when None).  gram:
    [n_neurons, 45] f32 or None, the Gram entries of every row.  Every extent is checked here, on the host; the table's rules by the library."""
    assert host_table.dtype == torch.int64 and host_table.dim() == 2 and host_table.shape[1] == LIPSCHITZ_JOB_INTS and host_table.is_contiguous()
    assert host_table.device.type == "cpu" and host_table.shape[0] >= 1
    assert w.is_contiguous() and w.dtype == torch.float32
    jobs = host_table.tolist()
    n = sum(j[1] for j in jobs)
    blocks = sum((j[1] + 3) // 4 for j in jobs)
    assert all(j[0] >= 0 and j[0] + j[1] * j[2] * j[3] <= w.numel() for j in jobs if min(j[1:4]) >= 1), "a job leaves the weight buffer"
    for v, per in ((out, 1), (scale, 1), (gram, LIPSCHITZ_GRAM)):
        assert v is None or (v.is_contiguous() and v.dtype == torch.float32 and v.numel() == per * n and v.device == w.device), "one entry per neuron"
    if table is None:
        table = upload_table(host_table, w.device)
    nbytes = 4.0 * sum(j[1] * j[2] * j[3] for j in jobs) + 4.0 * n * (1 + (scale is not None))
    _timed("channel_lipschitz (channel_lipschitz_kernel)", nbytes, "hbm", lambda: L.check(     # every weight read once; one float per row written
        _lib().vd_channel_lipschitz(_p(w), host_table.data_ptr(), _p(table), len(jobs), blocks, _p(scale), _p(out), _p(gram), _s()),
        "vd_channel_lipschitz"))
    return out


# --------------------------------------------------------------------------------------------- samplers / data
def sched_step(x, eps, out, *, c_eps, c_div, clip, c_x0, c_x, c_e, c_z, z=None, x0_out=None, seed=0, offset=0):
    assert x.is_contiguous() and eps.is_contiguous() and out.is_contiguous()
    L.check(_lib().vd_sched_step(_p(x), _p(eps), _p(z), _p(out), _p(x0_out), x.numel(), c_eps, c_div, clip, c_x0, c_x, c_e,
                                 c_z, seed, offset, _s()), "vd_sched_step")
    return out


def batch_l2norm(x, out):
    """out[b] = ||x[b]||_2 over all non-batch dims."""
    Bn = x.shape[0]
    assert x.is_contiguous() and out.numel() >= Bn
    L.check(_lib().vd_batch_l2norm(_p(x), _p(out), Bn, x.numel() // Bn, _s()), "vd_batch_l2norm")
    return out


def ssim(a, b, win, out, c1, c2):
    """out[n] = mean SSIM map of (a[n], b[n]); win: [K, K] window (vd_ssim)."""
    Bn, Cc, H, W = a.shape
    assert a.is_contiguous() and b.is_contiguous() and win.is_contiguous() and a.shape == b.shape and win.shape[0] == win.shape[1]
    L.check(_lib().vd_ssim(_p(a), _p(b), _p(win), _p(out), Bn, Cc, H, W, win.shape[0], c1, c2, _s()), "vd_ssim")
    return out


def postprocess(x, out, mul, add, lo, hi, to_nhwc):
    Bn, Cc, H, W = x.shape
    assert x.is_contiguous() and out.is_contiguous()
    L.check(_lib().vd_postprocess(_p(x), _p(out), Bn, Cc, H * W, mul, add, lo, hi, int(to_nhwc), _s()), "vd_postprocess")
    return out


def fir_resample2(x, out, up: bool, scale: float = 1.0, accumulate: bool = False):
    """diffusers upsample_2d / downsample_2d ((1,3,3,1) FIR, factor 2) on contiguous [B, C, H, W]; out = scale * f(x) (+ out)."""
    Bn, Cc, H, W = x.shape
    assert x.is_contiguous() and out.is_contiguous()
    assert out.shape == ((Bn, Cc, 2 * H, 2 * W) if up else (Bn, Cc, H // 2, W // 2)), (x.shape, out.shape, up)
    L.check(_lib().vd_fir_resample2(_p(x), _p(out), Bn * Cc, H, W, int(up), scale, int(accumulate), _s()), "vd_fir_resample2")
    return out


def pyramid_dgrad(g, w, out, coarse=None, accumulate: bool = False):
    """out = w^T g (+ fir_resample2(coarse, up=True) / 4) (+ out): the gradient of one level of NCSN++'s input-image pyramid with respect to its
    image (vd_pyramid_dgrad).  g: [B, K, H, W], may be a channel slice of a wider buffer; w: [K, C] with C <= 4; coarse: [B, C, H/2, W/2] or None;
    out: contiguous [B, C, H, W].  Exact f32 in a fixed order: bit-reproducible."""
    Bn, K, H, W, gbs = _img(g)
    Cc = w.shape[1]
    assert w.is_contiguous() and tuple(w.shape) == (K, Cc) and w.dtype == torch.float32 and 1 <= Cc <= 4
    assert out.is_contiguous() and tuple(out.shape) == (Bn, Cc, H, W) and out.dtype == torch.float32
    assert coarse is None or (coarse.is_contiguous() and tuple(coarse.shape) == (Bn, Cc, H // 2, W // 2) and coarse.dtype == torch.float32
                              and H % 2 == 0 and W % 2 == 0)
    _timed("pyramid_dgrad (pyramid_dgrad_kernel)", 4.0 * (g.numel() + (2 + int(accumulate)) * out.numel()), "hbm", lambda: L.check(
        _lib().vd_pyramid_dgrad(_p(g), _p(w), _p(coarse), _p(out), Bn, K, Cc, H, W, gbs, int(accumulate), _s()), "vd_pyramid_dgrad"))
    return out


def fourier_embedding(t_f32, W, emb):
    Bn, half = t_f32.numel(), W.numel()
    assert emb.shape == (Bn, 2 * half) and emb.is_contiguous()
    L.check(_lib().vd_fourier_embedding(_p(t_f32), _p(W), _p(emb), Bn, half, _s()), "vd_fourier_embedding")
    return emb


def rowscale(x, s, out, divide=False):
    Bn = x.shape[0]
    assert x.is_contiguous() and out.is_contiguous() and s.numel() == Bn
    L.check(_lib().vd_rowscale(_p(x), _p(s), _p(out), Bn, x.numel() // Bn, int(divide), _s()), "vd_rowscale")
    return out


def vq_nearest(z, codebook, zq, idx=None):
    """zq[b, :, p] = codebook[argmin_e |z[b, :, p] - e|^2]  (VectorQuantizer forward)."""
    Bn, D, H, W, zbs = _img(z)
    qbs = _img(zq)[4]
    assert zq.shape == z.shape and codebook.is_contiguous() and codebook.shape[1] == D
    assert idx is None or (idx.dtype == torch.int64 and idx.numel() >= Bn * H * W)
    L.check(_lib().vd_vq_nearest(_p(z), _p(codebook), _p(zq), _p(idx), Bn, D, H * W, codebook.shape[0], zbs, qbs, _s()),
            "vd_vq_nearest")
    return zq


def randn(out, seed, offset):
    L.check(_lib().vd_randn(_p(out), out.numel(), seed, offset, _s()), "vd_randn")
    return out


def poison_batch(img_u8, flags_u8, trigger, target, pixel_values, tgt, image_out, vmin, vmax, R_trigger_only=False, idx=None):
    """img_u8: the [N, H, W, C] uint8 dataset (or exactly the batch when idx is None); idx: int64 [B] sample ids."""
    _, H, W, Cc = img_u8.shape
    Bn = flags_u8.numel()
    assert img_u8.dtype == torch.uint8 and flags_u8.dtype == torch.uint8 and img_u8.is_contiguous()
    assert idx is None or (idx.dtype == torch.int64 and idx.numel() == Bn and idx.is_contiguous())
    assert idx is not None or img_u8.shape[0] == Bn
    L.check(_lib().vd_poison_batch(_p(img_u8), _p(idx), _p(flags_u8), _p(trigger), _p(target), _p(pixel_values), _p(tgt),
                                   _p(image_out), Bn, Cc, H, W, vmin, vmax, int(R_trigger_only), _s()), "vd_poison_batch")
    return pixel_values, tgt
