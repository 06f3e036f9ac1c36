"""The persistent / grouped split-precision kernels at the edges of their tile walks, against exact references (tests/exact_ref.py).

Families: conv3_k32p_kernel (vd_gemm_tile 18), conv3_sm_kernel (20), gemm1x1_k32p_kernel (19) and the grouped weight gradients
(wgrad_ps_group_kernel, wgrad_k32_group_kernel, wgrad1x1_wide_group_kernel).  Tile counts are chosen per regime of the walk: idle
slots (193-255 tiles, not a multiple of 8), exactly 256, walks of one and two tiles across image and m-tile boundaries (385-511,
ragged M) and long walks with a remainder (> 1024).  Every case

* runs each arithmetic the dispatcher allows (bf16x3, f16, bf16) and asserts the kernel it reached, by tile / math (or weight-gradient
  class) and by the instantiation name ops records -- the same name test_kernel_census.py derives from these tables;
* reads its operands from channel slices of NaN-filled buffers and writes into outputs / workspaces surrounded by a bit pattern that
  must survive;
* launches twice into fresh NaN outputs: these kernels sum in a fixed order, so the results are bit-identical;
* is held to the exact f64 contraction of the operands the arithmetic multiplies: what remains is the f32 accumulation order.

Gates: each is at most 10x the worst value measured on MI355X for its family and arithmetic (GATES lists both).  f16 subnormal
activations (the "sub" values) are multiplied as such: the hardware does not flush them, and the reference keeps them too.  The
folded GroupNorm loader (mode 3) computes silu(x * scale + shift) with a hardware exp, a few f32 ulps from torch's value; at one
product per term the kernel rounds ITS value to bf16 / f16, so an operand near a rounding midpoint may land on the other neighbour.
Those operands are found (exact_ref.rounding_ambiguity) and their largest possible effect, conv(|w|, distance between the two
neighbours), is allowed per output element on top of the same gate as the other cases.  At bf16x3 the lo part absorbs it."""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_ref as X  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.lib import B_CONV3, B_CONV3_T, B_CONV3_UP, B_PLAIN  # noqa: E402

DEV = X.DEV
# (family, arithmetic): gate  -- measured worst value alongside
GATES = {("k18", "bf16x3"): 1e-5,          # 1.5e-6
         ("k18", "f16"): 5e-6,             # 5.5e-7
         ("k18", "bf16"): 5e-6,            # 5.6e-7
         ("k18_gn_part", "bf16x3"): 1e-6,  # 1.5e-7
         ("k18_gn_part", "bf16"): 1e-6,    # 1.2e-7
         ("k20", "bf16x3"): 5e-6,          # 5.6e-7
         ("k20", "bf16"): 2e-6,            # 2.4e-7
         ("k19", "bf16x3"): 2e-6,          # 2.4e-7
         ("k19", "f16"): 1e-6,             # 1.4e-7
         ("k19", "bf16"): 1e-6,            # 1.4e-7
         ("wgrad", "bf16x3"): 2e-6,        # 2.9e-7
         ("wgrad", "bf16"): 2e-6}          # 2.9e-7
WORST = {}


def b(v):
    return "true" if v else "false"


# ------------------------------------------------------------------------------------------------- instantiation names (pure)
def k18_name(OW, md, arith, ps):
    return f"conv3_k32p_kernel<{16 if OW == 16 else 32}, {md}, true, true, {b(arith == 'f16')}, {b(ps)}, {b(arith == 'bf16')}>"


def k20_name(OW, md, arith):
    return f"conv3_sm_kernel<{OW}, {md}, {2 if OW == 8 else 4}, 1, {b(arith == 'bf16')}>"


def k19_name(M, N, arith):
    big = arith != "f16" and M % 256 == 0 and N % 128 == 0
    return f"gemm1x1_k32p_kernel<{b(arith == 'f16')}, {256 if big else 128}, {b(arith == 'bf16')}>"


def wgrad_name(kind, S, up, arith):
    one = b(arith == "bf16")
    if kind == "wide":
        return f"wgrad1x1_wide_group_kernel<{one}>"
    fam = "wgrad_ps_group_kernel" if kind == "ps" else "wgrad_k32_group_kernel"
    return f"{fam}<{S}, {2 if up else 0}, {one}>"


ARITY = {"conv3_k32p_kernel": 7, "conv3_sm_kernel": 5, "gemm1x1_k32p_kernel": 3, "wgrad_ps_group_kernel": 3, "wgrad_k32_group_kernel": 3,
         "wgrad1x1_wide_group_kernel": 1,
         "wgrad_bx3_group_kernel": 3, "wgrad_bx3_kernel": 3, "wgrad_k32_kernel": 2}        # (WIDE = false by default; cases: test_wgrad_edges_gpu.py)


def normalise(name):
    """An instantiation name as ops records it -> the full template argument list (defaulted arguments are all false), without the
    '@<width>' and '(+group_reduce)' / '(+slab_reduce)' suffixes."""
    name = name.replace("(+group_reduce)", "").replace("(+slab_reduce)", "").split("@")[0].strip()
    fam, _, args = name.partition("<")
    args = [a.strip() for a in args.rstrip(">").split(",") if a.strip()]
    return f"{fam}<{', '.join(args + ['false'] * (ARITY[fam] - len(args)))}>"


# ------------------------------------------------------------------------------------------------------------- case tables
# conv3_k32p (tile 18): id, B, Cin, Cout, OH, OW, mode, options, values.  16x16 outputs: tiles = ceil(Cout / 128) * B; 32-wide tiles are
# 8 rows x 32 columns.  Modes: fwd (0), t (1, flipped taps), up (2, nearest 2x), gn (3, folded GroupNorm + SiLU).
K18 = [
    ("s16_idle", 203, 32, 128, 16, 16, "fwd", "bias rowadd res gnpart", "std"),          # 203 tiles: idle slots, r8 = 3
    ("s16_256", 256, 64, 128, 16, 16, "t", "res acc", "std"),                          # exactly 256
    ("s16_walk2", 229, 32, 160, 16, 16, "up", "bias res", "std"),                      # tiles_m = 2, ragged M: 458 tiles, walks of 1 and 2
    ("s16_long", 1031, 32, 128, 16, 16, "gn", "bias rowadd gnpart", "std"),            # 1031 tiles: walks of 4 and 5
    ("s16_deep", 200, 256, 96, 16, 16, "fwd", "acc", "std"),                           # 8 K-stages, ragged M
    ("s16_pool2", 200, 64, 96, 16, 16, "t", "pool2", "std"),                           # 2x2 block sums in the epilogue
    ("s16_wide", 203, 32, 128, 16, 16, "fwd", "bias res", "wide"),                     # |x| from 1e-4 to 1e4
    ("s16_sub", 203, 32, 128, 16, 16, "fwd", "", "sub"),                               # f16 subnormal activations
    ("s32_idle", 53, 32, 128, 32, 32, "fwd", "bias res gnpart", "std"),                # 212 tiles
    ("w64_256", 16, 32, 128, 64, 64, "t", "acc rowadd", "std"),                        # 64-wide images: 16 tiles each, 256 in all
    ("s32_walk", 33, 32, 320, 32, 32, "up", "bias res", "std"),                        # tiles_m = 3, ragged M: 396 tiles
    ("s32_long", 263, 32, 128, 32, 32, "gn", "bias rowadd res", "std"),                # 1052 tiles
    ("w64_up", 13, 32, 64, 64, 64, "up", "bias acc gnpart", "std"),                    # 208 tiles, M = 64
    ("w64x32", 25, 64, 128, 32, 64, "fwd", "res gnpart", "std"),                        # 32 x 64 images: 200 tiles
]
MODES = {"fwd": (B_CONV3, 0), "t": (B_CONV3_T, 1), "up": (B_CONV3_UP, 2), "gn": (B_CONV3, 3)}


def _ariths(vals, allowed):
    return {"std": allowed, "wide": ("bf16x3",), "sub": ("f16",)}[vals]


def k18_cases():
    out = []
    for row in K18:
        rid, _, _, _, _, _, mode, _, vals = row
        for ps in ((False, True) if mode != "gn" else (False,)):
            if ps and vals != "std":
                continue
            for arith in _ariths(vals, ("bf16x3", "bf16") if ps else ("bf16x3", "f16", "bf16")):
                out.append(pytest.param(row, arith, ps, id=f"{rid}-{arith}{'-ps' if ps else ''}"))
    return out


def k18_expected(row, arith, ps):
    return k18_name(row[5], MODES[row[6]][1], arith, ps)


# conv3_sm (tile 20): id, B, Cin, Cout, side, mode, options.  tiles = ceil(Cout / 64) * ceil(B / images per tile)
K20 = [
    ("s8_ragged", 45, 64, 160, 8, "fwd", "bias rowadd res"),       # 3 x 23 = 69 tiles (grid % 8 != 0), ragged M, last group one image
    ("s8_even", 64, 96, 128, 8, "t", "acc"),                        # 2 x 32 = 64 tiles (grid % 8 == 0)
    ("s4_even", 255, 64, 256, 4, "fwd", "bias res"),                # 4 x 64 = 256 tiles, last group three images
    ("s4_ragged", 343, 64, 160, 4, "t", "acc rowadd"),              # 3 x 86 = 258 tiles, ragged M
]


def k20_cases():
    return [pytest.param(row, arith, id=f"{row[0]}-{arith}") for row in K20 for arith in ("bf16x3", "bf16")]


def k20_expected(row, arith):
    return k20_name(row[4], MODES[row[5]][1], arith)


# gemm1x1_k32p (tile 19): id, B, Cin, Cout, side, options, values.  tiles = ceil(Cout / 128) * B * side^2 / 256
K19 = [
    ("m128_idle", 412, 64, 192, 8, "bias res", "std"),             # 2 x 103 = 206 tiles of 4 images each, ragged M
    ("m256_walk", 1000, 128, 256, 8, "acc res", "std"),            # 256-row tiles (500 of them) at bf16x3 / bf16
    ("m128_long", 1029, 64, 128, 16, "res", "std"),                 # 1029 tiles
    ("m128_wide", 412, 64, 192, 8, "res", "wide"),
]


def k19_cases():
    return [pytest.param(row, arith, id=f"{row[0]}-{arith}") for row in K19 for arith in _ariths(row[6], ("bf16x3", "f16", "bf16"))]


def k19_expected(row, arith):
    return k19_name(row[3], row[1] * row[4] * row[4], arith)


# grouped weight gradients: id, kind (ps | k32 | wide), output side, upsample-fused, jobs [(B, Cin, Cout)], values.  Two jobs of
# different sizes per launch (uneven block split), ragged M and C; dW accumulates onto non-zero values.
WG = [
    ("ps32", "ps", 32, False, [(6, 72, 96), (10, 64, 136)], "std"),
    ("ps32up", "ps", 32, True, [(6, 80, 96), (4, 64, 64)], "std"),
    ("ps16", "ps", 16, False, [(24, 72, 96), (40, 64, 136)], "std"),
    ("ps16up", "ps", 16, True, [(24, 80, 96), (16, 64, 64)], "std"),
    ("ps8", "ps", 8, False, [(96, 72, 96), (160, 64, 136)], "std"),
    ("ps8up", "ps", 8, True, [(96, 80, 96), (64, 64, 64)], "std"),
    ("k32_32", "k32", 32, False, [(6, 72, 96), (10, 64, 136)], "std"),
    ("k32_32up", "k32", 32, True, [(6, 80, 96), (4, 64, 64)], "std"),
    ("k32_16", "k32", 16, False, [(24, 72, 96), (40, 64, 136)], "std"),
    ("k32_16up", "k32", 16, True, [(24, 80, 96), (16, 64, 64)], "std"),
    ("k32_8", "k32", 8, False, [(96, 72, 96), (160, 64, 136)], "std"),
    ("k32_8up", "k32", 8, True, [(96, 80, 96), (64, 64, 64)], "std"),
    ("k32_16wide", "k32", 16, False, [(24, 72, 96)], "wide"),
    ("wide1x1", "wide", 16, False, [(40, 200, 96), (24, 64, 328)], "std"),
    ("wide1x1_8", "wide", 8, False, [(100, 72, 264)], "std"),
]


def wg_cases():
    return [pytest.param(row, arith, id=f"{row[0]}-{arith}") for row in WG for arith in _ariths(row[5], ("bf16x3", "bf16"))]


def wg_expected(row, arith):
    return wgrad_name(row[1], row[2], row[3], arith)


def wg_class(row, arith):
    kind, S, up = row[1], row[2], row[3]
    base = 1000 if kind == "wide" else (3000 if kind == "ps" else 0) + 4 * S + (2 if up else 0)
    return base + (ops.WGRAD_ONE if arith == "bf16" else 0)


def all_expected_names():
    """Every instantiation the cases of this module reach (test_kernel_census.py compares them with the library)."""
    names = set()
    for p in k18_cases():
        names.add(k18_expected(*p.values))
    for p in k20_cases():
        names.add(k20_expected(*p.values))
    for p in k19_cases():
        names.add(k19_expected(*p.values))
    for p in wg_cases():
        names.add(wg_expected(*p.values))
    return names


# ------------------------------------------------------------------------------------------------------------------ helpers
def seed_of(rid):
    return zlib.crc32(rid.encode()) % 1000


def gen(seed):
    return torch.Generator().manual_seed(seed)


def values(shape, vals, seed):
    t = torch.randn(*shape, generator=gen(seed))
    if vals == "wide":                                  # magnitudes spread over 1e-4 .. 1e4
        t = t * torch.pow(10.0, torch.rand(*shape, generator=gen(seed + 1)) * 8 - 4)
    elif vals == "sub":                                 # mostly below the smallest normal f16 (6.1e-5)
        t = t * 2e-5
    return t.to(DEV)


def check(family, arith, err, what):
    """Record err for the family's report and hold it to the gate."""
    key = (family, arith)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"[edge] {family} {arith} {what}: {err:.2e} (gate {GATES[key]:.0e})")
    assert err <= GATES[key], (family, arith, what, err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[edge] worst error per family and arithmetic against the exact reference:")
    for (fam, arith), v in sorted(WORST.items()):
        print(f"[edge]   {fam:12s} {arith:7s} {v:.2e}   gate {GATES[(fam, arith)]:.0e}")


@pytest.fixture
def no_gemm_ws(monkeypatch):
    """vd_gemm's split-K workspace, allocated at exactly the planner's size plus a guarded tail (these kernels must ask for none)."""
    asked = []

    def ws(n, device):
        g = X.GuardedFlat(int(n))
        asked.append(g)
        return g.view
    monkeypatch.setattr(ops, "_gemm_ws", ws)
    return asked


def packed_operand(w2d, M, Cc, arith, transposed=False, taps=9):
    pk, pbuf, n = X.packed_guarded(w2d, M, Cc, transposed=transposed, taps=taps)
    keep = [pbuf]
    if arith == "bf16x3":
        return pk, keep
    if arith == "bf16":
        return (pk, pk, 3), keep
    pk16, p16buf, _ = X.packed_guarded(w2d, M, Cc, transposed=transposed, taps=taps, f16=True)
    keep.append(p16buf)
    return (pk, pk16), keep


MATH = {"bf16x3": 0, "f16": 2, "bf16": 3}


def launch_twice(call, outs, init, name_expected, tile, arith):
    """Launch into fresh NaN (or `init`) outputs twice; the first under ops.profile_start() -> the recorded name.  Returns the results."""
    res = []
    for k in range(2):
        for o, i in zip(outs, init):
            o.fresh(i)
        if k == 0:
            ops.profile_start()
        call()
        if k == 0:
            rec = ops.profile_stop()
            assert ops.LAST_GEMM_TILE == tile and ops.LAST_GEMM_MATH == MATH[arith], (ops.LAST_GEMM_TILE, ops.LAST_GEMM_MATH)
            names = [r["name"] for r in rec if r["kind"] == "mfma"]
            assert len(names) == 1 and normalise(names[0]) == name_expected, (names, name_expected)
        torch.cuda.synchronize()
        res.append([o.view.clone() for o in outs])
        assert all(o.intact() for o in outs), "a write landed outside the output"
    for a, c in zip(*res):
        assert torch.equal(a, c), "two launches of a fixed-order kernel differ"
    return res[0]


# --------------------------------------------------------------------------------------------------------- the 3x3 kernels
def _conv_case(B, Cin, Cout, OH, OW, mode, opts, vals, arith, ps, seed):
    bmode, md = MODES[mode]
    up = bmode == B_CONV3_UP
    H, W = (OH // 2, OW // 2) if up else (OH, OW)
    opts = opts.split()
    x = values((B, Cin, H, W), vals, seed)
    if bmode == B_CONV3_T:                                            # forward weights [Cin, Cout]: the input gradient of Cout -> Cin
        w = torch.randn(Cin, Cout, 3, 3, generator=gen(seed + 2)).to(DEV) / math.sqrt(Cout * 9)
    else:
        w = torch.randn(Cout, Cin, 3, 3, generator=gen(seed + 2)).to(DEV) / math.sqrt(Cin * 9)
    w2d = w.reshape(w.shape[0], -1).contiguous()
    pk, keep = packed_operand(w2d, Cout, Cin, arith, transposed=bmode == B_CONV3_T)
    pool2 = "pool2" in opts
    OHo, OWo = (OH // 2, OW // 2) if pool2 else (OH, OW)
    bias = X.nan_vector(torch.randn(Cout, generator=gen(seed + 3)))[0] if "bias" in opts else None
    rowadd, rbs = X.nan_vector(torch.randn(B, Cout, generator=gen(seed + 4))) if "rowadd" in opts else (None, 0)
    res = X.nan_slice(torch.randn(B, Cout, OHo, OWo, generator=gen(seed + 5)).to(DEV), pre=16, post=8) if "res" in opts else None
    acc = torch.randn(B, Cout, OHo, OWo, generator=gen(seed + 6)).to(DEV) if "acc" in opts else None
    gn_ss, a_op, bound = None, x, None
    if mode == "gn":
        gamma, beta = (torch.rand(Cin, generator=gen(seed + 7)) + 0.5).to(DEV), (torch.randn(Cin, generator=gen(seed + 8)) * 0.3).to(DEV)
        gn_ss = torch.empty(B, Cin, 2, device=DEV)
        mean, rstd = torch.empty(B * 32, device=DEV), torch.empty(B * 32, device=DEV)
        ops.groupnorm_stats(x, gamma, beta, gn_ss, mean, rstd, 32, 1e-6)
        z, a_op = X.gn_silu_operand(x, gn_ss)                         # the loader's operand, in f32
        amb = X.rounding_ambiguity(a_op, z, arith)
        if arith != "bf16x3":                                         # the operands that may round the other way, at most this much
            bound = X.conv_f64(amb, X.operands(w, arith)[0].abs(), B_CONV3)
            print(f"[edge] {int((amb > 0).sum())} of {amb.numel()} operands within the window of a rounding midpoint")
            if arith == "bf16":                                       # no blanket allowance: truncating the operand instead of rounding it fails
                wr = X.operands(w, arith)[0]
                at = (a_op.view(torch.int32) & -65536).view(torch.float32)
                off = X.rel_bounded(X.conv_f64(at, wr, B_CONV3), X.conv_f64(X.operands(a_op, arith)[0], wr, B_CONV3), bound)
                assert off > 10 * GATES[("k18", arith)], off
    xin = X.nan_presplit(x) if ps else X.nan_slice(x)
    out = X.GuardedOut(B, Cout, OHo, OWo)
    TW = 16 if OW == 16 else 32
    gp = X.GuardedFlat(B * (OH * OW // 256) * Cout * 2) if "gnpart" in opts and arith != "f16" else None
    outs = [out] + ([gp] if gp is not None else [])
    gp_view = gp.view if gp is not None else None
    w_unused = torch.full((Cout, Cin * 9), float("nan"), device=DEV)     # the f32 weights: shape checks only, a_packed is what runs

    def call():
        ops.conv3x3(xin, w_unused, bias, out.view, mode=bmode, rowadd=rowadd, rowadd_bstride=rbs, residual=res,
                    accumulate=acc is not None, gn_ss=gn_ss, a_packed=pk, pool2=pool2, gn_part=gp_view)
    ref = X.conv3_f64(a_op, w, bmode, arith, bias=bias, rowadd=rowadd, residual=res, acc=acc, pool2=pool2)
    return call, out, gp, ref, acc, keep, TW, bound


class _FlatOut:
    """GuardedFlat with the GuardedOut interface (fresh / view / intact)."""

    def __init__(self, g):
        self.g, self.view = g, g.view

    def fresh(self, init=None):
        self.g.arm()
        return self.view

    def intact(self):
        return self.g.intact()


@pytest.mark.parametrize("row,arith,ps", k18_cases())
def test_conv3_k32p_edges(row, arith, ps, no_gemm_ws):
    rid, B, Cin, Cout, OH, OW, mode, opts, vals = row
    call, out, gp, ref, acc, keep, TW, bound = _conv_case(B, Cin, Cout, OH, OW, mode, opts, vals, arith, ps, seed=seed_of(rid))
    outs, init = [out], [acc]
    if gp is not None:
        outs.append(_FlatOut(gp))
        init.append(None)
    got = launch_twice(call, outs, init, k18_expected(row, arith, ps), 18, arith)
    assert not no_gemm_ws, "the persistent kernel asked for a split-K workspace"
    e = X.rel(got[0], ref) if bound is None else X.rel_bounded(got[0], ref, bound)
    check("k18", arith, e, f"{rid}{' ps' if ps else ''}")
    if gp is not None:
        assert ops.GN_PART_WRITTEN
        part = got[1].view(B, OH * OW // 256, Cout, 2)
        check("k18_gn_part", arith, X.rel(part, X.gn_part_f64(got[0], TW)), rid)


@pytest.mark.parametrize("row,arith", k20_cases())
def test_conv3_sm_edges(row, arith, no_gemm_ws):
    rid, B, Cin, Cout, S, mode, opts = row
    call, out, gp, ref, acc, keep, _, _ = _conv_case(B, Cin, Cout, S, S, mode, opts, "std", arith, False, seed=seed_of(rid))
    got = launch_twice(call, [out], [acc], k20_expected(row, arith), 20, arith)
    assert not no_gemm_ws
    check("k20", arith, X.rel(got[0], ref), rid)


# --------------------------------------------------------------------------------------------------------- the 1x1 kernel
@pytest.mark.parametrize("row,arith", k19_cases())
def test_gemm1x1_k32p_edges(row, arith, no_gemm_ws):
    rid, B, Cin, Cout, S, opts, vals = row
    opts = opts.split()
    seed = seed_of(rid)
    x = values((B, Cin, S, S), vals, seed)
    w = torch.randn(Cout, Cin, generator=gen(seed + 2)).to(DEV) / math.sqrt(Cin)
    pk, keep = packed_operand(w, Cout, Cin, arith, taps=1)
    bias = X.nan_vector(torch.randn(Cout, generator=gen(seed + 3)))[0] if "bias" in opts else None
    res = X.nan_slice(torch.randn(B, Cout, S, S, generator=gen(seed + 5)).to(DEV), pre=16, post=8) if "res" in opts else None
    acc = torch.randn(B, Cout, S, S, generator=gen(seed + 6)).to(DEV) if "acc" in opts else None
    xin = X.nan_slice(x)
    out = X.GuardedOut(B, Cout, S, S)

    def call():
        ops.conv1x1(xin, w, bias, out.view, residual=res, accumulate=acc is not None, a_packed=pk)
    got = launch_twice(call, [out], [acc], k19_expected(row, arith), 19, arith)
    assert not no_gemm_ws
    check("k19", arith, X.rel(got[0], X.gemm1x1_f64(x, w, arith, bias=bias, residual=res, acc=acc)), rid)


# --------------------------------------------------------------------------------------------------- grouped weight gradients
@pytest.mark.parametrize("row,arith", wg_cases())
def test_grouped_wgrad_edges(row, arith, monkeypatch):
    rid, kind, S, up, jobs, vals = row
    seed = seed_of(rid)
    mode = B_PLAIN if kind == "wide" else (B_CONV3_UP if up else B_CONV3)
    T = 1 if kind == "wide" else 9
    H = S // 2 if up else S
    math_mode = 3 if arith == "bf16" else 1
    descs, keep, refs, outs, inits = [], [], [], [], []
    for k, (B, Cin, Cout) in enumerate(jobs):
        x = values((B, Cin, H, H), vals, seed + 10 * k)
        dy = values((B, Cout, S, S), "std", seed + 10 * k + 3)
        dw0 = torch.randn(Cout, Cin * T, generator=gen(seed + 10 * k + 5)).to(DEV)
        o = X.GuardedFlat(Cout * Cin * T)
        dw = o.view.view(Cout, Cin * T)
        xo, dyo = (X.nan_presplit(x), X.nan_presplit(dy)) if kind == "ps" else (X.nan_slice(x), X.nan_slice(dy, pre=16, post=8))
        d = ops.wgrad_desc(dyo, xo, dw, mode, None, accumulate=True, math_mode=math_mode)
        assert ops.wgrad_group_class(d) == wg_class(row, arith), (ops.wgrad_group_class(d), wg_class(row, arith))
        descs.append(d)
        keep.append((xo, dyo))
        refs.append(X.wgrad_arith_f64(dy, x, mode, arith, taps=T, acc=dw0))
        outs.append(_FlatOut(o))
        inits.append(dw0)
    wsf, blocks = X.wgrad_group_ws_floats(descs)
    ws = X.GuardedFlat(wsf)
    monkeypatch.setitem(ops._WG_WS, torch.device(DEV), ws.view)
    res = []
    for rep in range(2):
        for o, i in zip(outs, inits):
            o.g.arm()
            o.view.copy_(i.flatten())
        ws.arm()
        if rep == 0:
            ops.profile_start()
        ops.conv_wgrad_group(descs, torch.device(DEV))
        if rep == 0:
            names = [r["name"] for r in ops.profile_stop()]
            assert len(names) == 1 and normalise(names[0]) == wg_expected(row, arith), names
        torch.cuda.synchronize()
        assert ws.intact(), "the grouped weight gradient wrote past its planned workspace"
        assert all(o.intact() for o in outs), "a write landed outside dW"
        res.append([o.view.clone() for o in outs])
    for k, (a, c) in enumerate(zip(*res)):
        assert torch.equal(a, c), "two launches of a fixed-order kernel differ"
        check("wgrad", arith, X.rel(a.view_as(refs[k]), refs[k]), f"{rid} job {k}")


# ------------------------------------------------------------------------------------------------------------- the format
def test_split_bf16_gives_the_presplit_bits_and_the_packed_weight_values():
    """split_bf16 against the pre-split image bit for bit (the format defines the layout), and against the packed weights as a
    MULTISET of bf16 values: every hi and lo part and the zero padding rows are there.  How the packer pairs and places them (its
    fragment order) is not defined outside the kernels; the kernel cases above check it through their results."""
    x = torch.randn(3, 16, 8, 8, generator=gen(1)) * torch.pow(10.0, torch.rand(3, 16, 8, 8, generator=gen(2)) * 8 - 4)
    hi, lo = X.split_bf16(x)
    ps = X.nan_presplit(x.to(DEV))
    raw = ps.t.contiguous().view(torch.int16).view(3, 2, 64, 2, 8).cpu()            # [B, octet, pixel, part, 8]
    want = torch.stack([t.view(torch.int16).view(3, 2, 8, 64).permute(0, 1, 3, 2) for t in (hi, lo)], dim=3)
    assert torch.equal(raw, want)
    M, Cc = 72, 32
    w = torch.randn(M, Cc * 9, generator=gen(3)).to(DEV)
    pk, _, n = X.packed_guarded(w, M, Cc)
    got = pk.view(torch.int16).cpu().sort().values
    hw, lw = X.split_bf16(w.cpu())
    pad = torch.zeros(((M + 127) // 128 * 128 - M) * Cc * 9 * 2, dtype=torch.int16)
    want = torch.cat([hw.view(torch.int16).flatten(), lw.view(torch.int16).flatten(), pad]).sort().values
    assert torch.equal(got, want)
