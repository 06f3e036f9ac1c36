"""The remaining split-precision (bf16x3) weight-gradient kernels against the exact reference (tests/exact_ref.py), at the edges of their
tile walks -- the conventions of test_persistent_edges_gpu.py:

* grouped: wgrad_bx3_group_kernel, all 7 instantiations (4x4 outputs; stride 2 at 8 / 16 / 32-pixel outputs and 32-pixel segments of wider
  ones, both paddings; stride-1 and upsample-fused wide images), two jobs of unequal size per launch, + wgrad_group_reduce_kernel in its
  unrolled, tail and scalar (M * C * 9 odd) forms;
* single launch (ops.conv_wgrad at math_mode = 1): wgrad_bx3_kernel (the same 7), wgrad_k32_kernel (6), wgrad1x1_bx3_kernel, each unsplit
  (the kernel adds into dW itself) and at the planner's own split count (slabs + slab_reduce_perm / slab_reduce / slab_reduce_scalar).

Every case asserts the kernel class or tile and the instantiation name ops records (test_kernel_census.py derives the same names from these
tables), reads x and dy from channel slices of NaN-filled buffers, accumulates into a dW of exactly M * C * T floats between sentinels,
gives the kernel a workspace of exactly the planner's size between sentinels, launches twice (fixed summation order: bit-identical) and
holds the result to the f64 contraction of the bf16x3 operands: what remains is the f32 accumulation order.

The grouped table is sized from the planner's documented rule (group_plan below: K-steps per workgroup = clamp(ceil(work / 768), 8, 128),
32 output pixels per step); the planned workspace and grid must equal what that rule predicts, and test_kernel_census.py checks that the
table reaches slab counts of 1, 2..4 and >= 6, the scalar reduce and both launch geometries (gx * gy a multiple of 8 or not).

Gates: each is at most 10x the worst value measured on MI355X for its family (GATES lists both)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import exact_ref as X  # noqa: E402
from test_persistent_edges_gpu import _FlatOut, gen, normalise, seed_of, values  # noqa: E402
from villandiffusion_amd import lib as L  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.lib import B_CONV3, B_CONV3_S2, B_CONV3_UP, B_PLAIN  # noqa: E402

DEV = X.DEV
# family: gate  -- measured worst value alongside
GATES = {"wgrad_bx3": 5e-6,             # 1.63e-6 (unsplit single launches: 128 K-steps in one f32 accumulator; 4.2e-7 grouped, 3.4e-7 split)
         "wgrad_k32_single": 5e-6,      # 7.72e-7 (unsplit; 3.9e-7 split)
         "wgrad1x1_single": 3e-6}       # 5.52e-7 (unsplit; 3.5e-7 split)
WORST = {}


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------- names, classes, plans (pure)
CLASS_MODE = {16: B_CONV3, 2008: B_CONV3_S2, 2016: B_CONV3_S2, 2032: B_CONV3_S2, 2033: B_CONV3_S2, 129: B_CONV3, 131: B_CONV3_UP}
CLASS_ARGS = {16: "4, 0", 2008: "8, 4", 2016: "16, 4", 2032: "32, 4", 2033: "32, 4, true", 129: "32, 0, true", 131: "32, 2, true"}


def group_name(cls):
    return normalise(f"wgrad_bx3_group_kernel<{CLASS_ARGS[cls]}>")


def source_dims(mode, OH, OW):
    """The input image under an OH x OW output."""
    return {B_CONV3_UP: (OH // 2, OW // 2), B_CONV3_S2: (2 * OH, 2 * OW)}.get(mode, (OH, OW))


def group_plan(jobs):
    """The grouped planner's documented rule for the 3x3 classes of wgrad_bx3_group_kernel.  jobs: [(M, C, nb, NP)] -> ([(gx, gy)], workspace
    floats, compute blocks).  A job is 3 * ceil(M / 128) * ceil(C / 64) tiles of ceil(nb * NP / 32) K-steps; every workgroup gets
    clamp(ceil(work / 768), 8, 128) steps; a split job owns gy slabs of M * C * 9 floats (16-byte aligned) and its blocks are padded to 8."""
    base = [cdiv(M, 128) * cdiv(Cc, 64) * 3 for M, Cc, _, _ in jobs]
    ks = [cdiv(nb * NP, 32) for _, _, nb, NP in jobs]
    per = min(max(cdiv(sum(b * k for b, k in zip(base, ks)), 768), 8), 128)
    grid, off, blk = [], 0, 0
    for (M, Cc, _, _), b, k in zip(jobs, base, ks):
        gy = cdiv(k, cdiv(k, max(cdiv(k, per), 1)))
        grid.append((b, gy))
        blk += cdiv(b * gy, 8) * 8
        if gy > 1:
            off = cdiv(off + gy * M * Cc * 9, 4) * 4
    return grid, off, blk


# ------------------------------------------------------------------------------------------------------------- case tables
# grouped wgrad_bx3_group_kernel: id, class, values, jobs [(B, Cin, Cout, OH, OW, pad)].  M in {72, 136} / C in {72, 80}: second m- and
# c-tiles that are nearly empty; (67 -> 65): M * C * 9 odd, the scalar reduce.  Slab counts (group_plan) alongside.  (Stride 2 at 8-pixel
# outputs has one octet per row, so the 17th column of its window is always the zero padding; from 16 pixels up it is a loaded pixel.)
GW = [
    ("w4_unsplit", 16, "std", [(1, 72, 72, 4, 4, 0), (7, 80, 136, 4, 4, 0)]),                 # B = 1: one half-empty step; B = 7: 4 steps, the last half empty; 1, 1
    ("w4_split", 16, "std", [(40, 72, 136, 4, 4, 0), (101, 80, 72, 4, 4, 0)]),                # 3 slabs (36 blocks) and 7 (42 blocks), odd batch
    ("w4_odd", 16, "wide", [(33, 67, 65, 4, 4, 0), (12, 72, 72, 4, 4, 0)]),                   # 3 slabs of an odd M * C * 9, 1
    ("s2_8", 2008, "std", [(3, 72, 72, 8, 8, 0), (28, 80, 136, 8, 8, 1)]),                    # 1 and 7 slabs, the paddings mixed in one group
    ("s2_8_odd", 2008, "wide", [(12, 67, 65, 8, 8, 1), (16, 72, 136, 8, 8, 0)]),              # 3 (odd) and 4 slabs (48 blocks: the XCD remap)
    ("s2_16", 2016, "std", [(1, 72, 72, 16, 16, 1), (7, 80, 136, 16, 16, 0)]),                # 1 and 7
    ("s2_16_odd", 2016, "wide", [(3, 67, 65, 16, 16, 0), (4, 72, 136, 16, 16, 1)]),           # 3 (odd) and 4
    ("s2_32", 2032, "std", [(1, 72, 72, 32, 32, 0), (2, 80, 136, 32, 32, 1)]),                # 4 (24 blocks) and 8 (96)
    ("s2_32_odd", 2032, "wide", [(1, 67, 65, 32, 32, 1), (1, 72, 72, 32, 32, 0)]),            # 4 (odd) and 4
    ("s2_w64", 2033, "std", [(1, 72, 72, 64, 64, 0), (1, 80, 136, 64, 64, 1)]),               # input 128 -> output 64, two segments: 16 and 16
    ("s2_w64_odd", 2033, "wide", [(1, 67, 65, 64, 64, 1), (1, 72, 72, 64, 64, 0)]),
    ("seg", 129, "std", [(2, 72, 72, 8, 96, 0), (3, 80, 136, 8, 64, 0)]),                    # three segments (a middle one) and two; 8-row images
    ("seg_odd", 129, "wide", [(1, 67, 65, 8, 64, 0), (1, 72, 72, 4, 64, 0)]),                # 2 slabs (odd) and an unsplit 4 x 64 image
    ("seg_up", 131, "std", [(1, 72, 72, 64, 64, 0), (1, 80, 136, 8, 64, 0)]),                # source 32 -> output 64; source 4 x 32
    ("seg_up_odd", 131, "wide", [(1, 67, 65, 8, 96, 0), (1, 72, 136, 64, 64, 0)]),           # source 4 x 48: three segments
]


def gw_jobs(row):
    """(M, C, nb, NP) per job, as group_plan takes them."""
    return [(Cout, Cin, B, OH * OW) for B, Cin, Cout, OH, OW, _ in row[3]]


def gw_cases():
    return [pytest.param(row, id=row[0]) for row in GW]


# single launch, 3x3: id, expected instantiation, mode, B, Cin, Cout, OH, OW, pad, values.  B: the planner's own split count is above 1
# (at least 16 K-steps of 32 pixels; 4x4: two images per step).
SW = [
    ("b_w4", "wgrad_bx3_kernel<4, 0>", B_CONV3, 33, 72, 136, 4, 4, 0, "std"),                 # odd batch: the last step is half empty
    ("b_w4_odd", "wgrad_bx3_kernel<4, 0>", B_CONV3, 32, 67, 65, 4, 4, 0, "wide"),
    ("b_s2_8_p0", "wgrad_bx3_kernel<8, 4>", B_CONV3_S2, 9, 80, 72, 8, 8, 0, "std"),
    ("b_s2_8_p1", "wgrad_bx3_kernel<8, 4>", B_CONV3_S2, 9, 67, 65, 8, 8, 1, "std"),
    ("b_s2_16_p0", "wgrad_bx3_kernel<16, 4>", B_CONV3_S2, 3, 72, 136, 16, 16, 0, "std"),
    ("b_s2_16_p1", "wgrad_bx3_kernel<16, 4>", B_CONV3_S2, 3, 80, 72, 16, 16, 1, "wide"),
    ("b_s2_32_p0", "wgrad_bx3_kernel<32, 4>", B_CONV3_S2, 1, 80, 72, 32, 32, 0, "std"),
    ("b_s2_32_p1", "wgrad_bx3_kernel<32, 4>", B_CONV3_S2, 1, 72, 136, 32, 32, 1, "std"),
    ("b_s2_w_p0", "wgrad_bx3_kernel<32, 4, true>", B_CONV3_S2, 1, 72, 72, 64, 64, 0, "std"),
    ("b_s2_w_p1", "wgrad_bx3_kernel<32, 4, true>", B_CONV3_S2, 1, 67, 65, 64, 64, 1, "std"),
    ("b_wide", "wgrad_bx3_kernel<32, 0, true>", B_CONV3, 2, 72, 136, 8, 96, 0, "std"),
    ("b_wide_up", "wgrad_bx3_kernel<32, 2, true>", B_CONV3_UP, 2, 80, 72, 8, 64, 0, "std"),
    ("k_8", "wgrad_k32_kernel<8, 0>", B_CONV3, 9, 72, 136, 8, 8, 0, "std"),
    ("k_8up", "wgrad_k32_kernel<8, 2>", B_CONV3_UP, 9, 67, 65, 8, 8, 0, "std"),
    ("k_16", "wgrad_k32_kernel<16, 0>", B_CONV3, 3, 67, 65, 16, 16, 0, "wide"),
    ("k_16up", "wgrad_k32_kernel<16, 2>", B_CONV3_UP, 3, 80, 136, 16, 16, 0, "std"),
    ("k_32", "wgrad_k32_kernel<32, 0>", B_CONV3, 1, 80, 72, 32, 32, 0, "std"),
    ("k_32up", "wgrad_k32_kernel<32, 2>", B_CONV3_UP, 1, 72, 136, 32, 32, 0, "std"),
]
# single launch, 1x1 (wgrad1x1_bx3_kernel: 128 x 128 tiles, K-steps of 64 pixels): id, B, Cin, Cout, side, values
S1 = [
    ("one_ragged_k", 29, 128, 128, 4, "std"),          # 58 octets: the last of 8 K-steps holds two, and every step spans four images
    ("one_ragged_mc", 8, 200, 136, 8, "wide"),         # second m- and c-tiles nearly empty
    ("one_odd", 9, 67, 65, 8, "std"),                  # M * C odd: slab_reduce_scalar_kernel
]


def sw_cases():
    return [pytest.param(row, id=row[0]) for row in SW]


def s1_cases():
    return [pytest.param(row, id=row[0]) for row in S1]


def sw_family(row):
    return "wgrad_k32_single" if row[1].startswith("wgrad_k32") else "wgrad_bx3"


def all_expected_names():
    """Every template instantiation the cases of this module reach (test_kernel_census.py compares them with the library)."""
    return {group_name(row[1]) for row in GW} | {normalise(row[1]) for row in SW}


PLAIN_KERNELS = ("wgrad1x1_bx3_kernel",)          # not templates: reached by name (the S1 cases)


# ------------------------------------------------------------------------------------------------------------------ helpers
def check(family, err, what):
    WORST[family] = max(WORST.get(family, 0.0), err)
    print(f"[wgrad-edge] {family} {what}: {err:.2e} (gate {GATES[family]:.0e})")
    assert err <= GATES[family], (family, what, err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[wgrad-edge] worst error per family against the exact reference:")
    for fam, v in sorted(WORST.items()):
        print(f"[wgrad-edge]   {fam:18s} {v:.2e}   gate {GATES[fam]:.0e}")


def operands(B, Cin, Cout, OH, OW, mode, vals, seed):
    """x, dy (plain tensors, for the reference), their NaN-surrounded channel slices, the initial dW and its guarded buffer."""
    T = 1 if mode == B_PLAIN else 9
    H, W = source_dims(mode, OH, OW)
    x = values((B, Cin, H, W), vals, seed)
    dy = values((B, Cout, OH, OW), "std", seed + 3)
    dw0 = torch.randn(Cout, Cin * T, generator=gen(seed + 5)).to(DEV)
    return x, dy, X.nan_slice(x), X.nan_slice(dy, pre=16, post=8), dw0, X.GuardedFlat(Cout * Cin * T)


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("H,W", [(16, 16), (12, 136)])
@pytest.mark.parametrize("pad", [0, 1])
def test_the_stride2_reference_is_autograd_of_a_float64_convolution(H, W, pad):
    B, Cin, Cout = 2, 5, 6
    x = torch.randn(B, Cin, H, W, generator=gen(1), dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen(2), dtype=torch.float64).requires_grad_()
    y = F.conv2d(x, w, None, stride=2, padding=1) if pad else F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=2)
    assert y.shape[2:] == (H // 2, W // 2)
    dy = torch.randn(y.shape, generator=gen(3), dtype=torch.float64)
    y.backward(dy)
    got = X.wgrad_f64(dy, x, B_CONV3_S2, pad=pad).cpu()
    assert X.rel(got, w.grad.view(Cout, -1)) <= 1e-12
    acc = torch.randn(Cout, Cin * 9, generator=gen(4))
    got = X.wgrad_arith_f64(dy.float(), x.float(), B_CONV3_S2, "f32", acc=acc, pad=pad).cpu()          # the arithmetic wrapper passes pad on
    assert X.rel(got, X.wgrad_f64(dy.float(), x.float(), B_CONV3_S2, pad=pad).cpu() + acc.double()) <= 1e-12


# ------------------------------------------------------------------------------------------------ grouped wgrad_bx3_group_kernel
@pytest.mark.parametrize("row", gw_cases())
def test_grouped_wgrad_bx3_edges(row, monkeypatch):
    rid, cls, vals, jobs = row
    seed, mode = seed_of(rid), CLASS_MODE[cls]
    descs, keep, refs, outs, inits = [], [], [], [], []
    for k, (B, Cin, Cout, OH, OW, pad) in enumerate(jobs):
        x, dy, xo, dyo, dw0, o = operands(B, Cin, Cout, OH, OW, mode, vals, seed + 10 * k)
        d = ops.wgrad_desc(dyo, xo, o.view.view(Cout, Cin * 9), mode, None, accumulate=True, pad=pad, math_mode=1)
        assert ops.wgrad_group_class(d) == cls, (ops.wgrad_group_class(d), cls)
        descs.append(d)
        keep.append((xo, dyo))
        refs.append(X.wgrad_arith_f64(dy, x, mode, "bf16x3", acc=dw0, pad=pad))
        outs.append(_FlatOut(o))
        inits.append(dw0)
    grid, ws_want, blocks_want = group_plan(gw_jobs(row))
    wsf, blocks = X.wgrad_group_ws_floats(descs)
    assert (wsf, blocks) == (ws_want, blocks_want), f"planned workspace / grid {wsf} / {blocks}, the documented rule gives {ws_want} / {blocks_want} ({grid})"
    ws = X.GuardedFlat(wsf)
    monkeypatch.setitem(ops._WG_WS, torch.device(DEV), ws.view)
    res = []
    for rep in range(2):
        for o, i in zip(outs, inits):
            o.fresh()
            o.view.copy_(i.flatten())
        ws.arm()
        if rep == 0:
            ops.profile_start()
        ops.conv_wgrad_group(descs, torch.device(DEV))
        if rep == 0:
            names = [r["name"] for r in ops.profile_stop()]
            assert len(names) == 1 and normalise(names[0]) == group_name(cls), (names, group_name(cls))
        torch.cuda.synchronize()
        assert ws.intact(), "the grouped weight gradient wrote outside its planned workspace"
        assert all(o.intact() for o in outs), "a write landed outside dW"
        res.append([o.view.clone() for o in outs])
    for k, (a, c) in enumerate(zip(*res)):
        assert torch.equal(a, c), "two launches of a fixed-order kernel differ"
        check("wgrad_bx3", X.rel(a.view_as(refs[k]), refs[k]), f"{rid} job {k} ({grid[k][0]} tiles x {grid[k][1]} slabs)")


# ------------------------------------------------------------------------------------------------------- single launches
def _single(rid, family, name, tile_want, mode, B, Cin, Cout, OH, OW, pad, vals):
    """ops.conv_wgrad at math_mode = 1, unsplit and at the planner's own split count, twice each."""
    T = 1 if mode == B_PLAIN else 9
    x, dy, xo, dyo, dw0, o = operands(B, Cin, Cout, OH, OW, mode, vals, seed_of(rid))
    dw = o.view.view(Cout, Cin * T)
    ref = X.wgrad_arith_f64(dy, x, mode, "bf16x3", taps=T, acc=dw0, pad=pad)
    lib = L.load()
    for forced in (1, 0):
        d = ops.wgrad_desc(dyo, xo, dw, mode, None, accumulate=True, splits=forced, pad=pad, math_mode=1)
        tile, splits = C.c_int32(0), C.c_int32(0)
        assert lib.vd_conv_wgrad_plan(C.byref(d), C.byref(tile), C.byref(splits)) == 0
        assert tile.value == tile_want, (tile.value, tile_want)
        need = ops.wgrad_ws_floats(Cout, Cin, T, B, OH * OW, OH, OW, mode, math_mode=1) if forced == 0 else 0
        assert int(lib.vd_conv_wgrad_ws_floats(C.byref(d))) == need
        if forced == 0:
            assert splits.value > 1 and need == splits.value * Cout * Cin * T, (splits.value, need)
        else:
            assert splits.value == 1
        ws = X.GuardedFlat(need)
        res = []
        for rep in range(2):
            o.arm()
            o.view.copy_(dw0.flatten())
            ws.arm()
            if rep == 0:
                ops.profile_start()
            ops.conv_wgrad(dyo, xo, dw, mode, ws.view if need else None, accumulate=True, splits=forced, pad=pad, math_mode=1)
            if rep == 0:
                names = [r["name"] for r in ops.profile_stop()]
                assert len(names) == 1 and names[0].endswith("(+slab_reduce)"), names
                got_name = names[0][:-len("(+slab_reduce)")]
                assert (got_name if name in PLAIN_KERNELS else normalise(got_name)) == (name if name in PLAIN_KERNELS else normalise(name)), (names, name)
            torch.cuda.synchronize()
            assert ws.intact(), "the weight gradient wrote outside its planned workspace"
            assert o.intact(), "a write landed outside dW"
            res.append(o.view.clone())
        assert torch.equal(res[0], res[1]), "two launches of a fixed-order kernel differ"
        check(family, X.rel(res[0].view_as(ref), ref), f"{rid} {splits.value} split(s)")


@pytest.mark.parametrize("row", sw_cases())
def test_single_wgrad_3x3_edges(row):
    rid, name, mode, B, Cin, Cout, OH, OW, pad, vals = row
    _single(rid, sw_family(row), name, 4, mode, B, Cin, Cout, OH, OW, pad, vals)


@pytest.mark.parametrize("row", s1_cases())
def test_single_wgrad_1x1_edges(row):
    rid, B, Cin, Cout, S, vals = row
    _single(rid, "wgrad1x1_single", "wgrad1x1_bx3_kernel", 5, B_PLAIN, B, Cin, Cout, S, S, 0, vals)
