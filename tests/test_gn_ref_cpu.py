"""The GroupNorm edge tests' own ground (tests/gn_ref.py), checked without a GPU: the float64 backward formula against float64 autograd,
plain torch float32 against every bound, the hard inputs, the library's host-only dispatch query against the case table, and a census of
the gn_* kernels of vd_norm.hip in the built library against the kernels the cases name."""
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import gn_ref as R
from villandiffusion_amd import lib, ops

# the kernel families of vd_norm.hip; the pre-split GroupNorm kernels of vd_presplit.hip have their own tests (test_presplit_gpu.py)
FAMILIES = ("gn_fwd_reg_kernel", "gn_fwd_wave_kernel", "gn_fwd_kernel", "gn_bwd_kernel", "gn_bwd_reg_kernel", "gn_bwd_wave_kernel",
            "gn_chunk_stats_kernel", "gn_chunk_apply_kernel", "gn_chunk_bwd_stats_kernel", "gn_chunk_bwd_apply_kernel", "gn_chunk_rowsum_kernel",
            "gn_chunk1_fwd_kernel", "gn_chunk1_bwd_kernel", "gn_stats_from_part_kernel")
ELSEWHERE = ("gn_fwd_ps_kernel", "gn_bwd_ps_kernel")
UNREACHABLE = {
    "gn_chunk1_bwd_kernel<16>": "the backward cuts chunks of at most 8192 floats (gn_chunks), so slab / S > 8192 is never true in vd_groupnorm_bwd_fused",
}


def _ref(dims, kind, silu, _cache={}):
    key = (dims, kind, silu)
    if key not in _cache:
        _cache[key] = R.Reference(dims, kind, silu)
    return _cache[key]


SMALL = [d for d in R.CASES if d[1] * d[2] * d[3] <= 1 << 16]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("dims", [(3, 6, 2, 2, 3), (2, 6, 12, 12, 3), (3, 12, 7, 7, 3), (1, 64, 4, 4, 1)], ids=str)
def test_backward_formula_is_float64_autograd(dims, silu):
    B, C, H, W, G = dims
    x = R.make_input("plain", B, C, H, W, G).double().requires_grad_()
    gamma, beta = (t.double() for t in R.make_params(C))
    dy, extra, extra2 = R.make_grads(x.shape)
    dgs, dbs = [], []
    for b in range(B):                                          # the rows are per image
        g_, b_ = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        y = F.group_norm(x[b:b + 1], G, g_, b_, R.EPS)
        (F.silu(y) if silu else y).backward(dy[b:b + 1].double())
        dgs.append(g_.grad)
        dbs.append(b_.grad)
    mean, rstd = R.stats_f64(x.detach().float(), G)
    dx, dg, db, rs = R.bwd_f64(dy, x.detach().float(), mean, rstd, gamma.float(), beta.float(), G, silu, extra, extra2)
    want = x.grad + extra.double() + extra2.double()
    assert R.slab_err(dx, want, G) <= 1e-12
    assert R.row_err(dg, torch.stack(dgs)) <= 1e-12 and R.row_err(db, torch.stack(dbs)) <= 1e-12
    assert R.row_err(rs, want.sum((2, 3))) <= 1e-12
    yf, mf, rf = R.fwd_f64(x.detach().float(), gamma.float(), beta.float(), G, silu)
    y64 = F.group_norm(x.detach(), G, gamma, beta, R.EPS)
    assert R.slab_err(yf, F.silu(y64) if silu else y64, G) <= 1e-12
    ss = R.ss_f64(x.detach().float(), gamma.float(), beta.float(), G)
    z = x.detach() * ss[:, :, 0, None, None] + ss[:, :, 1, None, None]
    assert R.slab_err(z, y64, G) <= 1e-10                       # scale / shift reproduce the normalisation


@pytest.mark.parametrize("dims,kind", [(d, k) for d in R.CASES for k in R.KINDS if d in SMALL or k == "plain"], ids=str)   # the 10 MB case: plain only
def test_torch_float32_passes_every_bound(dims, kind):
    """Each bound is max(floor, 4 x torch float32's error), so torch passes by construction; what is asserted beyond that is WHERE the floor
    decides: on plain, outlier and flat inputs torch float32 stays under the suite's tolerance for y, mean, rstd and dx, so the tolerance is
    the bound there.  The measured term decides on `offset` (mean 100 x the spread), and for the [B, C] rows where they are cancelling sums
    (a flat image's dx is 1000 x its residuals, and the dx of a one-channel group sums to zero); no bound of a combination the GPU tests
    run exceeds the 1e-3 the project promises end to end."""
    ref = _ref(dims, kind, True)
    for what, terr in sorted(ref.torch_err.items()):
        bnd, _ = ref.bound(what)
        print(f"[bounds] gn {dims} {kind} {what}: torch_f32={terr:.3e} floor={ref.floor[what]:.1e} bound={bnd:.3e}")
        assert terr == terr and terr <= bnd
        if kind == "plain" or dims in R.KIND_CASES:             # what the GPU tests run
            assert bnd <= 1e-3, (what, bnd)
        if kind != "offset" and what in ("y", "mean", "rstd", "dx0", "dx1", "dx2"):
            assert terr <= ref.floor[what], (what, terr)


def test_hard_inputs_are_what_they_claim():
    for dims in R.KIND_CASES:
        B, C, H, W, G = dims
        flat = R.make_input("flat", B, C, H, W, G)
        assert bool((flat[0] == 0).all())
        y, mean, rstd = R.fwd_f64(flat, *R.make_params(C), G, True)
        assert bool(torch.isfinite(y).all()) and bool((mean[:G] == 0).all())
        assert torch.allclose(rstd[:G], torch.full((G,), R.EPS ** -0.5, dtype=torch.float64), rtol=1e-12)     # zero variance: rstd = 1000
        if B > 1:
            assert bool((rstd[G:] < 10).all())
        off = R.make_input("offset", B, C, H, W, G).double().view(B, G, -1)
        assert bool((off.mean(-1) / off.std(-1).clamp(min=1e-3) > 50).all()) or C // G * H * W < 32
        out = R.make_input("outlier", B, C, H, W, G)
        assert bool((out[:, :, 0, 0] == 50).all()) and float(out.flatten(2)[:, :, 1:].abs().max()) < 1
        for kind in R.KINDS:
            assert R._mean_condition(R.make_input(kind, B, C, H, W, G), G) <= R.MEAN_COND_MAX


def test_metric_sees_a_wrong_small_group_and_an_exact_zero():
    a = torch.zeros(2, 4, 2, 2)
    a[0, :2], a[0, 2:], a[1] = 1000.0, 1.0, 1.0
    b = a.clone()
    b[0, 3, 0, 0] = 1.01                                         # 1e-2 of its own slab, 1e-5 of the tensor
    assert R.slab_err(b, a, 2) == pytest.approx(1e-2) and float((a - b).abs().max() / a.abs().max()) < 2e-5
    assert R.row_err(torch.zeros(2, 3), torch.zeros(2, 3)) == 0 and R.row_err(torch.full((2, 3), 1e-9), torch.zeros(2, 3)) == float("inf")
    assert R.elem_err(torch.tensor([0.0, 2.0]), torch.tensor([0.0, 1.0])) == 1.0
    assert not (R.slab_err(torch.full_like(a, float("nan")), a, 2) <= 1.0)


def test_partial_statistics_reference_matches_the_direct_one():
    B, C, HW, G, tiles = 2, 6, 64, 3, 4
    x = R.make_input("plain", B, C, 8, 8, G)
    gamma, beta = R.make_params(C)
    t = x.double().view(B, C, tiles, HW // tiles)
    part = torch.stack([t.sum(-1), (t * t).sum(-1)], -1).permute(0, 2, 1, 3).contiguous()
    ss, mean, rstd = R.partial_stats_f64(part, gamma, beta, HW, G)
    m0, r0 = R.stats_f64(x, G)
    assert R.elem_err(mean, m0) <= 1e-12 and R.elem_err(rstd, r0) <= 1e-12
    assert float((ss - R.ss_f64(x, gamma, beta, G)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------- the library's dispatch query
def test_plan_query_reports_the_table_without_a_device():
    """vd_groupnorm_plan runs the entry points' own choice functions on the host.  The one-launch polling kernels need a device's
    occupancy figures, so without one the chunked cases report the two-launch names (the GPU test asserts the one-launch names); every
    other name, every S and every refusal must be the table's here already."""
    two = R.child_cases()
    for dims, (f, fs, b, bs) in R.CASES.items():
        B, C, H, W, G = dims
        name, S = ops.groupnorm_plan(ops.GN_FWD, B, C, H * W, G)
        assert S == fs and name in ((f, two[dims][0]) if R.is_chunked(f) else (f,)), (dims, name, S)
        if b is R.REFUSED:
            with pytest.raises(lib.VillanHipError, match="bad dims"):
                ops.groupnorm_plan(ops.GN_BWD, B, C, H * W, G)
        else:
            name, S = ops.groupnorm_plan(ops.GN_BWD, B, C, H * W, G)
            assert S == bs and name in ((b, two[dims][2]) if R.is_chunked(b) else (b,)), (dims, name, S)
        # unaligned, or without a workspace: the generic kernels
        assert ops.groupnorm_plan(ops.GN_FWD, B, C, H * W, G, aligned=False) == (R.FWD_GENERIC, 0)
        assert ops.groupnorm_plan(ops.GN_FWD, B, C, H * W, G, has_ws=False)[0] == (R.FWD_GENERIC if R.is_chunked(f) else f)
        if b is not R.REFUSED:
            assert ops.groupnorm_plan(ops.GN_BWD, B, C, H * W, G, aligned=False) == (R.BWD_GENERIC, 0)
            assert ops.groupnorm_plan(ops.GN_BWD, B, C, H * W, G, has_ws=False)[0] == (R.BWD_GENERIC if R.is_chunked(b) else b)
    for dims, name in R.stats_cases().items():
        B, C, H, W, G = dims
        assert ops.groupnorm_plan(ops.GN_STATS, B, C, H * W, G) == (name, 0), dims
    # the forward alone could chunk these two (has_ws forced): the workspace is sized by the backward, which cannot
    assert ops.groupnorm_plan(ops.GN_FWD, 1, 4, 20 * 461, 1, has_ws=True)[1] == 4
    assert ops.groupnorm_plan(ops.GN_FWD, 1, 40, 256 * 256, 1, has_ws=True)[1] == 160


@pytest.mark.parametrize("which,dims,aligned", [(ops.GN_BWD, (1, 130, 16, 2), True), (ops.GN_STATS, (1, 514, 4, 2), True),
                                                (ops.GN_STATS, (1, 1, 28676, 1), True), (ops.GN_STATS, (3, 12, 49, 3), True),
                                                (ops.GN_STATS, (2, 2, 1024, 1), False), (ops.GN_FWD, (2, 6, 16, 4), True),
                                                (ops.GN_BWD, (2, 6, 16, 4), True), (ops.GN_STATS, (2, 6, 16, 4), True), (3, (2, 6, 16, 3), True)])
def test_plan_query_refuses_what_the_entry_points_refuse(which, dims, aligned):
    with pytest.raises(lib.VillanHipError):
        ops.groupnorm_plan(which, *dims, aligned=aligned)


# --------------------------------------------------------------------------------------------------------------------- census
def library_instantiations():
    out = subprocess.check_output([shutil.which("nm") or "nm", "-C", lib.LIB_PATH], text=True)
    names, strangers = set(), set()
    for m in re.finditer(r"__device_stub__(gn_\w+)(<[^>]*>)?", out):
        if m.group(1) in FAMILIES:
            names.add(m.group(1) + (m.group(2) or ""))
        elif m.group(1) not in ELSEWHERE:
            strangers.add(m.group(1))
    return names, strangers


def test_every_groupnorm_instantiation_has_an_edge_case():
    if shutil.which("nm") is None:
        pytest.fail("nm (binutils) is needed to read the library's symbols")
    built, strangers = library_instantiations()
    assert strangers == set(), f"gn_* kernels of no known family: {sorted(strangers)}"
    covered = R.all_expected_names()
    assert set(UNREACHABLE) <= built and not (set(UNREACHABLE) & covered)
    reachable = built - set(UNREACHABLE)
    print(f"[census] {len(reachable & covered)} of {len(reachable)} GroupNorm instantiations covered; unreachable: {sorted(UNREACHABLE)}")
    assert reachable - covered == set(), f"instantiations without an edge case: {sorted(reachable - covered)}"
    assert covered - built == set(), f"edge cases expect instantiations the library does not have: {sorted(covered - built)}"


def test_census_fails_on_a_new_instantiation_and_on_a_case_without_a_kernel(monkeypatch):
    built, _ = library_instantiations()
    covered = R.all_expected_names()
    assert (built | {"gn_fwd_reg_kernel<16, 256>"}) - set(UNREACHABLE) - covered == {"gn_fwd_reg_kernel<16, 256>"}
    monkeypatch.setitem(R.CASES, (1, 1, 4, 4, 1), ("gn_fwd_wave_kernel<8>", 0, "gn_bwd_wave_kernel<1>", 0))
    assert R.all_expected_names() - built == {"gn_fwd_wave_kernel<8>"}
