"""GroupNorm (vd_norm.hip) at its dispatch edges, odd groupings and hard inputs, against the float64 references of tests/gn_ref.py.

Every case of gn_ref.CASES names the kernel the library must take for it (ops.groupnorm_plan, a host-only query of the same choice
functions the entry points switch on), so a dispatch change cannot silently move a case off its kernel; test_gn_ref_cpu.py checks that
the cases together reach every gn_* instantiation of the built library.  Operands sit inside NaN and outputs inside a sentinel pattern
(exact_ref), errors are taken per (image, group) slab, and each bound is max(the suite's tolerance, 4 x torch float32's own error)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_ref as X  # noqa: E402
import gn_ref as R  # noqa: E402
from villandiffusion_amd import lib as L  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402

DEV = "cuda"
SENT = X.SENTINEL
BIG = 1 << 20           # elements: the one large case runs once (plain, SiLU on)


@functools.lru_cache(maxsize=None)
def ref(dims, kind, silu):
    return R.Reference(dims, kind, silu)


def _aligned(*ts):
    return all(t is None or (t.data_ptr() % 16 == 0 and (t.shape[0] == 1 or t.stride(0) % 4 == 0)) for t in ts)


def check_plan(dims, names, aligned=True, has_ws=None):
    B, Cc, H, W, G = dims
    f, fs, b, bs = names
    assert ops.groupnorm_plan(ops.GN_FWD, B, Cc, H * W, G, aligned, has_ws, ops._s()) == (f, fs), dims
    if b is R.REFUSED:
        with pytest.raises(L.VillanHipError, match="bad dims"):
            ops.groupnorm_plan(ops.GN_BWD, B, Cc, H * W, G, aligned, has_ws, ops._s())
    else:
        assert ops.groupnorm_plan(ops.GN_BWD, B, Cc, H * W, G, aligned, has_ws, ops._s()) == (b, bs), dims


class Rows:
    """Rows [B, n] as columns [8, 8 + n) of a [B, n + 16] matrix whose other columns hold the sentinel."""

    def __init__(self, B, n):
        self.buf = torch.empty(B, n + 16, device=DEV)
        self.view, self.ld = self.buf[:, 8:8 + n], n + 16
        self.mask = torch.ones(B, n + 16, dtype=torch.bool, device=DEV)
        self.mask[:, 8:8 + n] = False

    def arm(self):
        self.buf.view(torch.int32).fill_(SENT)
        self.view.fill_(float("nan"))
        return self.view

    def intact(self):
        return bool((self.buf.view(torch.int32)[self.mask] == SENT).all())


def fwd_via_ops(x, gamma, beta, y, mean, rstd, G, silu):
    ops.groupnorm_fwd(x, gamma, beta, y, mean, rstd, G, R.EPS, silu)


def fwd_without_ws(x, gamma, beta, y, mean, rstd, G, silu):
    B, Cc, H, W, xbs = ops._img(x)
    L.check(L.load().vd_groupnorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, Cc, H * W,
                                      G, R.EPS, int(silu), xbs, ops._img(y)[4], None, ops._s()), "vd_groupnorm_fwd")


def bwd_via_ops(dy, x, mean, rstd, gamma, beta, dx, wg, wb, G, silu, extra, extra2, rowsum, ld):
    ops.groupnorm_bwd(dy, x, mean, rstd, gamma, beta, dx, wg, wb, G, silu, extra=extra, extra2=extra2, rowsum=rowsum, rowsum_ld=ld)


def bwd_without_ws(dy, x, mean, rstd, gamma, beta, dx, wg, wb, G, silu, extra, extra2, rowsum, ld, ws=None):
    B, Cc, H, W, xbs = ops._img(x)
    p = ops._p
    L.check(L.load().vd_groupnorm_bwd_fused(p(dy), p(x), p(mean), p(rstd), p(gamma), p(beta), p(extra), p(extra2), p(dx), p(wg), p(wb), p(rowsum), B, Cc,
                                            H * W, G, int(silu), ops._img(dy)[4], xbs, ops._img(extra)[4] if extra is not None else 0,
                                            ops._img(extra2)[4] if extra2 is not None else 0, ops._img(dx)[4], ld or 0, p(ws), ops._s()), "vd_groupnorm_bwd")


def run_forward(r, label="", x_dev=None, call=fwd_via_ops, want_aligned=True):
    """Forward of a Reference: x a channel slice of a wider NaN buffer (or x_dev), y a guarded slice, mean / rstd in exact-size guarded
    buffers; twice, bit-identical; y / mean / rstd against float64; sentinels intact, x unchanged."""
    B, Cc, H, W, G = r.dims
    x = X.nan_slice(r.x.to(DEV)) if x_dev is None else x_dev
    gamma, beta = r.gamma.to(DEV), r.beta.to(DEV)
    yg, mg, rg = X.GuardedOut(B, Cc, H, W), X.GuardedFlat(B * G), X.GuardedFlat(B * G)
    if (H * W) % 4 == 0:
        assert _aligned(x, yg.view) == want_aligned
    outs = []
    for _ in range(2):
        call(x, gamma, beta, yg.fresh(), mg.arm(), rg.arm(), G, r.silu)
        torch.cuda.synchronize()
        assert yg.intact() and mg.intact() and rg.intact(), f"{r.dims} {label}: the forward wrote outside y / mean / rstd"
        outs.append((yg.view.clone(), mg.view.clone(), rg.view.clone()))
    assert all(torch.equal(u, v) for u, v in zip(*outs)), f"{r.dims} {label}: the forward is not deterministic"
    assert torch.equal(x, r.x.to(DEV)) and torch.equal(gamma, r.gamma.to(DEV)) and torch.equal(beta, r.beta.to(DEV))
    y, mean, rstd = outs[0]
    r.check("y", R.slab_err(y, r.y, G), label)
    r.check("mean", R.elem_err(mean, r.mean), label)
    r.check("rstd", R.elem_err(rstd, r.rstd), label)
    return y, mean, rstd


def run_backward(r, label="", x_dev=None, call=bwd_via_ops, variants=(0, 1, 2), want_aligned=True):
    """Backward of a Reference, fed the float32-rounded float64 statistics: no residual, extra, extra + extra2 (a slice of a wider buffer) +
    row sums (columns of a wider matrix); dx guarded, the dgamma / dbeta rows in exact-size guarded buffers and compared as rows; twice,
    bit-identical; every input unchanged."""
    B, Cc, H, W, G = r.dims
    x = X.nan_slice(r.x.to(DEV)) if x_dev is None else x_dev
    ins = {"dy": r.dy.to(DEV), "mean": r.mean32.to(DEV), "rstd": r.rstd32.to(DEV), "gamma": r.gamma.to(DEV), "beta": r.beta.to(DEV),
           "extra": r.extra.to(DEV), "extra2": X.nan_slice(r.extra2.to(DEV), pre=16, post=8)}
    keep = {k: v.clone() for k, v in ins.items()}
    dxg, wg, wb, rows = X.GuardedOut(B, Cc, H, W), X.GuardedFlat(B * Cc), X.GuardedFlat(B * Cc), Rows(B, Cc)
    if (H * W) % 4 == 0:
        assert _aligned(x, dxg.view, ins["dy"], ins["extra"], ins["extra2"]) == want_aligned
    for v in variants:
        e1 = ins["extra"] if v >= 1 else None
        e2, rs = (ins["extra2"], rows) if v == 2 else (None, None)
        outs = []
        for _ in range(2):
            call(ins["dy"], x, ins["mean"], ins["rstd"], ins["gamma"], ins["beta"], dxg.fresh(), wg.arm(), wb.arm(), G, r.silu, e1, e2,
                 rs.arm() if rs else None, rs.ld if rs else None)
            torch.cuda.synchronize()
            assert dxg.intact() and wg.intact() and wb.intact() and (rs is None or rs.intact()), \
                f"{r.dims} {label} variant {v}: the backward wrote outside dx / the rows"
            outs.append((dxg.view.clone(), wg.view.clone(), wb.view.clone()) + ((rs.view.clone(),) if rs else ()))
        assert all(torch.equal(a, b) for a, b in zip(*outs)), f"{r.dims} {label} variant {v}: the backward is not deterministic"
        dx, dg, db, rsum = r.bwd[v]
        r.check(f"dx{v}", R.slab_err(outs[0][0], dx, G), label)
        r.check("dgamma", R.row_err(outs[0][1].view(B, Cc), dg), f"{label} variant {v}")
        r.check("dbeta", R.row_err(outs[0][2].view(B, Cc), db), f"{label} variant {v}")
        if rs:
            r.check("rowsum", R.row_err(outs[0][3], rsum), label)
    assert torch.equal(x, r.x.to(DEV)) and all(torch.equal(ins[k], keep[k]) for k in ins), f"{r.dims} {label}: the backward changed an input"


def run_case(dims, kind, silu, names=None, label=""):
    names = names or R.CASES[dims]
    check_plan(dims, names)
    r = ref(dims, kind, silu)
    out = run_forward(r, label)
    if names[2] is not R.REFUSED:
        run_backward(r, label)
    return out


PLAIN = [(d, s) for d in R.CASES for s in (False, True) if s or d[1] * d[2] * d[3] < BIG]


@pytest.mark.parametrize("dims,silu", PLAIN, ids=str)
def test_every_dispatch_edge_on_plain_inputs(dims, silu):
    run_case(dims, "plain", silu)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("kind", [k for k in R.KINDS if k != "plain"])
@pytest.mark.parametrize("dims", R.KIND_CASES, ids=str)
def test_hard_inputs_on_every_kernel_family(dims, kind, silu):
    run_case(dims, kind, silu)


# ------------------------------------------------------------------------------------------------------------------ unaligned
@pytest.mark.parametrize("dims", R.UNALIGNED_CASES, ids=str)
def test_unaligned_tensors_take_the_generic_kernels(dims):
    B, Cc, H, W, G = dims
    n = Cc * H * W
    r = ref(dims, "plain", True)
    generic = (R.FWD_GENERIC, 0, R.BWD_GENERIC, 0)
    check_plan(dims, generic, aligned=False)
    # a storage offset of one float: every block takes the scalar branch
    buf = torch.full((B * n + 8,), float("nan"), device=DEV)
    x1 = buf[1:1 + B * n].view(B, Cc, H, W)
    x1.copy_(r.x)
    assert x1.data_ptr() % 16 == 4
    run_forward(r, "x + 1 float", x1, want_aligned=False)
    run_backward(r, "x + 1 float", x1, variants=(0, 2), want_aligned=False)
    # a batch stride of C * HW + 2: image 0 takes the vector branch, image 1 the scalar one
    buf = torch.full((B * (n + 2) + 8,), float("nan"), device=DEV)
    x2 = buf[:B * (n + 2)].view(B, n + 2)[:, :n].view(B, Cc, H, W)
    x2.copy_(r.x)
    assert x2.stride(0) == n + 2 and x2.data_ptr() % 16 == 0
    run_forward(r, "batch stride + 2", x2, want_aligned=False)
    run_backward(r, "batch stride + 2", x2, variants=(0, 2), want_aligned=False)
    # aligned, but called without a workspace: a chunkable slab then has only the generic kernels; the others keep theirs
    names = generic if R.is_chunked(R.CASES[dims][0]) else R.CASES[dims]
    check_plan(dims, names, has_ws=False)
    if names is generic:
        run_forward(r, "ws = NULL", call=fwd_without_ws)
        run_backward(r, "ws = NULL", call=bwd_without_ws, variants=(0, 2))


# ----------------------------------------------------------------------------------------------------------------- statistics
def _ss_check(what, got, want, torch32):
    """ss [B, C, 2]: the scales and the shifts as rows per image, bound = max(1e-5, 4 x torch float32's error)."""
    B = want.shape[0]
    for j, part in enumerate(("scale", "shift")):
        err, terr = R.row_err(got[..., j].reshape(B, -1), want[..., j].reshape(B, -1)), R.row_err(torch32[..., j].reshape(B, -1), want[..., j].reshape(B, -1))
        bnd = R.bound(R.TOL_FWD, terr)
        print(f"[parity] gn {what} ss {part}: err={err:.3e} torch_f32={terr:.3e} bound={bnd:.3e}")
        assert err <= bnd, (what, part, err, bnd)


def _torch_ss(gamma, beta, mean, rstd, B, Cc, G):
    sc = gamma.view(1, Cc) * R._bc(rstd, B, G, Cc // G).view(B, Cc)
    return torch.stack([sc, beta.view(1, Cc) - R._bc(mean, B, G, Cc // G).view(B, Cc) * sc], -1)


@pytest.mark.parametrize("dims", list(R.stats_cases()), ids=str)
def test_statistics_only_pass(dims):
    """vd_groupnorm_stats takes the forward's kernel, so its mean / rstd are the forward's bit for bit; ss against float64."""
    B, Cc, H, W, G = dims
    name = R.stats_cases()[dims]
    assert ops.groupnorm_plan(ops.GN_STATS, B, Cc, H * W, G) == (name, 0)
    assert ops.groupnorm_plan(ops.GN_FWD, B, Cc, H * W, G) == (name, 0)
    x32 = R.make_input("plain", B, Cc, H, W, G)
    g32, b32 = R.make_params(Cc)
    x, gamma, beta = X.nan_slice(x32.to(DEV)), g32.to(DEV), b32.to(DEV)
    ssg, mg, rg = X.GuardedFlat(B * Cc * 2), X.GuardedFlat(B * G), X.GuardedFlat(B * G)
    outs = []
    for _ in range(2):
        ops.groupnorm_stats(x, gamma, beta, ssg.arm().view(B, Cc, 2), mg.arm(), rg.arm(), G, R.EPS)
        torch.cuda.synchronize()
        assert ssg.intact() and mg.intact() and rg.intact()
        outs.append((ssg.view.clone(), mg.view.clone(), rg.view.clone()))
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    y, m2, r2 = torch.empty(B, Cc, H, W, device=DEV), torch.empty(B * G, device=DEV), torch.empty(B * G, device=DEV)
    ops.groupnorm_fwd(x, gamma, beta, y, m2, r2, G, R.EPS, False)
    assert torch.equal(outs[0][1], m2) and torch.equal(outs[0][2], r2), "statistics differ from the forward's"
    assert torch.equal(x, x32.to(DEV))
    mean, rstd = R.stats_f64(x32, G)
    _, tm, tr = R.torch_f32_fwd(x32, g32, b32, G, False)
    for what, got, want, t32 in (("mean", outs[0][1], mean, tm), ("rstd", outs[0][2], rstd, tr)):
        err, terr = R.elem_err(got, want), R.elem_err(t32, want)
        print(f"[parity] gn stats {dims} {what}: err={err:.3e} torch_f32={terr:.3e} bound={R.bound(R.TOL_FWD, terr):.3e}")
        assert err <= R.bound(R.TOL_FWD, terr)
    _ss_check(f"stats {dims}", outs[0][0].view(B, Cc, 2).cpu(), R.ss_f64(x32, g32, b32, G), _torch_ss(g32, b32, tm, tr, B, Cc, G))


@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("cpg", [1, 70])
@pytest.mark.parametrize("tiles", [1, 3])
def test_statistics_from_partials(tiles, cpg, kind):
    """vd_groupnorm_stats_from_partials on synthetic per-tile (sum, sum of squares): float64 of the same float32 partials.  The offset
    kind (mean 100, spread 1) makes E[x^2] - mean^2 cancel four digits, which the kernel's double accumulation has to carry."""
    B, G, P = 2, 3, 16
    Cc, HW = G * cpg, tiles * P
    v = R.make_input(kind, B, Cc, tiles, P, G).double()                                              # [B, C, tiles, P]
    part32 = torch.stack([v.sum(-1), (v * v).sum(-1)], -1).permute(0, 2, 1, 3).contiguous().float()     # [B, tiles, C, 2]
    g32, b32 = R.make_params(Cc)
    ss, mean, rstd = R.partial_stats_f64(part32, g32, b32, HW, G)
    assert bool((rstd < 100).all())                                                                 # the float32 partials still carry the variance
    pg = X.GuardedFlat(part32.numel())
    pg.view.copy_(part32.flatten())
    ssg, mg, rg = X.GuardedFlat(B * Cc * 2), X.GuardedFlat(B * G), X.GuardedFlat(B * G)
    ops.groupnorm_stats_from_partials(pg.view, tiles, g32.to(DEV), b32.to(DEV), ssg.view.view(B, Cc, 2), mg.view, rg.view, HW, G, R.EPS)
    torch.cuda.synchronize()
    assert ssg.intact() and mg.intact() and rg.intact() and torch.equal(pg.view.cpu(), part32.flatten())
    # torch float32 of the same formula from the same partials: what the bound allows for the final roundings of mean, rstd, scale, shift
    s = part32.double().sum(1).view(B, G, cpg, 2).sum(2)
    tm = (s[..., 0] / (cpg * HW)).float().flatten()
    tr = ((s[..., 1] / (cpg * HW) - (s[..., 0] / (cpg * HW)) ** 2).clamp(min=0) + R.EPS).rsqrt().float().flatten()
    for what, got, want, t32 in (("mean", mg.view, mean, tm), ("rstd", rg.view, rstd, tr)):
        err, terr = R.elem_err(got, want), R.elem_err(t32, want)
        print(f"[parity] gn partials tiles={tiles} cpg={cpg} {kind} {what}: err={err:.3e} torch_f32={terr:.3e} bound={R.bound(R.TOL_FWD, terr):.3e}")
        assert err <= R.bound(R.TOL_FWD, terr)
    _ss_check(f"partials tiles={tiles} cpg={cpg} {kind}", ssg.view.view(B, Cc, 2).cpu(), ss, _torch_ss(g32, b32, tm, tr, B, Cc, G))


# ------------------------------------------------------------------------------------------------------------------ refusals
def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _refused(call, outs, match):
    with pytest.raises(L.VillanHipError, match=match):
        call()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), "a refused call wrote to an output"


@pytest.mark.parametrize("what", ["bwd cpg 65", "stats cpg 257", "stats slab 28676", "stats HW % 4", "C % G", "rowsum_ld < C"])
def test_refusals_leave_the_outputs_untouched(what):
    dims = {"bwd cpg 65": (1, 130, 4, 4, 2), "stats cpg 257": (1, 514, 2, 2, 2), "stats slab 28676": (1, 1, 2, 14338, 1),
            "stats HW % 4": (3, 12, 7, 7, 3), "C % G": (2, 6, 4, 4, 4), "rowsum_ld < C": (2, 8, 4, 4, 2)}[what]
    B, Cc, H, W, G = dims
    x = torch.randn(B, Cc, H, W, device=DEV)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    mean, rstd = torch.zeros(B * G, device=DEV), torch.ones(B * G, device=DEV)
    y, dx, wg, wb, ss, rs = _nan(B, Cc, H, W), _nan(B, Cc, H, W), _nan(B * Cc), _nan(B * Cc), _nan(B, Cc, 2), _nan(B, Cc)
    om, orr = _nan(B * G), _nan(B * G)
    fwd = lambda: ops.groupnorm_fwd(x, gamma, beta, y, om, orr, G, R.EPS, True)                                  # noqa: E731
    bwd = lambda: ops.groupnorm_bwd(x, x, mean, rstd, gamma, beta, dx, wg, wb, G, True)                          # noqa: E731
    stats = lambda: ops.groupnorm_stats(x, gamma, beta, ss, om, orr, G, R.EPS)                                   # noqa: E731
    if what == "bwd cpg 65":
        _refused(bwd, (dx, wg, wb), "bad dims")
    elif what.startswith("stats cpg"):
        _refused(stats, (ss, om, orr), "bad dims")
    elif what.startswith("stats"):
        _refused(stats, (ss, om, orr), "16-B aligned groups of at most 28672")
    elif what == "C % G":
        for call in (fwd, bwd, stats):
            _refused(call, (y, dx, wg, wb, ss, om, orr), "bad dims")
    else:
        _refused(lambda: bwd_without_ws(x, x, mean, rstd, gamma, beta, dx, wg, wb, G, True, None, None, rs, Cc - 1), (dx, wg, wb, rs), "rowsum_ld < C")


# -------------------------------------------------------------------------------------------------------------- child process
def child_main(out_path):
    """Run inside a fresh process with VD_GN_CHUNK1_OFF=1 VD_GN_WAVE_OFF=1: the chunked cases take the two-launch kernels and the slabs
    of at most 1024 elements the smallest block kernels; the same checks under the same bounds, and the plan names of gn_ref.child_cases().
    The forward results of the chunked cases go to out_path for the parent."""
    assert os.environ.get("VD_GN_CHUNK1_OFF") == "1" and os.environ.get("VD_GN_WAVE_OFF") == "1"
    cases, saved = R.child_cases(), {}
    for dims, names in cases.items():
        for silu in (False, True):
            out = run_case(dims, "plain", silu, names, label="child")
            if silu and R.is_chunked(names[0]):
                saved[dims] = [t.cpu() for t in out]
    torch.save(saved, out_path)
    print(f"GN edges child ok: {len(cases)} cases")


def test_two_launch_and_block_kernels_in_a_child_process(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))), VD_GN_CHUNK1_OFF="1", VD_GN_WAVE_OFF="1")
    f = str(tmp_path / "two_launch.pt")
    r = subprocess.run([sys.executable, "-c", "import sys, test_groupnorm_edges_gpu as T; T.child_main(sys.argv[1])", f], capture_output=True,
                       text=True, env=env, cwd=root, timeout=300)
    print(r.stdout[-20000:])
    assert r.returncode == 0 and f"GN edges child ok: {len(R.child_cases())} cases" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    # the one-launch forward combines the same chunk partials in the same fixed order as the two-launch form: bit-identical y, mean, rstd
    saved = torch.load(f)
    assert sorted(saved) == sorted(d for d, n in R.CASES.items() if R.is_chunked(n[0]))
    for dims, two in saved.items():
        one = run_forward(ref(dims, "plain", True), "one launch")
        assert all(torch.equal(u.cpu(), v) for u, v in zip(one, two)), f"{dims}: the one-launch forward differs from the two-launch form"
