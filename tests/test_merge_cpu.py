"""Checkpoint merging without a GPU: rank_of, MergeConfig, the three C entry points in the header / the ctypes table / ops, vd_merge_plan and every
refusal of vd_merge_select and vd_merge_apply through ctypes with fake pointers (the checks run before any launch), the float32 oracle of
tests/merge_ref.py against its float64 restatement (exact on integers; within the derived bound on normal data), its properties, the refusals
of merge() and the tool's argument errors -- none of them may ask for a kernel."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import merge_ref
from villandiffusion_amd import lib, merge, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd.merge import MergeConfig, rank_of
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
f32 = np.float32


def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


# ------------------------------------------------------------------------------------------------------------------------------- host code
def test_rank_of_is_the_floor_in_float64_clamped():
    assert rank_of(0.0, 1000) == 0 and rank_of(1.0, 1000) == 1000 and rank_of(0, 0) == 0 and rank_of(1, 0) == 0
    assert rank_of(0.2, 100003) == 20000 and rank_of(0.2, 5) == 1 and rank_of(0.2, 4) == 0
    assert rank_of(0.3, 10) == math.floor(0.3 * 10.0) == 3                      # 0.3 * 10 is exactly 3.0 in float64
    assert rank_of(0.7, 10) == math.floor(0.7 * 10.0) == 7
    assert rank_of(0.29999999999999993, 10) == 2 and rank_of(0.30000000000000004, 10) == 3      # just below and just above an integer
    assert rank_of(math.nextafter(0.5, 0.0), 1 << 30) == (1 << 29) - 1 and rank_of(0.5, 1 << 30) == 1 << 29
    assert rank_of(math.nextafter(1.0, 0.0), 35746307) == 35746306
    for n in (1, 7, 2051, 35746307):
        for d in (0.0, 1e-9, 0.2, 0.5, 0.999999, 1.0):
            k = rank_of(d, n)
            assert 0 <= k <= n and k == min(n, int(math.floor(d * float(n))))


def test_merge_config_is_validated():
    c = MergeConfig()
    assert (c.method, c.density, c.lam, c.weights) == ("ties", 0.2, 1.0, None)
    assert MergeConfig(method="linear", density=1, lam=-0.5, weights=[0.5, 0.5, -1]).weights == (0.5, 0.5, -1.0)
    with pytest.raises(ValueError, match="method must be one of"):
        MergeConfig(method="dare")
    for bad in (-0.1, 1.1, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match=r"density must be a number in \[0, 1\]"):
            MergeConfig(density=bad)
    for bad in (float("inf"), float("nan"), True, "1"):
        with pytest.raises(ValueError, match="lam must be a finite number"):
            MergeConfig(lam=bad)
    for bad in ([], "0.5,0.5", [0.5, float("nan")], [True, 1.0], 0.5):
        with pytest.raises(ValueError, match="weights must be a non-empty sequence of finite numbers"):
            MergeConfig(method="linear", weights=bad)
    with pytest.raises(ValueError, match="weights are the per-task coefficients of method 'linear'; method is 'ties'"):
        MergeConfig(weights=[1.0])


def test_the_coefficients_are_float32_values_of_the_float64_rule():
    assert merge.coefficients(MergeConfig(method="linear", lam=0.7), 3) == [float(f32(0.7 / 3))] * 3
    assert merge.coefficients(MergeConfig(method="linear", lam=2.0, weights=[0.5, -1.0]), 2) == [1.0, -2.0]
    assert merge.coefficients(MergeConfig(method="linear", weights=[0.1, 0.2]), 2, lam=0.5) == [float(f32(0.5 * 0.1)), float(f32(0.5 * 0.2))]
    with pytest.raises(ValueError, match="holds 2 weights, but 3 task checkpoints"):
        merge.coefficients(MergeConfig(method="linear", weights=[0.1, 0.2]), 3)


def test_merge_refuses_by_name_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    net = UNet2DModel(**merge_ref.SMALL, device="cpu")
    n = net.flat_numel
    good = torch.zeros(n)
    for base, tasks, what in ((torch.zeros(8), [good], "base"), (good, [good, torch.zeros(n + 1)], r"tasks\[1\]"),
                              (good, [torch.zeros(n, dtype=torch.float64)], r"tasks\[0\]"), (good, [good, [0.0] * 4], r"tasks\[1\]"),
                              (good, [good, good, torch.zeros(n, device="meta")], r"tasks\[2\]"), (good, [torch.zeros(2 * n)[::2]], r"tasks\[0\]")):
        with pytest.raises(ValueError, match=rf"merge: {what} must be a flat contiguous float32 tensor of the model's {n} floats .* on cpu, got"):
            merge.merge(net, base, tasks, MergeConfig())
    with pytest.raises(ValueError, match=rf"{n} floats .*got \(8,\) torch.float32 on cpu"):
        merge.merge(net, torch.zeros(8), [good])
    with pytest.raises(ValueError, match="9 task checkpoints were given; one launch merges 1 to 8"):
        merge.merge(net, good, [good] * 9)
    with pytest.raises(ValueError, match="0 task checkpoints were given"):
        merge.merge(net, good, [])
    with pytest.raises(ValueError, match="holds 2 weights, but 3 task checkpoints"):
        merge.merge(net, good, [good] * 3, MergeConfig(method="linear", weights=[1.0, 1.0]))
    with pytest.raises(TypeError, match="MergeConfig"):
        merge.merge(net, good, [good], {"method": "ties"})
    with pytest.raises(ValueError, match="no batches"):
        merge.merge_scan(net, good, [good], MergeConfig(), None, [], [0.5])
    with pytest.raises(ValueError, match="every lam must be finite"):
        merge.merge_scan(net, good, [good], MergeConfig(), None, [good], [float("nan")])
    with pytest.raises(ValueError, match="must be copies, not the network's own flat_param"):
        merge.merge_scan(net, good, [net.flat_param.detach()], MergeConfig(), None, [good], [0.5])


# ------------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_table_and_ops_agree_on_the_three_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "villan_hip.h")).read(), flags=re.S)
    for name, n_args in (("vd_merge_plan", 5), ("vd_merge_select", 8), ("vd_merge_apply", 12)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m is not None and len(m.group(1).split(",")) == n_args == len(lib.PROTOTYPES[name][1]), name
        assert lib.PROTOTYPES[name][0] is lib._i32 and hasattr(lib.load(), name) and callable(getattr(ops, name[3:])), name
    assert "enum { VD_MERGE_LINEAR = 0, VD_MERGE_TIES = 1 };" in hdr and ops.MERGE_MODES == {"linear": 0, "ties": 1}
    assert lib.load().vd_abi_version() == 12 and "#define VD_ABI_VERSION 12" in hdr
    src = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_merge.hip" in src and re.search(r"vd_merge\.o:.*\n\t.*-ffp-contract=off", src)


def test_merge_plan_is_host_only_and_is_curve_plans_rule_with_the_scratch_bytes(monkeypatch):
    _no_kernels(monkeypatch)
    for n in (0, 1, 4096, 4097, 100003, 1 << 22, (1 << 22) + 1, (1 << 31) - 1):
        grid, block, fpt, ws = ops.merge_plan(n)
        assert (grid, block, fpt) == ops.curve_plan(n) and ws == 32 + grid * 257 * 4, n
    cap, block, fpt, ws = ops.merge_plan((1 << 31) - 1)
    assert (cap, block, fpt) == (1024, 256, 16) and ops.MERGE_PARTIAL == 18 * cap
    per = block * fpt
    assert ops.merge_plan(cap * per - 1)[0] == cap == ops.merge_plan(cap * per + 1)[0] and ops.merge_plan((cap - 1) * per)[0] == cap - 1
    h = lib.load()
    g, b, f, w = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert h.vd_merge_plan(-1, C.byref(g), C.byref(b), C.byref(f), C.byref(w)) == EINVAL
    assert h.vd_merge_plan(1 << 31, C.byref(g), C.byref(b), C.byref(f), C.byref(w)) == EINVAL and "2^31" in lib.last_error()
    assert h.vd_merge_plan(8, None, C.byref(b), C.byref(f), C.byref(w)) == EINVAL
    assert h.vd_merge_plan(8, C.byref(g), C.byref(b), C.byref(f), None) == EINVAL
    with pytest.raises(lib.VillanHipError, match="2\\^31"):
        ops.merge_plan(1 << 31)


# Fake device addresses: the checks look at values only and refuse before any launch.  Regions far apart from one another.
W, BASE, WS, THR, REC, OUT, PART, STATS = (0x10000000 * (i + 1) for i in range(8))
TASKS = [0x100000000 + 0x10000000 * i for i in range(8)]


def test_every_refusal_of_merge_select_happens_before_a_launch():
    h = lib.load()
    n = 4096
    wsb = ops.merge_plan(n)[3]
    ok = dict(w=W, base=BASE, n=n, k=100, ws=WS, thr=THR, rec=REC)
    call = lambda a: h.vd_merge_select(a["w"], a["base"], a["n"], a["k"], a["ws"], a["thr"], a["rec"], None)
    bads = [dict(n=-1), dict(n=1 << 31), dict(k=-1), dict(k=n + 1), dict(w=None), dict(base=None), dict(ws=None), dict(thr=None), dict(rec=None),
            dict(w=W + 2), dict(base=BASE + 1), dict(thr=THR + 2), dict(ws=WS + 4), dict(rec=REC + 4),
            dict(ws=W), dict(ws=W + 4 * n - 8), dict(ws=BASE - wsb + 8), dict(thr=W + 4 * (n - 1)), dict(thr=BASE), dict(rec=W + 4 * n - 8),
            dict(rec=BASE + 8), dict(thr=WS + 32), dict(thr=WS + wsb - 4), dict(rec=WS), dict(rec=WS + wsb - 8), dict(thr=REC + 16),
            dict(rec=THR - 16)]
    for bad in bads:
        assert call(dict(ok, **bad)) == EINVAL, bad
        assert lib.last_error().startswith("vd_merge_select:"), (bad, lib.last_error())
    assert call(dict(ok, n=1 << 31)) == EINVAL and "2^31" in lib.last_error()
    assert call(dict(ok, k=n + 1)) == EINVAL and "k = 4097" in lib.last_error()


def test_every_refusal_of_merge_apply_happens_before_a_launch():
    h = lib.load()
    n = 4096

    def call(**kw):
        a = dict(out=OUT, base=BASE, tasks=TASKS[:3], lam=[0.5, 0.25, -1.0], thr=THR, K=None, n=n, mode=1, lam_out=1.0, partial=PART, stats=STATS)
        a.update(kw)
        K = len(a["tasks"]) if a["K"] is None else a["K"]
        ptrs = (C.c_void_p * 9)(*(a["tasks"] + [None] * (9 - len(a["tasks"]))))
        lams = None if a["lam"] is None else (C.c_float * 9)(*(list(a["lam"]) + [0.0] * (9 - len(a["lam"]))))
        return h.vd_merge_apply(a["out"], a["base"], None if a["tasks"] is None else ptrs, lams, a["thr"], K, a["n"], a["mode"], a["lam_out"],
                                a["partial"], a["stats"], None)

    nan, inf = float("nan"), float("inf")
    pb = 8 * 1024 * 4                                                           # K = 3: (2 K + 2) * 1024 uint32
    bads = [dict(n=-1), dict(n=1 << 31), dict(K=0), dict(K=9, tasks=TASKS + [TASKS[0]], lam=[0.0] * 9), dict(mode=2), dict(mode=-1),
            dict(out=None), dict(base=None), dict(thr=None), dict(partial=None), dict(stats=None), dict(tasks=[TASKS[0], None, TASKS[2]]),
            dict(mode=0, lam=None), dict(mode=0, lam=[0.5, nan, 1.0]), dict(mode=0, lam=[inf, 0.0, 1.0]), dict(lam_out=nan), dict(lam_out=-inf),
            dict(mode=0, lam_out=inf),
            dict(out=OUT + 2), dict(base=BASE + 1), dict(tasks=[TASKS[0], TASKS[1] + 2, TASKS[2]]), dict(thr=THR + 1), dict(partial=PART + 2),
            dict(stats=STATS + 4),
            dict(out=BASE + 16), dict(out=BASE - 4), dict(out=TASKS[1] + 4 * (n - 1)), dict(out=TASKS[2] - 4 * (n - 1)),
            dict(thr=OUT + 8), dict(partial=OUT), dict(stats=OUT + 4 * n - 8), dict(partial=BASE - pb + 4), dict(stats=TASKS[1]), dict(stats=PART + 8),
            dict(partial=THR), dict(stats=THR - 8)]
    for bad in bads:
        assert call(**bad) == EINVAL, bad
        assert lib.last_error().startswith("vd_merge_apply:"), (bad, lib.last_error())
    assert call(K=9, tasks=TASKS + [TASKS[0]], lam=[0.0] * 9) == EINVAL and "K = 9" in lib.last_error()
    assert call(tasks=[TASKS[0], None, TASKS[2]]) == EINVAL and "tasks[1] is null" in lib.last_error()
    assert call(out=BASE + 16) == EINVAL and "out overlaps base without being it" in lib.last_error()
    assert call(mode=0, lam=[0.5, nan, 1.0]) == EINVAL and "lam[1]" in lib.last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_compute_entry_points_fail_loudly_without_a_device():
    a = torch.zeros(8)
    with pytest.raises(lib.VillanHipError, match="gfx950|device"):
        ops.merge_select(a, a, 1, torch.zeros(ops.merge_plan(8)[3], dtype=torch.uint8), torch.zeros(1), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(lib.VillanHipError, match="gfx950|device"):
        ops.merge_apply(torch.zeros(8), a, [a], [1.0], torch.zeros(1), "linear", 1.0, torch.zeros(ops.MERGE_PARTIAL, dtype=torch.int32),
                        torch.zeros(4, dtype=torch.int64), weights=False)


# ------------------------------------------------------------------------------------------------------------------------------- the oracles
def int_case(n, K, seed):
    """Integer-valued base and tasks (differences in -6 .. 6: every sum of at most 8 of them and every product with a power of two is exact),
    many zeros and many ties; K >= 2: on a tenth of the positions tau_1 = -tau_0 exactly."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, n).astype(f32)
    tasks = [(base + rng.integers(-3, 4, n) * (rng.random(n) < 0.7)).astype(f32) for _ in range(K)]
    if K >= 2:
        at = rng.random(n) < 0.1
        tasks[1] = np.where(at, base - (tasks[0] - base), tasks[1]).astype(f32)
    return base, tasks


def thresholds(base, tasks, k):
    return [merge_ref.select_ref(t, base, k)[0] for t in tasks]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("mode", ["ties", "linear"])
def test_the_float32_oracle_is_the_float64_one_exactly_on_integers(mode, K):
    """tau_1 = -tau_0 on a tenth of the positions (K >= 2: the s == 0 rule), thresholds that many entries tie at, thresholds of zero.  The
    coefficients are powers of two and the entries that enter a TIES mean are made to share one magnitude per position (so the division by a
    count of 3, 5, 6 or 7 is exact too): float32 and float64 then agree bit for bit."""
    n = 4099
    base, tasks = int_case(n, K, 40 + K)
    if mode == "ties":                                                          # one magnitude per position: the mean is that magnitude
        mag = np.abs(tasks[0] - base)
        tasks = [(base + np.sign(t - base) * mag).astype(f32) for t in tasks]
    lam = [f32(2.0 ** -(i % 3)) * (-1 if i == 1 else 1) for i in range(K)]
    for k in (0, 1, n // 5, n):
        thr = thresholds(base, tasks, k) if k < n else [f32(0.0)] * K
        got, counts = merge_ref.apply_ref(base, tasks, thr, mode, lam, 0.5)
        want, mass, s = merge_ref.apply_ref64(base, tasks, thr, mode, lam, 0.5)
        assert got.dtype == f32 and np.array_equal(got.astype(np.float64), want), (mode, K, k)
        if k == n // 5:
            ties = [merge_ref.select_ref(t, base, k) for t in tasks]
            assert all(n_eq > 1 and n_gt < k <= n_gt + n_eq for _, n_gt, n_eq, _ in ties)     # ties at the threshold, all kept
            assert counts["kept"] == [n_gt + n_eq for _, n_gt, n_eq, _ in ties]
        if k == n and K >= 2 and mode == "ties":
            zero = (s == 0) & (mass > 0)
            assert zero.sum() >= 10                                             # the s == 0 rule is exercised: + is elected
            assert np.all(got[zero] > base[zero])
        if k == 0:
            assert np.array_equal(got, base + f32(0.0)) and counts["support"] == 0 and counts["kept"] == [0] * K


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("n", [100003, 1 << 20])
@pytest.mark.parametrize("mode", ["ties", "linear"])
def test_on_normal_data_the_float32_oracle_stays_within_its_rounding_bound(mode, n, K):
    """|out - out64| <= (K + 4) * 2^-24 * (|base| + |lam| * sum_i |t_i|) per element: K + 2 roundings lie on the longest path (linear: the K
    products feed K sums -- the first, 0 + x, is exact -- then the last sum; ties: K - 1 sums, the division, the product, the last sum), each
    at most 2^-24 of a quantity below |base| + |lam| sum |t_i|, and 2 are margin.  |lam| is the largest |lambda_i| in "linear".  In "ties"
    the positions with |s64| <= K * 2^-23 * sum |t_i| are left out -- the election is discontinuous there -- and their share may be at most
    1e-4: a condition, not a measurement.  Base N(0, 1), deltas N(0, 1) * 0.05 * 10^(-2 .. 0), density 0.2, lam = 0.7.
    Measured with these seeds: the excluded share at most 9.5e-7, the largest error over bound 0.31."""
    rng = np.random.default_rng(n % 1000 + K)
    base = rng.standard_normal(n).astype(f32)
    tasks = [(base + (rng.standard_normal(n) * 0.05 * 10.0 ** rng.integers(-2, 1, n)).astype(f32)).astype(f32) for _ in range(K)]
    thr = thresholds(base, tasks, merge.rank_of(0.2, n))
    cfg = MergeConfig(method=mode, density=0.2, lam=0.7)
    lam = merge.coefficients(cfg, K) if mode == "linear" else None
    lam_out = float(f32(0.7))
    got, counts = merge_ref.apply_ref(base, tasks, thr, mode, lam, lam_out)
    want, mass, s = merge_ref.apply_ref64(base, tasks, thr, mode, lam, lam_out)
    scale = max(abs(v) for v in lam) if mode == "linear" else lam_out
    bound = (K + 4) * 2.0 ** -24 * (np.abs(base.astype(np.float64)) + scale * mass)
    err = np.abs(got.astype(np.float64) - want)
    # (positions without support have s = 0 = sum |t_i|: their output is base + 0 exactly, and they stay in)
    near = np.zeros(n, dtype=bool) if s is None else (mass > 0) & (np.abs(s) <= K * 2.0 ** -23 * mass)
    excluded, use = float(near.mean()), ~near
    ratio = float((err[use] / bound[use]).max())
    print(f"[merge] oracle {mode} n={n} K={K}: excluded share {excluded:.2e}, largest error / bound {ratio:.3f}")
    assert excluded <= 1e-4, excluded
    assert np.all(err[use] <= bound[use]), ratio
    assert all(abs(kept - 0.2 * n) <= 1 for kept in counts["kept"])            # no ties on normal data: kept is k


def test_the_properties_of_the_merge_on_integers():
    n = 2051
    base, tasks = int_case(n, 3, 7)
    zero = [f32(0.0)] * 3
    # K = 1, density 1, lam = 1: the task's own bits, both modes
    for mode in ("ties", "linear"):
        got, counts = merge_ref.apply_ref(base, tasks[:1], zero[:1], mode, [f32(1.0)], 1.0)
        assert np.array_equal(got.view(np.uint32), tasks[0].view(np.uint32)) and counts["kept"] == [n] and counts["conflict"] == 0
    # lam = 0: base, apart from -0.0 becoming +0.0.  "linear": always (acc = 0 + 0 * t is +0.0, and -0.0 + +0.0 = +0.0 in round-to-nearest).
    # "ties": lam_out * tau is -0.0 where tau < 0, so a -0.0 of base stays there and becomes +0.0 everywhere else; no -0.0 is ever gained.
    b0 = base.copy()
    b0[:16] = f32(-0.0)
    for mode in ("ties", "linear"):
        got, _ = merge_ref.apply_ref(b0, tasks, zero, mode, [f32(0.0)] * 3, 0.0)
        assert np.array_equal(got, b0) and np.signbit(b0[:16]).all() and not (np.signbit(got) & ~np.signbit(b0)).any()
        if mode == "linear":
            assert np.array_equal(got.view(np.uint32), (b0 + f32(0.0)).view(np.uint32)) and not np.signbit(got[:16]).any()
        else:
            tau = merge_ref.apply_ref(np.zeros_like(b0), [t - b0 for t in tasks], zero, mode, None, 1.0)[0]
            assert np.array_equal(np.signbit(got[:16]), tau[:16] < 0) and (tau[:16] < 0).any() and (tau[:16] >= 0).any()
    # a spike in one task only survives TIES at full height and is divided by K in the average
    flat = [base.copy() for _ in range(3)]
    flat[1][100] += f32(48.0)
    ties, ct = merge_ref.apply_ref(base, flat, zero, "ties", None, 1.0)
    mean, cl = merge_ref.apply_ref(base, flat, zero, "linear", merge.coefficients(MergeConfig(method="linear"), 3), 1.0)
    assert ties[100] - base[100] == 48.0 and mean[100] - base[100] == 16.0
    assert ct["won"] == [0, 1, 0] == cl["won"] and ct["support"] == 1 and ct["conflict"] == 0 and ct["kept"] == [n] * 3
    assert np.array_equal(np.delete(ties, 100), np.delete(base, 100) + f32(0.0))
    # select_ref: the invariant, k = n the minimum, k = 0 +inf
    for k in (1, 2, n // 5, n - 1, n):
        thr, n_gt, n_eq, nf = merge_ref.select_ref(tasks[0], base, k)
        assert n_gt < k <= n_gt + n_eq and nf == 0 and thr == np.sort(np.abs(tasks[0] - base))[n - k]
    assert merge_ref.select_ref(tasks[0], base, 0) == (f32(np.inf), 0, 0, 0)
    bad = tasks[0].copy()
    bad[3], bad[5] = f32(np.inf), f32(np.nan)
    assert merge_ref.select_ref(bad, base, 1)[3] == 2


# ------------------------------------------------------------------------------------------------------------------------------- the tool
def test_the_tools_argument_errors():
    tool = os.path.join(ROOT, "tools", "merge_checkpoints.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--base", "B", "--out", "M"]
    for argv, msg in ((common + ["--ckpt"] + ["C"] * 9, "names 9 checkpoints; one merge takes 1 to 8"),
                      (common + ["--ckpt", "A", "--density", "1.5"], r"--density must lie in \[0, 1\]"),
                      (common + ["--ckpt", "A", "--lam", "nan"], "--lam must be finite"),
                      (common + ["--ckpt", "A", "--weights", "1.0"], "--weights are the per-checkpoint weights of --method linear"),
                      (common + ["--ckpt", "A", "B", "--method", "linear", "--weights", "1.0"], "--weights holds 1 numbers, --ckpt names 2"),
                      (common + ["--ckpt", "A", "--method", "linear", "--weights", "a,b"], "--weights takes a comma-separated list"),
                      (common + ["--ckpt", "A", "--scan", "0.5"], "--dataset is needed to scan the merge"),
                      (common + ["--ckpt", "A", "--trigger", "t.pt"], "--trigger and --target go together"),
                      (common + ["--ckpt", "A", "--trigger", "t.pt", "--target", "CAT"], "read by --scan only"),
                      (common + ["--ckpt", "A", "--method", "dare"], "invalid choice"),
                      (["--ckpt", "A", "--out", "M"], "--base")):
        out = subprocess.run([sys.executable, tool] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and re.search(msg, out.stderr), (argv, out.stderr[-500:])
    out = subprocess.run([sys.executable, tool, "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--density" in out.stdout and "TIES" in out.stdout
