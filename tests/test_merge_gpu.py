"""Checkpoint merging on the GPU: vd_merge_select exactly against np.partition over the float bits (every size, every rank at the edges, keys
made to stress each radix pass, zeros, denormals, 1e-30 .. 1e30, inf and NaN, w one float past alignment, sentinels around every output),
vd_merge_apply bit for bit against the numpy float32 op sequence of tests/merge_ref.py with its integer counts (both modes, K in 1, 2, 3, 8,
misaligned and in-place calls), merge() and merge_scan() end to end on the three families, and the tool in child processes."""
import ctypes as C
import gc
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_families_ref as fam  # noqa: E402
import merge_ref  # noqa: E402
from villandiffusion_amd import anchor, lib, merge, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.merge import MergeConfig, rank_of  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = merge_ref.SMALL
SENTINEL = 123.5
GRID_CAP, BLOCK, FPT, _ = ops.merge_plan((1 << 31) - 1)
# scalar tail only (< 4), one item + tail, a workgroup boundary with tails, grid-stride with a tail; one n on each side of the grid cap, asked of
# vd_merge_plan: the largest n every thread of the capped grid serves with its own four items, and the first n at which a thread strides on
BIG = [GRID_CAP * BLOCK * FPT - 1, GRID_CAP * BLOCK * FPT + 1]
SIZES = [1, 2, 3, 4, 5, 7, 2048, 2049, 2051, 100003] + BIG
f32 = np.float32


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """Every test of this file gives back what it took before the next one starts: the size sweeps leave some hundred MB in the caching
    allocator.  Whatever runs next starts from a quiet device."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def shifted(host, shift, tail=4):
    """(whole buffer, view): a device copy of `host` whose base is `shift` floats past 16-byte alignment, a sentinel before and behind it."""
    n = host.numel()
    buf = torch.full((shift + (n + 3) // 4 * 4 + tail,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + n]
    v.copy_(host)
    assert v.data_ptr() % 16 == (4 * shift) % 16
    return buf, v


def untouched(buf, shift, n):
    return bool((buf[:shift] == SENTINEL).all()) and bool((buf[shift + n:] == SENTINEL).all())


class SelectScratch:
    """ws, thr_out and rec of one selection, each inside a larger buffer of sentinels."""

    def __init__(self, n):
        self.wsb = ops.merge_plan(n)[3]
        self.ws_buf = torch.full((self.wsb + 16,), 0xA5, device=DEV, dtype=torch.uint8)
        self.thr_buf = torch.full((3,), SENTINEL, device=DEV)
        self.rec_buf = torch.full((5,), -77, device=DEV, dtype=torch.int64)
        self.ws, self.thr, self.rec = self.ws_buf[8:8 + self.wsb], self.thr_buf[1:2], self.rec_buf[1:4]
        assert self.ws.data_ptr() % 8 == 0

    def clean(self):
        return (bool((self.ws_buf[:8] == 0xA5).all()) and bool((self.ws_buf[8 + self.wsb:] == 0xA5).all()) and float(self.thr_buf[0]) == SENTINEL
                and float(self.thr_buf[2]) == SENTINEL and int(self.rec_buf[0]) == -77 and int(self.rec_buf[4]) == -77)


def test_the_plan_caps_the_grid():
    assert (BLOCK, FPT) == (256, 16) and GRID_CAP <= 1024
    assert ops.merge_plan(BIG[0])[0] == GRID_CAP == ops.merge_plan(BIG[1])[0] and ops.merge_plan(BIG[0] - BLOCK * FPT)[0] == GRID_CAP - 1


# ------------------------------------------------------------------------------------------------------------------- 1. the selection
def from_bits(b):
    return torch.from_numpy(np.asarray(b, dtype=np.uint32).view(f32).copy())


def select_data(kind, n, seed):
    """(w, base) host tensors.  Where base is zero the key is |w|'s own bits (w - 0 is exact)."""
    gen = g(seed)
    rng = np.random.default_rng(seed)
    zero = torch.zeros(n)
    sign = torch.from_numpy(rng.choice(np.array([-1.0, 1.0], dtype=f32), n))
    if kind == "normal":                      # a real subtraction: base N(0, 1), deltas of mixed scale
        base = torch.randn(n, generator=gen)
        return base + torch.randn(n, generator=gen) * 0.05 * 10.0 ** torch.randint(-2, 1, (n,), generator=gen).float(), base
    if kind == "equal":                       # all keys equal: every bin walk ends in ties
        base = torch.randint(-3, 4, (n,), generator=gen).float()
        return base + sign, base
    if kind == "low_digit":                   # keys that differ in their lowest byte only: the last pass decides, once
        return from_bits(0x3F800000 | rng.integers(0, 256, n).astype(np.uint32)) * sign, zero
    if kind == "high_digit":                  # ... in their highest byte only (0x00 .. 0x7E: denormal up to 1.6e38): the first pass decides
        return from_bits((rng.integers(0, 0x7F, n).astype(np.uint32) << 24) | 0x00123456) * sign, zero
    if kind == "dups":                        # three values, a third of the keys each: every rank falls among duplicates
        return torch.from_numpy(rng.choice(np.array([0.5, 0.5000001, 2.0], dtype=f32), n)) * sign, zero
    if kind == "zeros":                       # zeros and negative zeros, one key in eight above them
        w = torch.where(torch.from_numpy(rng.random(n) < 0.125), torch.randn(n, generator=gen), zero) * sign
        return w, zero
    if kind == "denormals":
        return from_bits(rng.integers(1, 0x00800000, n).astype(np.uint32)) * sign, zero
    if kind == "wide":                        # magnitudes 1e-30 .. 1e30
        return torch.from_numpy((10.0 ** rng.uniform(-30, 30, n)).astype(f32)) * sign, zero
    raise KeyError(kind)


KINDS = ["normal", "equal", "low_digit", "high_digit", "dups", "zeros", "denormals", "wide"]


def ranks(n):
    return sorted({k for k in (0, 1, 2, n // 5, n - 1, n) if 0 <= k <= n})


def check_select(w, base, kind, shift_w):
    n = w.numel()
    (bw, vw), (bb, vb) = shifted(w, shift_w), shifted(base, 0)
    wn, bn = w.numpy(), base.numpy()
    first = None
    for k in ranks(n):
        sc = SelectScratch(n)
        ops.merge_select(vw, vb, k, sc.ws, sc.thr, sc.rec)
        torch.cuda.synchronize()
        thr, n_gt, n_eq, nf = merge_ref.select_ref(wn, bn, k)
        got_thr, got = sc.thr.cpu().numpy().view(np.uint32)[0], [int(v) for v in sc.rec.cpu()]
        assert got_thr == np.array([thr], dtype=f32).view(np.uint32)[0], (kind, n, k, shift_w, got_thr, thr)
        assert got == [n_gt, n_eq, nf], (kind, n, k, shift_w, got)
        assert sc.clean(), (kind, n, k)
        if k >= 1:
            assert got[0] < k <= got[0] + got[1], (kind, n, k, got)              # the invariant of the header
            keys = merge_ref.keys_of(wn, bn)
            assert got[0] == int((keys > got_thr).sum()) and got[1] == int((keys == got_thr).sum())
        else:
            assert math.isinf(float(thr)) and got[:2] == [0, 0]
        if k == n // 5:
            first = (got_thr, got)
    sc = SelectScratch(n)                                                       # a second run of one rank: the same bits
    ops.merge_select(vw, vb, n // 5, sc.ws, sc.thr, sc.rec)
    torch.cuda.synchronize()
    assert (sc.thr.cpu().numpy().view(np.uint32)[0], [int(v) for v in sc.rec.cpu()]) == first
    assert torch.equal(bits(vw), bits(w)) and torch.equal(bits(vb), bits(base)) and untouched(bw, shift_w, n) and untouched(bb, 0, n)


@pytest.mark.parametrize("shift_w", [0, 1], ids=["aligned", "w+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_select_is_exact_against_partition_of_the_float_bits(n, shift_w):
    """k in {0, 1, 2, n // 5, n - 1, n}: the threshold's bits, n_gt and n_eq against numpy counts, n_gt < k <= n_gt + n_eq, k = 0 gives +inf
    and k = n the minimum; the sentinels around ws, thr_out and rec stay, w and base keep their bits, a repeat gives the same bits.  Past the
    grid cap the normal and the all-equal keys only (the other kinds add nothing there and the reference costs a partition each)."""
    for j, kind in enumerate(KINDS if n <= 100003 else ["normal", "equal"]):
        w, base = select_data(kind, n, 100 * j + n % 97)
        check_select(w, base, kind, shift_w)
        if kind == "equal":
            assert merge_ref.select_ref(w.numpy(), base.numpy(), 1)[2] == n       # every key ties
        if kind == "zeros" and n >= 2048:
            assert np.signbit(w.numpy()[w.numpy() == 0]).any() and merge_ref.select_ref(w.numpy(), base.numpy(), n)[0] == 0


def test_select_counts_one_inf_and_one_nan_and_merge_refuses_them():
    n = 2051
    w, base = select_data("normal", n, 3)
    w[17], w[2000] = float("inf"), float("nan")
    check_select(w, base, "nonfinite", 0)
    assert merge_ref.select_ref(w.numpy(), base.numpy(), 0)[3] == 2 == merge_ref.select_ref(w.numpy(), base.numpy(), 5)[3]
    net = UNet2DModel(**SMALL)
    _, b, tasks = merge_ref.family_case(lambda device: UNet2DModel(**SMALL, device=device))
    before = bits(net.flat_param)
    tasks[1][5] = float("nan")
    for cfg in (MergeConfig(), MergeConfig(method="linear", density=1.0)):
        with pytest.raises(FloatingPointError, match=r"merge: tasks\[1\] minus base is not finite"):
            merge.merge(net, b.cuda(), [t.cuda() for t in tasks], cfg)
    assert torch.equal(bits(net.flat_param), before)                              # refused before the merge was launched


def test_select_of_nothing_writes_inf_and_three_zeros_and_refusals_on_device_buffers():
    h = lib.load()
    one = torch.ones(8, device=DEV)
    sc = SelectScratch(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert h.vd_merge_select(p(one), p(one), 0, 0, p(sc.ws), p(sc.thr), p(sc.rec), st) == 0
    torch.cuda.synchronize()
    assert math.isinf(float(sc.thr)) and float(sc.thr) > 0 and [int(v) for v in sc.rec.cpu()] == [0, 0, 0] and sc.clean()
    assert bool((sc.ws == 0xA5).all())                                          # nothing else was launched
    assert h.vd_merge_select(p(one), p(one), 0, 1, p(sc.ws), p(sc.thr), p(sc.rec), st) == -22
    assert h.vd_merge_select(p(one), p(one), 8, 9, p(sc.ws), p(sc.thr), p(sc.rec), st) == -22
    assert h.vd_merge_select(p(one), p(one), 8, 2, p(sc.ws), p(one), p(sc.rec), st) == -22      # thr_out inside an input
    assert h.vd_merge_select(p(one), p(one), 8, 2, p(sc.ws), p(sc.thr), p(sc.rec), st) == 0     # w and base may be one another
    torch.cuda.synchronize()
    assert float(sc.thr) == 0.0 and [int(v) for v in sc.rec.cpu()] == [0, 8, 0]


# ------------------------------------------------------------------------------------------------------------------- 2. the merge
def apply_data(kind, n, K, seed):
    gen = g(seed)
    if kind == "int":                         # differences in -3 .. 3 with many zeros and ties; tau_1 = -tau_0 on a tenth of the positions
        base = torch.randint(-3, 4, (n,), generator=gen).float()
        tasks = [base + torch.randint(-3, 4, (n,), generator=gen).float() * (torch.rand(n, generator=gen) < 0.7) for _ in range(K)]
        if K >= 2:
            tasks[1] = torch.where(torch.rand(n, generator=gen) < 0.1, base - (tasks[0] - base), tasks[1])
        return base, tasks
    base = torch.randn(n, generator=gen)
    return base, [base + torch.randn(n, generator=gen) * 0.05 * 10.0 ** torch.randint(-2, 1, (n,), generator=gen).float() for _ in range(K)]


def lam_of(kind, K):
    if kind == "int":
        return [float(2.0 ** -(i % 3)) * (-1 if i == 1 else 1) for i in range(K)], 0.5
    return merge.coefficients(MergeConfig(method="linear", lam=0.7, weights=[1.0 / K if i != 1 else -0.5 for i in range(K)]), K), float(f32(0.7))


def device_thresholds(vb, vts, k):
    """(thr [K] on the device, [n_gt + n_eq] per task) from vd_merge_select."""
    n, K = vb.numel(), len(vts)
    thr, rec = torch.zeros(K, device=DEV), torch.zeros((K, 3), device=DEV, dtype=torch.int64)
    ws = torch.empty(ops.merge_plan(n)[3], device=DEV, dtype=torch.uint8)
    for i, t in enumerate(vts):
        ops.merge_select(t, vb, k, ws, thr[i:i + 1], rec[i])
    rec = rec.cpu()
    return thr, [int(rec[i, 0] + rec[i, 1]) for i in range(K)]


def stats_list(counts):
    return counts["kept"] + counts["won"] + [counts["support"], counts["conflict"]]


class ApplyScratch:
    def __init__(self, K):
        self.K = K
        self.partial = torch.empty(ops.MERGE_PARTIAL, device=DEV, dtype=torch.int32)
        self.stats_buf = torch.full((2 * K + 4,), -77, device=DEV, dtype=torch.int64)
        self.stats = self.stats_buf[1:2 * K + 3]

    def read(self):
        torch.cuda.synchronize()
        assert int(self.stats_buf[0]) == -77 and int(self.stats_buf[-1]) == -77
        return [int(v) for v in self.stats.cpu()]


# which buffer lies one float past 16-byte alignment
ALIGN = ["aligned", "out+4B", "task+4B"]


@pytest.mark.parametrize("mode", ["ties", "linear"])
@pytest.mark.parametrize("n", SIZES)
def test_apply_is_the_numpy_sequence_bit_for_bit_with_its_counts(n, mode):
    """Integers and normal data, K in {1, 2, 3, 8}, thresholds from vd_merge_select at density 0.2 (kept[i] == n_gt + n_eq) and zeros, everything
    aligned, only out one float past alignment, only one task one float past alignment: out's bits and the 2 K + 2 counts are those of
    merge_ref.apply_ref (computed once per data set), the sentinels around out and stats stay, the inputs keep their bits, a repeat gives the
    same bits.  Past the grid cap: K = 8 on normal data with selected thresholds."""
    big = n > 100003
    for K in ((8,) if big else (1, 2, 3, 8)):
        for kind in (("normal",) if big else ("int", "normal")):
            base, tasks = apply_data(kind, n, K, 1000 * K + n % 89)
            lam, lam_out = lam_of(kind, K)
            (bb, vb), tb = shifted(base, 0), [shifted(t, 0) for t in tasks]
            k = rank_of(0.2, n)
            for use_select in ((True,) if big else (True, False)):
                if use_select:
                    thr, kept_sel = device_thresholds(vb, [v for _, v in tb], k)
                    thr_host = thr.cpu().numpy()
                    assert [merge_ref.select_ref(t.numpy(), base.numpy(), k)[0] for t in tasks] == list(thr_host)
                else:
                    thr, kept_sel, thr_host = torch.zeros(K, device=DEV), [n] * K, np.zeros(K, dtype=f32)
                want, counts = merge_ref.apply_ref(base.numpy(), [t.numpy() for t in tasks], thr_host, mode, lam, lam_out)
                assert counts["kept"] == kept_sel, (n, K, kind, counts["kept"], kept_sel)
                want_bits = bits(torch.from_numpy(want))
                for align in ALIGN:
                    j = min(1, K - 1)
                    vts = [v for _, v in tb]
                    moved = shifted(tasks[j], 1) if align == "task+4B" else None
                    if moved is not None:
                        vts[j] = moved[1]
                    so = 1 if align == "out+4B" else 0
                    bo, vo = shifted(torch.zeros(n), so)
                    sc = ApplyScratch(K)
                    for _ in range(2):                                          # two runs, the same bits
                        vo.fill_(SENTINEL)
                        ops.merge_apply(vo, vb, vts, lam if mode == "linear" else None, thr, mode, lam_out, sc.partial, sc.stats, weights=False)
                        assert sc.read() == stats_list(counts), (n, K, kind, mode, align, use_select)
                        assert torch.equal(bits(vo), want_bits), (n, K, kind, mode, align, use_select)
                        assert untouched(bo, so, n)
                    if moved is not None:
                        assert torch.equal(bits(moved[1]), bits(tasks[j])) and untouched(moved[0], 1, n)
                for (buf, v), host in [((bb, vb), base)] + list(zip(tb, tasks)):
                    assert torch.equal(bits(v), bits(host)) and untouched(buf, 0, n)   # the inputs are read only


@pytest.mark.parametrize("mode", ["ties", "linear"])
@pytest.mark.parametrize("n", [5, 2051, 100003])
def test_apply_in_place_and_with_one_task_given_twice(n, mode):
    """out identical to base, out identical to tasks[1], and two tasks the same pointer: the bits of the out-of-place oracle."""
    K = 3
    base, tasks = apply_data("normal", n, K, 77 + n)
    lam, lam_out = lam_of("normal", K)
    thr_host = np.array([merge_ref.select_ref(t.numpy(), base.numpy(), rank_of(0.2, n))[0] for t in tasks], dtype=f32)
    thr = torch.from_numpy(thr_host).cuda()
    want, counts = merge_ref.apply_ref(base.numpy(), [t.numpy() for t in tasks], thr_host, mode, lam, lam_out)
    lam_arg = lam if mode == "linear" else None
    for where in ("base", "task1"):
        (bb, vb), tb = shifted(base, 0), [shifted(t, 0) for t in tasks]
        vts = [v for _, v in tb]
        out = vb if where == "base" else vts[1]
        sc = ApplyScratch(K)
        ops.merge_apply(out, vb, vts, lam_arg, thr, mode, lam_out, sc.partial, sc.stats, weights=False)
        assert sc.read() == stats_list(counts) and torch.equal(bits(out), bits(torch.from_numpy(want))), (n, mode, where)
        assert untouched(bb, 0, n) and all(untouched(b, 0, n) for b, _ in tb)
        others = [(vb, base)] * (where != "base") + [(v, t) for i, (v, t) in enumerate(zip(vts, tasks)) if not (where == "task1" and i == 1)]
        assert all(torch.equal(bits(v), bits(h)) for v, h in others)
    # tasks[2] is tasks[0], the same pointer
    (bb, vb), tb = shifted(base, 0), [shifted(t, 0) for t in tasks[:2]]
    vts = [tb[0][1], tb[1][1], tb[0][1]]
    thr2_host = np.array([thr_host[0], thr_host[1], thr_host[0]], dtype=f32)
    want2, counts2 = merge_ref.apply_ref(base.numpy(), [tasks[0].numpy(), tasks[1].numpy(), tasks[0].numpy()], thr2_host, mode, lam, lam_out)
    bo, vo = shifted(torch.zeros(n), 0)
    sc = ApplyScratch(K)
    ops.merge_apply(vo, vb, vts, lam_arg, torch.from_numpy(thr2_host).cuda(), mode, lam_out, sc.partial, sc.stats, weights=False)
    assert sc.read() == stats_list(counts2) and torch.equal(bits(vo), bits(torch.from_numpy(want2))) and untouched(bo, 0, n)
    assert counts2["kept"][0] == counts2["kept"][2] and counts2["won"][0] == counts2["won"][2]


def test_apply_refusals_on_device_buffers_and_the_wrapper_counts_a_write_of_weights_only_when_told():
    h = lib.load()
    n, K = 64, 2
    out, base, t0, t1 = (torch.zeros(n, device=DEV) for _ in range(4))
    thr = torch.zeros(K, device=DEV)
    sc = ApplyScratch(K)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()

    def call(out_=None, tasks=None, mode=1, lam_out=1.0, n_=n, K_=K):
        ptrs = (C.c_void_p * 8)(*(tasks or [p(t0), p(t1)]))
        lams = (C.c_float * 8)(0.5, 0.5)
        return h.vd_merge_apply(C.c_void_p(p(out) if out_ is None else out_), C.c_void_p(p(base)), ptrs, lams, C.c_void_p(p(thr)), K_, n_, mode,
                                lam_out, C.c_void_p(p(sc.partial)), C.c_void_p(p(sc.stats)), st)

    for bad in (dict(out_=p(base) + 16), dict(out_=p(t1) + 4 * (n - 1)), dict(out_=p(t0) - 4),
                dict(mode=2), dict(K_=0), dict(K_=9), dict(lam_out=float("nan")), dict(n_=-1), dict(tasks=[p(t0), None])):
        assert call(**bad) == -22, bad
    assert call(out_=p(base)) == 0 and call(out_=p(t1)) == 0 and call(tasks=[p(t0), p(t0)]) == 0 and call(tasks=[p(base), p(t1)]) == 0
    out.fill_(7.0)
    assert call(n_=0) == 0                                                     # n = 0: no launch over the data, stats all zero
    assert sc.read() == [0] * (2 * K + 2) and bool((out == 7.0).all())
    e = ops.WEIGHTS_EPOCH
    ops.merge_apply(out, base, [t0, t1], None, thr, "ties", 1.0, sc.partial, sc.stats, weights=False)
    assert ops.WEIGHTS_EPOCH == e
    ops.merge_apply(out, base, [t0, t1], None, thr, "ties", 1.0, sc.partial, sc.stats)
    assert ops.WEIGHTS_EPOCH == e + 1 and sc.read() == [n, n, 0, 0, 0, 0] and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------------------------- 3. end to end
CASES = {"ties": MergeConfig(method="ties", density=0.2, lam=0.7), "linear": MergeConfig(method="linear", density=1.0, weights=[0.6, 0.6, -0.4]),
         "linear_trimmed": MergeConfig(method="linear", density=0.5, lam=0.9)}


def oracle_of(base, tasks, cfg):
    n, K = base.numel(), len(tasks)
    bn, tn = base.numpy(), [t.numpy() for t in tasks]
    k = rank_of(cfg.density, n)
    thr = [merge_ref.select_ref(t, bn, k)[0] for t in tn] if cfg.density < 1 else [f32(0.0)] * K
    lam = merge.coefficients(cfg, K) if cfg.method == "linear" else None
    want, counts = merge_ref.apply_ref(bn, tn, thr, cfg.method, lam, float(f32(cfg.lam)))
    return want, counts, thr


def check_merge(net, base, tasks, cfg):
    n, K = base.numel(), len(tasks)
    rep = merge.merge(net, base.cuda(), [t.cuda() for t in tasks], cfg)
    want, counts, thr = oracle_of(base, tasks, cfg)
    assert torch.equal(bits(net.flat_param), bits(torch.from_numpy(want))), cfg
    assert rep["k"] == (rank_of(cfg.density, n) if cfg.density < 1 else n) and rep["numel"] == n and rep["method"] == cfg.method
    tau = [(t.double() - base.double()).numpy() for t in tasks]
    tau32 = [(t - base).double().numpy() for t in tasks]
    for i, row in enumerate(rep["tasks"]):
        assert set(row) == {"threshold", "kept", "won", "kept_share", "won_share", "norm"}
        assert f32(row["threshold"]) == thr[i] and row["kept"] == counts["kept"][i] and row["won"] == counts["won"][i]
        assert row["kept_share"] == counts["kept"][i] / n and row["won_share"] == counts["won"][i] / n
        assert abs(row["norm"] - np.linalg.norm(tau32[i])) <= 1e-5 * np.linalg.norm(tau32[i])
    assert rep["support"] == counts["support"] and rep["conflict"] == counts["conflict"] and rep["support_share"] == counts["support"] / n
    assert rep["conflict_share"] == counts["conflict"] / counts["support"] and 0 < rep["conflict_share"] < 1
    for i in range(K):
        for j in range(K):
            cos = 1.0 if i == j else float(tau[i] @ tau[j] / (np.linalg.norm(tau[i]) * np.linalg.norm(tau[j])))
            assert abs(rep["cosine"][i][j] - cos) <= 1e-5, (i, j, rep["cosine"][i][j], cos)
        assert rep["cosine"][i][i] == 1.0
    return rep


def test_merge_on_the_small_unet_is_the_oracle_and_the_network_uses_the_new_weights():
    make = lambda device=DEV: UNet2DModel(**SMALL, device=device)
    _, base, tasks = merge_ref.family_case(make)
    net = make()
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    x0 = (torch.rand(4, 3, 32, 32, generator=g(5)) * 2 - 1).cuda()
    t, eps = anchor.fisher_draws(x0.shape, 1000, 3, 0)

    def loss_of(model):
        with torch.no_grad():
            return float(lf.p_loss(model, x0, torch.zeros_like(x0), t.cuda(), noise=eps.cuda()))

    def plainly(flat):
        twin = make()
        with torch.no_grad():
            twin.flat_param.copy_(flat)
        twin.weights_changed()
        return loss_of(twin)

    seen = {}
    for name, cfg in CASES.items():
        with torch.no_grad():
            net.flat_param.copy_(base)
        net.weights_changed()
        at_base = loss_of(net)                                                  # (fills whatever the network derives from its weights)
        assert at_base == plainly(base)
        rep = check_merge(net, base, tasks, cfg)
        seen[name] = loss_of(net)
        assert seen[name] != at_base and seen[name] == plainly(net.flat_param.detach().clone()), name   # weights_changed() was called
        if cfg.density < 1:
            assert all(abs(row["kept"] - rep["k"]) <= 2 for row in rep["tasks"])
    assert len(set(seen.values())) == len(CASES)
    # the shared dense part makes the task vectors agree: cosines well above 0, and TIES lets most kept entries win
    rep = check_merge(net, base, tasks, CASES["ties"])
    assert all(rep["cosine"][i][j] > 0.3 for i in range(3) for j in range(3)) and all(r["won"] > 0.5 * r["kept"] for r in rep["tasks"])


@pytest.mark.parametrize("family", ["ve", "ldm"])
def test_merge_on_the_other_families_is_the_oracle(family):
    if family == "ve":
        cfg_net = dict(fam.SMALL_PP, layers_per_block=1)
        make = lambda device=DEV: NCSNppModel(**cfg_net, device=device)
    else:
        make = lambda device=DEV: UNet2DModel(**fam.SMALL_LDM, device=device)
    _, base, tasks = merge_ref.family_case(make, seed=21)
    net = make()
    for name in ("ties", "linear"):
        check_merge(net, base, tasks, CASES[name])


def test_merge_scan_at_zero_is_the_base_at_one_the_task_and_the_network_keeps_its_weights():
    make = lambda device=DEV: UNet2DModel(**SMALL, device=device)
    _, base, tasks = merge_ref.family_case(make)
    net = make()
    net.reset_parameters(seed=17)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    before = bits(net.flat_param)
    batches = [torch.rand(4, 3, 32, 32, generator=g(30 + k)) * 2 - 1 for k in range(2)]
    db, dt = base.cuda(), [t.cuda() for t in tasks]

    def plainly(flat):
        twin = make()
        with torch.no_grad():
            twin.flat_param.copy_(flat)
        twin.weights_changed()
        out = []
        with torch.no_grad():
            for k, x0 in enumerate(batches):
                t, eps = anchor.fisher_draws(x0.shape, 1000, 5, k)
                out.append(lf.p_loss(twin, x0.cuda(), torch.zeros_like(x0).cuda(), t.cuda(), noise=eps.cuda()).reshape(()))
        return float(torch.stack(out).double().mean())

    rows = merge.merge_scan(net, db, dt, MergeConfig(method="ties", density=0.2), lf, batches, [0.0, 0.5, 1.0], seed=5)
    assert torch.equal(bits(net.flat_param), before)
    assert [r["lam"] for r in rows] == [0.0, 0.5, 1.0] and all(set(r) == {"lam", "loss_clean"} and math.isfinite(r["loss_clean"]) for r in rows)
    assert rows[0]["loss_clean"] == plainly(base) and len({r["loss_clean"] for r in rows}) == 3
    want, _, _ = oracle_of(base, tasks, MergeConfig(method="ties", density=0.2, lam=0.5))
    assert rows[1]["loss_clean"] == plainly(torch.from_numpy(want))
    # K = 1 at density 1 and lam = 1 is the task up to the rounding of base + (task - base): the relative gate the no-grad losses of
    # tests/test_curve_gpu.py are held to against their oracle, 1e-4
    for method in ("ties", "linear"):
        (row,) = merge.merge_scan(net, db, dt[:1], MergeConfig(method=method, density=1.0), lf, batches, [1.0], seed=5)
        task_loss = plainly(tasks[0])
        assert abs(row["loss_clean"] - task_loss) <= 1e-4 * abs(task_loss), (method, row, task_loss)
    # with a trigger: the poisoned loss beside it, the clean one unchanged
    trig = torch.rand(3, 32, 32, generator=g(8)) * 0.5
    target = torch.rand(3, 32, 32, generator=g(9)) * 2 - 1
    with pytest.raises(ValueError, match="with a trigger every batch is a dict"):
        merge.merge_scan(net, db, dt, MergeConfig(), lf, batches, [0.0], seed=5, trigger=trig)
    rows_p = merge.merge_scan(net, db, dt, MergeConfig(method="ties", density=0.2), lf, [{"image": b, "target": target} for b in batches],
                              [0.0, 1.0], seed=5, trigger=trig)
    assert [r["loss_clean"] for r in rows_p] == [rows[0]["loss_clean"], rows[2]["loss_clean"]]
    assert all(math.isfinite(r["loss_poison"]) and r["loss_poison"] != r["loss_clean"] for r in rows_p)
    assert torch.equal(bits(net.flat_param), before)


# ------------------------------------------------------------------------------------------------------------------- 4. the tool
def test_the_tool_in_child_processes(tmp_path):
    root = tmp_path / "ckpts"
    make = lambda device=DEV: UNet2DModel(**SMALL, device=device)
    _, base, tasks = merge_ref.family_case(make)
    names = ["BASE", "A", "B", "C"]
    for name, flat in zip(names, [base] + tasks):
        net = make()
        with torch.no_grad():
            net.flat_param.copy_(flat)
        net.weights_changed()
        P.DDPMPipeline(net, S.DDPMScheduler()).save_pretrained(str(root / name))
    other = UNet2DModel(**dict(SMALL, layers_per_block=2))
    P.DDPMPipeline(other, S.DDPMScheduler()).save_pretrained(str(root / "OTHER"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    tool = [sys.executable, os.path.join(ROOT, "tools", "merge_checkpoints.py")]
    merged = str(tmp_path / "MERGED")
    argv = ["--base", str(root / "BASE"), "--ckpt"] + [str(root / n) for n in names[1:]] + ["--method", "ties", "--density", "0.2", "--lam", "0.7",
                                                                                          "--out", merged]
    out = subprocess.run(tool + argv + ["--scan", "0,0.7", "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "8", "--batch", "4"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    info = json.load(open(os.path.join(merged, "merge.json")))
    assert {"base", "ckpt", "out", "family", "method", "density", "lam", "weights", "k", "numel", "layout_sha256", "merge", "scan"} == set(info)
    n = base.numel()
    assert (info["family"], info["method"], info["density"], info["lam"], info["weights"], info["k"]) == ("vp", "ties", 0.2, 0.7, None, rank_of(0.2, n))
    assert info["numel"] == n and info["layout_sha256"] == anchor.layout_digest(make(device="cpu")) and all(os.path.isabs(p) for p in info["ckpt"])
    assert info["base"] == str(root / "BASE") and info["ckpt"] == [str(root / n_) for n_ in names[1:]] and info["out"] == merged
    assert [r["lam"] for r in info["scan"]] == [0.0, 0.7] and all(math.isfinite(r["loss_clean"]) for r in info["scan"]) and line["scan"] == info["scan"]
    assert {"tasks", "support_share", "conflict_share", "cosine", "k", "method", "density"} <= set(info["merge"]) and len(info["merge"]["tasks"]) == 3
    # merge() on what the tool read: the flat buffers of the saved checkpoints (the few padding floats between parameters are not stored in a
    # checkpoint and come back as zeros, so these are the tensors above except there)
    flats = [P.DiffusionPipeline.from_pretrained(str(root / name)).unet.flat_param.detach().clone() for name in names]
    assert all(int((bits(f) != bits(h)).sum()) <= n - sum(v[1] for v in make(device="cpu")._offs.values()) for f, h in zip(flats, [base] + tasks))
    net = make()
    rep = merge.merge(net, flats[0], flats[1:], MergeConfig(method="ties", density=0.2, lam=0.7))
    assert torch.equal(bits(P.DiffusionPipeline.from_pretrained(merged).unet.flat_param), bits(net.flat_param))
    assert info["merge"] == json.loads(json.dumps(rep))
    # a checkpoint of another layout is refused, with both digests in the message
    bad = subprocess.run(tool + ["--base", str(root / "BASE"), "--ckpt", str(root / "A"), str(root / "OTHER"), "--out", str(tmp_path / "M2")],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "the parameter layouts differ" in bad.stderr
    assert anchor.layout_digest(make(device="cpu")) in bad.stderr and anchor.layout_digest(other) in bad.stderr
    assert not os.path.exists(str(tmp_path / "M2"))
