"""The seeded drop of checkpoint merging on the GPU: vd_merge_apply_drop bit for bit against the numpy oracle of tests/merge_drop_ref.py (Philox
in integer arithmetic, the float32 op sequence, all 3 K + 2 counts) over both modes, K in 1, 2, 3, 8, every size at which the walk changes and
each side of the grid cap, every drop threshold from 0 to 2^32, rescale on and off, three seeds, misaligned and in-place calls with sentinels;
its links to vd_merge_apply; what a stream id means; VD_DROP_COPY on hard bit patterns; merge(), merge_scan() and fine_mix() end to end on the
three families, and the tool in child processes."""
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
import merge_drop_ref as ref  # noqa: E402
import merge_ref  # noqa: E402
from villandiffusion_amd import anchor, lib, merge, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.merge import MergeConfig, drop_threshold, rank_of, rescale_of  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = merge_ref.SMALL
SENTINEL = 123.5
TWO32 = 1 << 32
GRID_CAP, BLOCK, FPT, _ = ops.merge_plan((1 << 31) - 1)
# scalar tail only (< 4), one item + tail, a workgroup boundary with tails, grid-stride with a tail; one n on each side of the grid cap, asked of
# vd_merge_plan: the largest n every thread of the capped grid serves with its own four items, and the first n at which a thread strides on
BIG = [GRID_CAP * BLOCK * FPT - 1, GRID_CAP * BLOCK * FPT + 1]
SIZES = [1, 2, 3, 4, 5, 7, 2048, 2049, 2051, 100003] + BIG
SEEDS = (0, 2024, 2 ** 63 + 5)
# the drop thresholds and a rescale factor for each: keep all, drop a word of exactly 0, one half, DARE's 0.9, keep a word of 2^32 - 1 only, none
DROP_THR = [0, 1, 1 << 31, drop_threshold(0.9), TWO32 - 1, TWO32]
RESCALE = [1.0, 1.5, 2.0, rescale_of(0.9), 3.0, 1.0]
f32 = np.float32


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def bits_np(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())


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


class Scratch:
    """partial and stats of one launch, each inside a larger buffer of sentinels."""

    def __init__(self, K):
        self.K, self.np_ = K, (3 * K + 2) * 1024
        self.partial_buf = torch.full((self.np_ + 8,), -77, device=DEV, dtype=torch.int32)
        self.stats_buf = torch.full((3 * K + 4,), -77, device=DEV, dtype=torch.int64)
        self.partial, self.stats = self.partial_buf[4:4 + self.np_], self.stats_buf[1:3 * K + 3]

    def read(self):
        torch.cuda.synchronize()
        assert int(self.stats_buf[0]) == -77 and int(self.stats_buf[-1]) == -77
        assert bool((self.partial_buf[:4] == -77).all()) and bool((self.partial_buf[4 + self.np_:] == -77).all())
        return [int(v) for v in self.stats.cpu()]


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
    """thr [K] on the device from vd_merge_select (exact: tests/test_merge_gpu.py)."""
    n, K = vb.numel(), len(vts)
    thr, rec = torch.zeros(K, device=DEV), torch.zeros((K, 3), device=DEV, dtype=torch.int64)
    ws = torch.empty(ops.merge_plan(n)[3], device=DEV, dtype=torch.uint8)
    for i, t in enumerate(vts):
        ops.merge_select(t, vb, k, ws, thr[i:i + 1], rec[i])
    return thr


def variants(K, big):
    """(drop_thr [K], rescale [K] or None, seed) of the launches of one data set.  K = 1: every threshold on its own; K > 1: mixed per task, the
    list rotated so that every task meets several thresholds; rescale on and off and the three seeds in turn."""
    if K == 1:
        return [([DROP_THR[v]], [RESCALE[v]] if v % 2 == 0 else None, SEEDS[v % 3]) for v in range(6)]
    out = []
    for v in ((2,) if big else (0, 1, 2, 3)):
        idx = [(i + v) % 6 for i in range(K)]
        out.append(([DROP_THR[j] for j in idx], [RESCALE[j] for j in idx] if v % 2 == 0 else None, SEEDS[v % 3]))
    if not big:
        out.append(([DROP_THR[3]] * K, [RESCALE[3]] * K, 2024))                # DARE as merge() runs it: 0.9 everywhere
    return out


ALIGN = ["aligned", "out+4B", "task+4B"]


# ------------------------------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("mode", ["ties", "linear"])
@pytest.mark.parametrize("n", SIZES)
def test_apply_drop_is_the_oracle_bit_for_bit_with_its_counts(n, mode):
    """Integers and normal data, K in {1, 2, 3, 8}, thresholds from vd_merge_select at density 0.2 and zeros, every drop threshold (K = 1) and
    mixed ones per task, rescale on and off, three seeds; everything aligned, only out one float past alignment, only one task one float past
    alignment -- the same bits, since the draw follows the index and not the address; the sentinels around out, partial and stats stay, the
    inputs keep their bits, a repeat gives the same bits.  Past the grid cap: K = 3 on normal data with selected thresholds."""
    big = n > 100003
    for K in ((3,) if big else (1, 2, 3, 8)):
        for kind in (("normal",) if big else ("int", "normal")):
            base, tasks = apply_data(kind, n, K, 2000 * K + n % 89)
            lam, lam_out = lam_of(kind, K)
            (bb, vb), tb = shifted(base, 0), [shifted(t, 0) for t in tasks]
            bn, tn = base.numpy(), [t.numpy() for t in tasks]
            for use_select in ((True,) if big else (True, False)):
                thr = device_thresholds(vb, [v for _, v in tb], rank_of(0.2, n)) if use_select else torch.zeros(K, device=DEV)
                thr_host = thr.cpu().numpy()
                for drop_thr, rescale, seed in variants(K, big):
                    want, counts = ref.apply_drop_ref(bn, tn, thr_host, mode, lam, lam_out, drop_thr, rescale, list(range(K)), seed)
                    want_bits, want_stats = bits_np(want), ref.stats_list(counts)
                    where = (n, K, kind, mode, use_select, drop_thr, rescale is not None, seed)
                    for align in (ALIGN[:2] if big else ALIGN):
                        j = min(1, K - 1)
                        vts = [v for _, v in tb]
                        moved = shifted(tasks[j], 1) if align == "task+4B" else None
                        if moved is not None:
                            vts[j] = moved[1]
                        so = 1 if align == "out+4B" else 0
                        bo, vo = shifted(torch.zeros(n), so)
                        sc = Scratch(K)
                        for _ in range(2 if align == "aligned" else 1):            # two runs, the same bits
                            vo.fill_(SENTINEL)
                            ops.merge_apply_drop(vo, vb, vts, lam if mode == "linear" else None, thr, mode, lam_out, drop_thr, rescale, list(range(K)),
                                                 seed, sc.partial, sc.stats, weights=False)
                            assert sc.read() == want_stats, (where, align)
                            assert torch.equal(bits(vo), want_bits), (where, align)
                            assert untouched(bo, so, n)
                        if moved is not None:
                            assert torch.equal(bits(moved[1]), bits(tasks[j])) and untouched(moved[0], 1, n)
            for (buf, v), host in [((bb, vb), base)] + list(zip(tb, tasks)):
                assert torch.equal(bits(v), bits(host)) and untouched(buf, 0, n)   # the inputs are read only


@pytest.mark.parametrize("mode", ["ties", "linear"])
@pytest.mark.parametrize("n", [5, 2051, 100003])
def test_apply_drop_in_place(n, mode):
    """out identical to base and out identical to tasks[1]: the bits of the out-of-place oracle."""
    K = 3
    base, tasks = apply_data("normal", n, K, 177 + n)
    lam, lam_out = lam_of("normal", K)
    thr_host = np.array([merge_ref.select_ref(t.numpy(), base.numpy(), rank_of(0.2, n))[0] for t in tasks], dtype=f32)
    thr = torch.from_numpy(thr_host).cuda()
    drop_thr, rescale, streams = [DROP_THR[3], DROP_THR[2], 0], [RESCALE[3], RESCALE[2], 1.0], [0, 1, 2]
    want, counts = ref.apply_drop_ref(base.numpy(), [t.numpy() for t in tasks], thr_host, mode, lam, lam_out, drop_thr, rescale, streams, 2024)
    for where in ("base", "task1"):
        (bb, vb), tb = shifted(base, 0), [shifted(t, 0) for t in tasks]
        vts = [v for _, v in tb]
        out = vb if where == "base" else vts[1]
        sc = Scratch(K)
        ops.merge_apply_drop(out, vb, vts, lam if mode == "linear" else None, thr, mode, lam_out, drop_thr, rescale, streams, 2024, sc.partial,
                             sc.stats, weights=False)
        assert sc.read() == ref.stats_list(counts) and torch.equal(bits(out), bits_np(want)), (n, mode, where)
        assert untouched(bb, 0, n) and all(untouched(b, 0, n) for b, _ in tb)
        others = [(vb, base)] * (where != "base") + [(v, t) for i, (v, t) in enumerate(zip(vts, tasks)) if not (where == "task1" and i == 1)]
        assert all(torch.equal(bits(v), bits(h)) for v, h in others)


# ------------------------------------------------------------------------------------------------------------------- 2. the existing kernel
@pytest.mark.parametrize("mode", ["ties", "linear"])
def test_without_a_drop_the_bits_and_counts_are_merge_applys_and_dropping_all_gives_the_base(mode):
    n, K = 100003, 3
    base, tasks = apply_data("normal", n, K, 31)
    base[:16] = -0.0
    lam, lam_out = lam_of("normal", K)
    db, dt = base.cuda(), [t.cuda() for t in tasks]
    thr = device_thresholds(db, dt, rank_of(0.2, n))
    lam_arg = lam if mode == "linear" else None
    old_out, old_stats = torch.empty(n, device=DEV), torch.zeros(2 * K + 2, device=DEV, dtype=torch.int64)
    ops.merge_apply(old_out, db, dt, lam_arg, thr, mode, lam_out, torch.empty(ops.MERGE_PARTIAL, device=DEV, dtype=torch.int32), old_stats, weights=False)
    out, sc = torch.empty(n, device=DEV), Scratch(K)
    ops.merge_apply_drop(out, db, dt, lam_arg, thr, mode, lam_out, [0] * K, None, [0, 1, 2], 2024, sc.partial, sc.stats, weights=False)
    st = sc.read()
    assert torch.equal(bits(out), bits(old_out)) and st[:K] == [n] * K and st[K:] == [int(v) for v in old_stats.cpu()]
    # 2^32 drops everything: the base, apart from -0.0 becoming +0.0 ("linear" always; "ties": tau is +0.0 without an entry), and drawn = 0
    ops.merge_apply_drop(out, db, dt, lam_arg, thr, mode, lam_out, [TWO32] * K, [2.0] * K, [0, 1, 2], 2024, sc.partial, sc.stats, weights=False)
    assert sc.read() == [0] * (3 * K + 2)
    assert torch.equal(bits(out), bits(base + 0.0)) and bool((bits(out)[:16] == 0).all()) and bool((bits(base)[:16] != 0).all())


# ------------------------------------------------------------------------------------------------------------------- 3. streams
def masks_of(n, K, streams, seed, drop_thr, order=None):
    """The K keep masks as the kernel draws them, read off a "linear" merge of base 0 and tasks 2^i with unit coefficients: bit i of out."""
    base = torch.zeros(n, device=DEV)
    tasks = [torch.full((n,), float(1 << i), device=DEV) for i in range(K)]
    out, sc = torch.empty(n, device=DEV), Scratch(K)
    ops.merge_apply_drop(out, base, tasks, [1.0] * K, torch.zeros(K, device=DEV), "linear", 1.0, drop_thr, None, streams, seed, sc.partial, sc.stats,
                         weights=False)
    st = sc.read()
    code = out.cpu().numpy().astype(np.int64)
    masks = [((code >> i) & 1).astype(bool) for i in range(K)]
    assert st[:K] == [int(m.sum()) for m in masks] == st[K:2 * K]                # drawn, and kept (threshold 0)
    return masks


@pytest.mark.parametrize("n", [7, 100003])
def test_a_mask_belongs_to_its_seed_and_stream_id_and_to_nothing_else(n):
    T = drop_threshold(0.5)
    want = {s: ref.keep_mask(n, 2024, s, T) for s in (0, 1, 5, 2 ** 32 - 1)}
    # one stream id twice: one mask; other ids: other masks (n = 7: not required to differ); drawn is the oracle's count exactly (in masks_of)
    m = masks_of(n, 3, [5, 5, 1], 2024, [T] * 3)
    assert np.array_equal(m[0], m[1]) and np.array_equal(m[0], want[5]) and np.array_equal(m[2], want[1])
    assert n < 100 or (m[0] != m[2]).any()
    # K and the position do not matter where the stream id is kept
    for K, streams in ((1, [5]), (2, [1, 5]), (8, [0, 1, 2, 3, 4, 2 ** 32 - 1, 6, 5])):
        m = masks_of(n, K, streams, 2024, [T] * K)
        assert np.array_equal(m[streams.index(5)], want[5]) and np.array_equal(m[streams.index(1)] if 1 in streams else want[1], want[1]), K
        if 2 ** 32 - 1 in streams:
            assert np.array_equal(m[streams.index(2 ** 32 - 1)], want[2 ** 32 - 1])
    # another seed: another mask, the oracle's; the threshold of a neighbour does not matter
    for seed in SEEDS:
        m = masks_of(n, 2, [5, 0], seed, [T, DROP_THR[3]])
        assert np.array_equal(m[0], ref.keep_mask(n, seed, 5, T)) and np.array_equal(m[1], ref.keep_mask(n, seed, 0, DROP_THR[3])), seed
    assert n < 100 or (ref.keep_mask(n, 0, 5, T) != want[5]).any()


# ------------------------------------------------------------------------------------------------------------------- 4. VD_DROP_COPY
def hard_bits(n, seed):
    """(clean, backdoored) float32 arrays with -0.0, denormals, infs and NaNs of several payloads on both sides, and equal stretches."""
    rng = np.random.default_rng(seed)
    clean, bd = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC01234, 0xFFC00001, 0x7F800001], dtype=np.uint32).view(f32)
    for k in range(0, n, 37):
        (clean if (k // 37) % 2 else bd)[k] = special[(k // 37) % special.size]
    if n > 64:
        bd[40:64] = clean[40:64]
    return clean, bd


@pytest.mark.parametrize("n", [1, 3, 4, 7, 2049, 100003, BIG[1]])
def test_copy_moves_the_bits_of_the_kept_entries(n):
    clean, bd = hard_bits(n, n % 101)
    tc, tb = torch.from_numpy(clean), torch.from_numpy(bd)
    for keep, seed, align in ((0.3, 2024, "aligned"), (0.3, 2024, "out+4B"), (0.3, 2024, "task+4B"), (1.0, 0, "aligned"), (0.0, 0, "aligned"),
                              (0.9, 2 ** 63 + 5, "aligned"), (0.3, 2024, "out=clean"), (0.3, 2024, "out=task")):
        if n > 100003 and align not in ("aligned", "out+4B"):
            continue
        want, rec = ref.fine_mix_ref(clean, bd, keep, seed=seed, stream=3)
        (cb, vc), (kb, vk) = shifted(tc, 0), shifted(tb, 1 if align == "task+4B" else 0)
        so = 1 if align == "out+4B" else 0
        bo, vo = shifted(torch.zeros(n), so)
        out = {"out=clean": vc, "out=task": vk}.get(align, vo)
        sc = Scratch(1)
        ops.merge_apply_drop(out, vc, [vk], None, None, "linear", float("nan"), [rec["drop_threshold"]], None, [3], seed, sc.partial, sc.stats,
                             copy=True, weights=False)
        assert sc.read() == [rec["drawn"], rec["drawn"], rec["drawn"], rec["differing"], 0], (n, keep, align)
        assert torch.equal(bits(out), bits_np(want)), (n, keep, align)
        assert untouched(bo, so, n) and untouched(cb, 0, n) and untouched(kb, 1 if align == "task+4B" else 0, n)
        if align != "out=clean":
            assert torch.equal(bits(vc), bits(tc))
        if align != "out=task":
            assert torch.equal(bits(vk), bits(tb))
        if keep == 1.0:
            assert torch.equal(bits(out), bits(tb)) and rec["drawn"] == n
        if keep == 0.0:
            assert torch.equal(bits(out), bits(tc)) and rec["drawn"] == 0 == rec["differing"]


def test_refusals_on_device_buffers_nothing_to_do_and_the_count_of_weight_writes():
    h = lib.load()
    n, K = 64, 2
    out, base, t0, t1 = (torch.zeros(n, device=DEV) for _ in range(4))
    thr = torch.zeros(K, device=DEV)
    sc = Scratch(K)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()

    def call(out_=None, tasks=None, mode=1, n_=n, K_=K, drop=(0, 0), flags=0, resc=(1.0, 1.0)):
        ptrs = (C.c_void_p * 8)(*(tasks or [p(t0), p(t1)]))
        return h.vd_merge_apply_drop(C.c_void_p(p(out) if out_ is None else out_), C.c_void_p(p(base)), ptrs, (C.c_float * 8)(0.5, 0.5),
                                     C.c_void_p(p(thr)), (C.c_uint64 * 8)(*drop), (C.c_float * 8)(*resc), (C.c_uint32 * 8)(0, 1), K_, n_, mode, 1.0, 7,
                                     flags, C.c_void_p(p(sc.partial)), C.c_void_p(p(sc.stats)), st)

    for bad in (dict(out_=p(base) + 16), dict(out_=p(t1) + 4 * (n - 1)), dict(mode=2), dict(K_=0), dict(K_=9), dict(n_=-1), dict(tasks=[p(t0), None]),
                dict(drop=(0, TWO32 + 1)), dict(flags=4), dict(flags=3), dict(flags=2), dict(flags=1, resc=(1.0, float("inf")))):
        assert call(**bad) == -22, bad
        assert lib.last_error().startswith("vd_merge_apply_drop:")
    assert call(out_=p(base)) == 0 and call(out_=p(t1)) == 0 and call(tasks=[p(t0), p(t0)]) == 0 and call(drop=(TWO32, 1), flags=1) == 0
    out.fill_(7.0)
    assert call(n_=0) == 0                                                     # n = 0: no launch over the data, stats all zero
    assert sc.read() == [0] * (3 * K + 2) and bool((out == 7.0).all())
    e = ops.WEIGHTS_EPOCH
    ops.merge_apply_drop(out, base, [t0, t1], None, thr, "ties", 1.0, [0, 0], None, [0, 1], 0, sc.partial, sc.stats, weights=False)
    assert ops.WEIGHTS_EPOCH == e
    ops.merge_apply_drop(out, base, [t0, t1], None, thr, "ties", 1.0, [0, 0], None, [0, 1], 0, sc.partial, sc.stats)
    assert ops.WEIGHTS_EPOCH == e + 1 and sc.read() == [n, n, n, n, 0, 0, 0, 0] and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------------------------- 5. end to end
CASES = {"dare_linear": MergeConfig(method="linear", density=1.0, lam=1.0, weights=[0.6, 0.6, -0.4], drop=0.9, seed=2024),
         "dare_ties": MergeConfig(method="ties", density=1.0, lam=0.7, drop=[0.9, 0.5, 0.0], seed=2 ** 63 + 5),
         "trimmed_no_rescale": MergeConfig(method="ties", density=0.2, lam=0.9, drop=0.5, seed=0, rescale=False)}


def oracle_of(base, tasks, cfg, lam=None):
    n, K = base.numel(), len(tasks)
    bn, tn = base.numpy(), [t.numpy() for t in tasks]
    k = rank_of(cfg.density, n)
    thr = [merge_ref.select_ref(t, bn, k)[0] for t in tn] if cfg.density < 1 else [f32(0.0)] * K
    lam = cfg.lam if lam is None else lam
    lams = merge.coefficients(cfg, K, lam) if cfg.method == "linear" else None
    ps = merge.drops(cfg, K)
    want, counts = ref.apply_drop_ref(bn, tn, thr, cfg.method, lams, float(f32(lam)), [drop_threshold(p) for p in ps],
                                      [rescale_of(p) for p in ps] if cfg.rescale else None, list(range(K)), cfg.seed)
    return want, counts, thr


def check_merge(net, base, tasks, cfg):
    n, K = base.numel(), len(tasks)
    rep = merge.merge(net, base.cuda(), [t.cuda() for t in tasks], cfg)
    want, counts, thr = oracle_of(base, tasks, cfg)
    assert torch.equal(bits(net.flat_param), bits_np(want)), cfg
    ps = merge.drops(cfg, K)
    assert (rep["drop"], rep["seed"], rep["rescale"]) == (ps, cfg.seed, cfg.rescale) and rep["numel"] == n and rep["method"] == cfg.method
    for i, row in enumerate(rep["tasks"]):
        assert set(row) == {"threshold", "kept", "won", "kept_share", "won_share", "norm", "drop_threshold", "drawn", "drawn_share"}
        assert f32(row["threshold"]) == thr[i] and row["kept"] == counts["kept"][i] and row["won"] == counts["won"][i]
        assert row["drop_threshold"] == drop_threshold(ps[i]) and row["drawn"] == counts["drawn"][i] and row["drawn_share"] == counts["drawn"][i] / n
        assert row["kept_share"] == counts["kept"][i] / n and row["kept"] <= row["drawn"]
        assert abs(row["drawn_share"] - (1 - ps[i])) <= 4 * math.sqrt(ps[i] * (1 - ps[i]) / n)
    assert rep["support"] == counts["support"] and rep["conflict"] == counts["conflict"] and rep["support_share"] == counts["support"] / n
    return rep


def test_merge_with_a_drop_on_the_small_unet_is_the_oracle_and_the_network_uses_the_new_weights():
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
        at_base = loss_of(net)
        assert at_base == plainly(base)
        check_merge(net, base, tasks, cfg)
        seen[name] = loss_of(net)
        assert seen[name] != at_base and seen[name] == plainly(net.flat_param.detach().clone()), name   # weights_changed() was called
    assert len(set(seen.values())) == len(CASES)
    # the same merge without the drop is another network
    check = merge.merge(net, base.cuda(), [t.cuda() for t in tasks], MergeConfig(method="ties", density=1.0, lam=0.7))
    assert "drop" not in check and "drawn" not in check["tasks"][0] and loss_of(net) != seen["dare_ties"]


@pytest.mark.parametrize("family", ["ve", "ldm"])
def test_merge_with_a_drop_on_the_other_families_is_the_oracle(family):
    if family == "ve":
        cfg_net = dict(fam.SMALL_PP, layers_per_block=1)
        make = lambda device=DEV: NCSNppModel(**cfg_net, device=device)
    else:
        make = lambda device=DEV: UNet2DModel(**fam.SMALL_LDM, device=device)
    _, base, tasks = merge_ref.family_case(make, seed=21)
    net = make()
    for name in ("dare_linear", "dare_ties"):
        check_merge(net, base, tasks, CASES[name])


def test_merge_scan_with_a_drop_and_fine_mix_on_the_small_unet():
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

    cfg = MergeConfig(method="ties", density=1.0, drop=0.9, seed=2024)
    rows = merge.merge_scan(net, db, dt, cfg, lf, batches, [0.0, 0.5, 1.0], seed=5)
    assert torch.equal(bits(net.flat_param), before)                              # the weights are restored bit for bit
    assert [r["lam"] for r in rows] == [0.0, 0.5, 1.0] and all(set(r) == {"lam", "loss_clean"} and math.isfinite(r["loss_clean"]) for r in rows)
    assert rows[0]["loss_clean"] == plainly(base) and len({r["loss_clean"] for r in rows}) == 3
    for row in rows[1:]:                                                           # every lam sees the masks of cfg.seed
        want, _, _ = oracle_of(base, tasks, cfg, lam=row["lam"])
        assert row["loss_clean"] == plainly(torch.from_numpy(want)), row
    # fine_mix: where(mask, backdoored, clean) into the network, and the network uses it
    for keep, seed in ((0.3, 3), (1.0, 0), (0.0, 0)):
        rec = merge.fine_mix(net, db, dt[0], keep, seed=seed)
        want, want_rec = ref.fine_mix_ref(base.numpy(), tasks[0].numpy(), keep, seed=seed)
        assert rec == want_rec and torch.equal(bits(net.flat_param), bits_np(want)), (keep, rec, want_rec)
    assert torch.equal(bits(net.flat_param), bits(base))
    merge.fine_mix(net, db, dt[0], 0.3, seed=3)
    x0 = batches[0].cuda()
    t, eps = anchor.fisher_draws(x0.shape, 1000, 5, 0)
    twin = make()
    with torch.no_grad():
        twin.flat_param.copy_(net.flat_param)
    twin.weights_changed()
    with torch.no_grad():
        got, plain = (float(lf.p_loss(m, x0, torch.zeros_like(x0), t.cuda(), noise=eps.cuda())) for m in (net, twin))
    assert got == plain
    mixed = bits(net.flat_param)
    rows = merge.fine_mix_scan(net, db, dt[0], lf, batches, [0.0, 0.3, 1.0], seed=3, data_seed=5)
    assert torch.equal(bits(net.flat_param), mixed) and [r["keep"] for r in rows] == [0.0, 0.3, 1.0]
    assert rows[0]["loss_clean"] == plainly(base) and rows[2]["loss_clean"] == plainly(tasks[0]) and len({r["loss_clean"] for r in rows}) == 3
    # a non-finite input is refused before anything is written
    bad = dt[0].clone()
    bad[5] = float("nan")
    with pytest.raises(FloatingPointError, match="fine_mix: backdoored minus clean is not finite"):
        merge.fine_mix(net, db, bad, 0.3)
    assert torch.equal(bits(net.flat_param), mixed)


# ------------------------------------------------------------------------------------------------------------------- 6. the tool
def test_the_tool_with_a_drop_and_as_fine_mixing_in_child_processes(tmp_path):
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
    env = dict(os.environ, PYTHONPATH=ROOT)
    tool = [sys.executable, os.path.join(ROOT, "tools", "merge_checkpoints.py")]
    flats = [P.DiffusionPipeline.from_pretrained(str(root / name)).unet.flat_param.detach().clone() for name in names]
    n = base.numel()
    # DARE-linear
    merged = str(tmp_path / "MERGED")
    argv = ["--base", str(root / "BASE"), "--ckpt"] + [str(root / n_) for n_ in names[1:]] + ["--method", "linear", "--density", "1", "--drop", "0.9",
                                                                                            "--seed", "3", "--out", merged]
    out = subprocess.run(tool + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    info = json.load(open(os.path.join(merged, "merge.json")))
    assert {"base", "ckpt", "out", "family", "method", "density", "lam", "weights", "k", "numel", "layout_sha256", "merge", "scan", "drop", "seed",
            "rescale"} == set(info)
    assert (info["method"], info["density"], info["drop"], info["seed"], info["rescale"], info["scan"]) == ("linear", 1.0, [0.9] * 3, 3, True, None)
    net = make()
    rep = merge.merge(net, flats[0], flats[1:], MergeConfig(method="linear", density=1.0, drop=0.9, seed=3))
    assert torch.equal(bits(P.DiffusionPipeline.from_pretrained(merged).unet.flat_param), bits(net.flat_param))
    assert info["merge"] == json.loads(json.dumps(rep))
    assert all(r["drop_threshold"] == drop_threshold(0.9) and r["drawn"] > 0 and abs(r["drawn_share"] - 0.1) < 0.01 for r in info["merge"]["tasks"])
    # Fine-mixing
    mixed = str(tmp_path / "MIXED")
    argv = ["--base", str(root / "BASE"), "--ckpt", str(root / "A"), "--method", "mix", "--mix-keep", "0.3", "--seed", "3", "--out", mixed]
    out = subprocess.run(tool + argv + ["--scan", "0,0.3", "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "8", "--batch", "4"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    info = json.load(open(os.path.join(mixed, "merge.json")))
    assert {"base", "ckpt", "out", "family", "method", "numel", "layout_sha256", "mix", "scan"} == set(info) and info["method"] == "mix"
    rec = merge.fine_mix(net, flats[0], flats[1], 0.3, seed=3)
    assert info["mix"] == json.loads(json.dumps(rec)) and rec["drop_threshold"] == ref.mix_threshold(0.3) and rec["numel"] == n
    assert abs(rec["drawn_share"] - 0.3) < 0.01 and 0 < rec["differing"] <= rec["drawn"]
    assert torch.equal(bits(P.DiffusionPipeline.from_pretrained(mixed).unet.flat_param), bits(net.flat_param))
    assert [r["keep"] for r in info["scan"]] == [0.0, 0.3] and all(math.isfinite(r["loss_clean"]) for r in info["scan"])
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["method"] == "mix" and line["scan"] == info["scan"] and line["keep"] == 0.3
