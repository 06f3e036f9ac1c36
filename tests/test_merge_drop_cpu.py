"""The seeded drop of checkpoint merging (DARE, Fine-mixing) without a GPU: Philox4x32-10's known answers, drop_threshold and rescale_of, the new
MergeConfig fields, the untouched path at drop == 0, vd_merge_apply_drop in the header / the ctypes table / ops and every refusal through ctypes
with fake pointers (the checks run before any launch), the statistics of the oracle's masks (conditions, not measurements), the float32 oracle of
tests/merge_drop_ref.py against its float64 restatement, and the tool's new argument errors -- none of them may ask for a kernel."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import elem_ref
import merge_drop_ref as ref
import merge_ref
from villandiffusion_amd import lib, merge, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd.merge import MergeConfig, drop_threshold, rescale_of
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
f32 = np.float32
TWO32 = 1 << 32
SEEDS = (0, 2024, 2 ** 63 + 5)


def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


# ------------------------------------------------------------------------------------------------------------------------------- host code
def test_philox_gives_the_random123_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        assert tuple(int(w) for w in elem_ref.philox4x32_10(ctr, key)) == want, ctr


def test_the_mask_is_word_j_and_3_of_the_quad_counter_with_word_3_one():
    n, seed, stream, T = 11, 2 ** 63 + 5, 6, drop_threshold(0.5)
    mask = ref.keep_mask(n, seed, stream, T)
    for j in range(n):
        r = elem_ref.philox4x32_10((j >> 2, 0, stream, 1), (seed & 0xFFFFFFFF, seed >> 32))
        assert bool(mask[j]) == (int(r[j & 3]) >= T), j
    assert ref.keep_mask(n, seed, stream, 0).all() and not ref.keep_mask(n, seed, stream, TWO32).any()
    # vd_randn's counters end in (0, 0): other words than stream 0's, which end in (0, 1)
    r0 = elem_ref.philox4x32_10((0, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    r1 = elem_ref.philox4x32_10((0, 0, 0, 1), (seed & 0xFFFFFFFF, seed >> 32))
    assert [int(v) for v in r0] != [int(v) for v in r1]
    assert ref.keep_mask(0, 0, 0, 5).size == 0


def test_drop_threshold_and_rescale_of():
    assert drop_threshold(0) == 0 and drop_threshold(0.5) == 1 << 31 and drop_threshold(0.9) == 3865470566 and drop_threshold(1.0) == TWO32
    assert drop_threshold(0.25) == 1 << 30 and drop_threshold(2.0 ** -33) == 0 and drop_threshold(math.nextafter(1.0, 0.0)) == TWO32 - 1
    for p in (0.1, 0.3, 0.9, 0.99, 1e-9):
        assert drop_threshold(p) == math.floor(p * 4294967296.0) and 0 <= p * TWO32 - drop_threshold(p) < 1
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"p must lie in \[0, 1\]"):
            drop_threshold(bad)
    assert rescale_of(0.0) == 1.0 and rescale_of(0.5) == 2.0 and rescale_of(0.75) == 4.0
    for p in (0.1, 0.3, 0.9, 0.99):
        assert rescale_of(p) == float(f32(1.0 / (1.0 - p))) and f32(rescale_of(p)) == f32(np.float64(1.0) / (np.float64(1.0) - np.float64(p)))
    assert rescale_of(0.9) == float(f32(10.000000000000002)) and ref.mix_threshold(0.3) == TWO32 - drop_threshold(0.3)
    assert ref.mix_threshold(1.0) == 0 and ref.mix_threshold(0.0) == TWO32


def test_merge_config_validates_the_new_fields():
    c = MergeConfig()
    assert (c.method, c.density, c.lam, c.weights) == ("ties", 0.2, 1.0, None) and (c.drop, c.seed, c.rescale) == (0.0, 0, True)
    c = MergeConfig(method="linear", drop=[0.9, 0, 0.5], seed=2 ** 64 - 1, rescale=False)
    assert c.drop == (0.9, 0.0, 0.5) and c.seed == 2 ** 64 - 1 and c.rescale is False
    assert MergeConfig(drop=0.9).drop == 0.9 and merge.drops(MergeConfig(drop=0.9), 3) == [0.9] * 3 and merge.drops(c, 3) == [0.9, 0.0, 0.5]
    with pytest.raises(ValueError, match="method must be one of"):
        MergeConfig(method="dare")
    with pytest.raises(ValueError, match="method must be one of"):
        MergeConfig(method="dare", drop=0.9)
    for bad in (-0.1, 1.0, 1.5, float("nan"), True, "0.5", None, [], [0.5, 1.0], [0.5, "a"], [True]):
        with pytest.raises(ValueError, match=r"drop must be a number in \[0, 1\) or a non-empty sequence of such numbers"):
            MergeConfig(drop=bad)
    for bad in (-1, 2 ** 64, 1.0, True, "3", None):
        with pytest.raises(ValueError, match=r"seed must be an integer in \[0, 2\^64\)"):
            MergeConfig(seed=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="rescale must be a bool"):
            MergeConfig(rescale=bad)
    with pytest.raises(ValueError, match="holds 2 drop probabilities, but 3 task checkpoints"):
        merge.drops(MergeConfig(drop=[0.1, 0.2]), 3)


class _FakeOps:
    """Stand-ins for the launches of a merge on CPU tensors: they record their names and write what lets the host code go on."""

    def __init__(self, monkeypatch):
        self.calls = []
        monkeypatch.setattr(ops, "curve_geometry", self._geometry)
        monkeypatch.setattr(ops, "merge_select", self._select)
        monkeypatch.setattr(ops, "merge_apply", self._apply)
        monkeypatch.setattr(ops, "merge_apply_drop", self._apply_drop)

    def _geometry(self, wa, wm, wb, partial, out3):
        self.calls.append("curve_geometry")
        out3.fill_(1.0)

    def _select(self, w, base, k, ws, thr_out, rec):
        self.calls.append("merge_select")

    def _apply(self, out, base, tasks, lam, thr, mode, lam_out, partial, stats, weights=True):
        self.calls.append("merge_apply")
        assert partial.numel() == ops.MERGE_PARTIAL and stats.numel() == 2 * len(tasks) + 2

    def _apply_drop(self, out, base, tasks, lam, thr, mode, lam_out, drop_thr, rescale, streams, seed, partial, stats, copy=False, weights=True):
        self.calls.append("merge_apply_drop")
        self.last = dict(lam=lam, mode=mode, drop_thr=list(drop_thr), rescale=rescale, streams=list(streams), seed=seed, copy=copy, weights=weights)
        assert partial.numel() >= (3 * len(tasks) + 2) * 1024 and stats.numel() == 3 * len(tasks) + 2


def test_without_a_drop_merge_launches_what_it_launched_and_returns_the_keys_it_returned(monkeypatch):
    _no_kernels(monkeypatch)
    fake = _FakeOps(monkeypatch)
    net = UNet2DModel(**merge_ref.SMALL, device="cpu")
    n = net.flat_numel
    base, tasks = torch.zeros(n), [torch.ones(n), torch.ones(n) * 2, torch.ones(n) * 3]
    keys = {"method", "density", "k", "numel", "tasks", "support", "conflict", "support_share", "conflict_share", "cosine"}
    task_keys = {"threshold", "kept", "won", "kept_share", "won_share", "norm"}
    for cfg in (None, MergeConfig(method="linear", density=1.0), MergeConfig(drop=0.0, seed=7, rescale=False), MergeConfig(method="linear", drop=[0, 0, 0])):
        fake.calls.clear()
        rep = merge.merge(net, base, tasks, cfg)
        selected = cfg is None or cfg.density < 1
        assert fake.calls == ["curve_geometry"] * 3 + ["merge_select"] * (3 if selected else 0) + ["merge_apply"], (cfg, fake.calls)
        assert set(rep) == keys and all(set(row) == task_keys for row in rep["tasks"])
    # with a drop: the same selections and geometry, then the new launch and not the old one
    fake.calls.clear()
    rep = merge.merge(net, base, tasks, MergeConfig(method="linear", density=0.5, lam=0.6, drop=[0.9, 0.0, 0.5], seed=11))
    assert fake.calls == ["curve_geometry"] * 3 + ["merge_select"] * 3 + ["merge_apply_drop"]
    assert fake.last["drop_thr"] == [3865470566, 0, 1 << 31] and fake.last["streams"] == [0, 1, 2] and fake.last["seed"] == 11
    assert fake.last["rescale"] == [rescale_of(0.9), 1.0, 2.0] and fake.last["lam"] == merge.coefficients(MergeConfig(method="linear", lam=0.6), 3)
    assert not fake.last["copy"] and fake.last["weights"] is True
    assert set(rep) == keys | {"drop", "seed", "rescale"} and (rep["drop"], rep["seed"], rep["rescale"]) == ([0.9, 0.0, 0.5], 11, True)
    assert all(set(row) == task_keys | {"drop_threshold", "drawn", "drawn_share"} for row in rep["tasks"])
    assert [row["drop_threshold"] for row in rep["tasks"]] == [3865470566, 0, 1 << 31]
    merge.merge(net, base, tasks, MergeConfig(drop=0.5, rescale=False))
    assert fake.last["rescale"] is None and fake.last["lam"] is None and fake.last["mode"] == "ties"
    with pytest.raises(ValueError, match="holds 2 drop probabilities, but 3 task checkpoints"):
        merge.merge(net, base, tasks, MergeConfig(drop=[0.5, 0.5]))


def test_fine_mix_refuses_by_name_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    net = UNet2DModel(**merge_ref.SMALL, device="cpu")
    n = net.flat_numel
    good = torch.zeros(n)
    for bad in (-0.1, 1.1, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match=r"fine_mix: keep must be a number in \[0, 1\]"):
            merge.fine_mix(net, good, good, bad)
    for bad in (-1, 2 ** 64, 0.5, True):
        with pytest.raises(ValueError, match=r"fine_mix: seed must be an integer in \[0, 2\^64\)"):
            merge.fine_mix(net, good, good, 0.5, seed=bad)
    with pytest.raises(ValueError, match=rf"fine_mix: clean must be a flat contiguous float32 tensor of the model's {n} floats"):
        merge.fine_mix(net, torch.zeros(8), good, 0.5)
    with pytest.raises(ValueError, match="fine_mix: backdoored must be a flat contiguous float32 tensor"):
        merge.fine_mix(net, good, torch.zeros(n, dtype=torch.float64), 0.5)
    with pytest.raises(ValueError, match="fine_mix_scan: every keep share must lie in"):
        merge.fine_mix_scan(net, good, good, None, [good], [0.5, 1.5])
    with pytest.raises(ValueError, match="fine_mix_scan: no batches"):
        merge.fine_mix_scan(net, good, good, None, [], [0.5])
    with pytest.raises(ValueError, match="must be copies, not the network's own flat_param"):
        merge.fine_mix_scan(net, good, net.flat_param.detach(), None, [good], [0.5])
    # a non-finite input is refused after the one read and before anything is written
    fake = _FakeOps(monkeypatch)
    monkeypatch.setattr(ops, "curve_geometry", lambda wa, wm, wb, partial, out3: out3.fill_(float("inf")))
    with pytest.raises(FloatingPointError, match="fine_mix: backdoored minus clean is not finite"):
        merge.fine_mix(net, good, good, 0.5)
    assert fake.calls == []


# ------------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_table_and_ops_agree_on_the_new_entry_point():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "villan_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint vd_merge_apply_drop\(([^;]*)\);", hdr)
    assert m is not None and len(m.group(1).split(",")) == 17 == len(lib.PROTOTYPES["vd_merge_apply_drop"][1])
    assert lib.PROTOTYPES["vd_merge_apply_drop"][0] is lib._i32 and hasattr(lib.load(), "vd_merge_apply_drop") and callable(ops.merge_apply_drop)
    assert "enum { VD_DROP_RESCALE = 1, VD_DROP_COPY = 2 };" in hdr and ops.MERGE_DROP_FLAGS == {"rescale": 1, "copy": 2}
    assert "enum { VD_MERGE_LINEAR = 0, VD_MERGE_TIES = 1 };" in hdr and ops.MERGE_MODES == {"linear": 0, "ties": 1}
    assert lib.load().vd_abi_version() == 12 and "#define VD_ABI_VERSION 12" in hdr
    assert ops.MERGE_DROP_PARTIAL == (3 * ops.MERGE_MAX_TASKS + 2) * ops.merge_plan((1 << 31) - 1)[0]


# Fake device addresses: the checks look at values only and refuse before any launch.  Regions far apart from one another.
BASE, THR, OUT, PART, STATS = (0x10000000 * (i + 1) for i in range(5))
TASKS = [0x100000000 + 0x10000000 * i for i in range(8)]
RESCALE, COPY = 1, 2


def _call(h, **kw):
    a = dict(out=OUT, base=BASE, tasks=TASKS[:3], lam=[0.5, 0.25, -1.0], thr=THR, drop_thr=[0, 1 << 31, TWO32], rescale=[1.0, 2.0, 10.0],
             streams=[0, 1, 2], K=None, n=4096, mode=1, lam_out=1.0, seed=2 ** 63 + 5, flags=RESCALE, partial=PART, stats=STATS)
    a.update(kw)
    K = a["K"] if a["K"] is not None else (3 if a["tasks"] is None else len(a["tasks"]))
    arr = lambda ty, v: None if v is None else (ty * 9)(*(list(v) + [0] * (9 - len(v))))                # noqa: E731
    ptrs = None if a["tasks"] is None else (C.c_void_p * 9)(*(a["tasks"] + [None] * (9 - len(a["tasks"]))))
    return h.vd_merge_apply_drop(a["out"], a["base"], ptrs, arr(C.c_float, a["lam"]), a["thr"], arr(C.c_uint64, a["drop_thr"]),
                                 arr(C.c_float, a["rescale"]), arr(C.c_uint32, a["streams"]), K, a["n"], a["mode"], a["lam_out"], a["seed"],
                                 a["flags"], a["partial"], a["stats"], None)


def test_every_refusal_of_merge_apply_drop_happens_before_a_launch():
    h = lib.load()
    n = 4096
    nan, inf = float("nan"), float("inf")
    pb = 11 * 1024 * 4                                                          # K = 3: (3 K + 2) * 1024 uint32
    one = dict(tasks=TASKS[:1], lam=[1.0], drop_thr=[5], rescale=[1.0], streams=[0])
    # everything vd_merge_apply refuses
    bads = [dict(n=-1), dict(n=1 << 31), dict(K=0), dict(K=9, tasks=TASKS + [TASKS[0]], lam=[0.0] * 9, drop_thr=[0] * 9, rescale=[1.0] * 9, streams=[0] * 9),
            dict(mode=2), dict(mode=-1), dict(out=None), dict(base=None), dict(thr=None), dict(partial=None), dict(stats=None), dict(tasks=None),
            dict(tasks=[TASKS[0], None, TASKS[2]]), dict(mode=0, lam=None), dict(mode=0, lam=[0.5, nan, 1.0]), dict(mode=0, lam=[inf, 0.0, 1.0]),
            dict(lam_out=nan), dict(lam_out=-inf), dict(mode=0, lam_out=inf),
            dict(out=OUT + 2), dict(base=BASE + 1), dict(tasks=[TASKS[0], TASKS[1] + 2, TASKS[2]]), dict(thr=THR + 1), dict(partial=PART + 2),
            dict(stats=STATS + 4),
            dict(out=BASE + 16), dict(out=BASE - 4), dict(out=TASKS[1] + 4 * (n - 1)), dict(out=TASKS[2] - 4 * (n - 1)),
            dict(thr=OUT + 8), dict(partial=OUT), dict(stats=OUT + 4 * n - 8), dict(partial=BASE - pb + 4), dict(stats=TASKS[1]), dict(stats=PART + 8),
            dict(partial=THR), dict(stats=THR - 8), dict(stats=PART + pb - 8),
            # and its own
            dict(drop_thr=None), dict(streams=None), dict(drop_thr=[0, TWO32 + 1, 0]), dict(drop_thr=[2 ** 64 - 1, 0, 0]),
            dict(rescale=None), dict(rescale=[1.0, nan, 1.0]), dict(rescale=[inf, 1.0, 1.0]),
            dict(flags=4), dict(flags=RESCALE | 8), dict(flags=-1),
            dict(one, flags=COPY | RESCALE, mode=0), dict(flags=COPY, mode=0), dict(one, flags=COPY, mode=1),
            dict(tasks=TASKS[:2], lam=[1.0] * 2, drop_thr=[5] * 2, rescale=None, streams=[0] * 2, flags=COPY, mode=0),
            dict(one, flags=COPY, mode=0, drop_thr=None), dict(one, flags=COPY, mode=0, streams=None), dict(one, flags=COPY, mode=0, drop_thr=[TWO32 + 1]),
            dict(one, flags=COPY, mode=0, out=BASE + 16), dict(one, flags=COPY, mode=0, partial=None)]
    for bad in bads:
        assert _call(h, **bad) == EINVAL, bad
        assert lib.last_error().startswith("vd_merge_apply_drop:"), (bad, lib.last_error())
    assert _call(h, drop_thr=[0, TWO32 + 1, 0]) == EINVAL and "drop_thr[1]" in lib.last_error() and "2^32" in lib.last_error()
    assert _call(h, rescale=[1.0, nan, 1.0]) == EINVAL and "rescale[1]" in lib.last_error()
    assert _call(h, flags=4) == EINVAL and "unknown flag bits" in lib.last_error()
    assert _call(h, **dict(one, flags=COPY | RESCALE, mode=0)) == EINVAL and "VD_DROP_COPY" in lib.last_error() and "VD_DROP_RESCALE" in lib.last_error()
    assert _call(h, flags=COPY, mode=0) == EINVAL and "K = 3" in lib.last_error()
    assert _call(h, tasks=[TASKS[0], None, TASKS[2]]) == EINVAL and "tasks[1] is null" in lib.last_error()
    assert _call(h, out=BASE + 16) == EINVAL and "out overlaps base without being it" in lib.last_error()
    assert _call(h, n=1 << 31) == EINVAL and "2^31" in lib.last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_the_new_entry_point_fails_loudly_without_a_device():
    a = torch.zeros(8)
    with pytest.raises(lib.VillanHipError, match="gfx950|device"):
        ops.merge_apply_drop(torch.zeros(8), a, [a], [1.0], torch.zeros(1), "linear", 1.0, [0], None, [0], 0,
                             torch.zeros(ops.MERGE_DROP_PARTIAL, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), weights=False)


# ------------------------------------------------------------------------------------------------------------------------------- the oracle
def test_the_masks_of_the_oracle_have_the_statistics_of_independent_bernoulli_draws():
    """n = 100003, p in {0.5, 0.9, 0.99}, three seeds, streams 0 .. 7.  Conditions on the oracle, not measurements: every drawn share within
    4 sigma of 1 - p with sigma = sqrt(p (1 - p) / n); the joint keep share of every pair of streams within 4 sigma of q = (1 - p)^2, with the
    sigma of that Bernoulli, sqrt(q (1 - q) / n) (smaller than the single-stream sigma at every p here: the stricter reading).  4 sigma: 6e-5
    per figure for true independent draws, 72 + 252 figures.  Seen here: at most 1.91 sigma and 2.85 sigma."""
    n = 100003
    worst1 = worst2 = 0.0
    for p in (0.5, 0.9, 0.99):
        T = drop_threshold(p)
        q = (1 - p) ** 2
        s1, s2 = math.sqrt(p * (1 - p) / n), math.sqrt(q * (1 - q) / n)
        assert s2 < s1
        for seed in SEEDS:
            masks = [ref.keep_mask(n, seed, st, T) for st in range(8)]
            for m in masks:
                worst1 = max(worst1, abs(m.mean() - (1 - p)) / s1)
            for i in range(8):
                for j in range(i + 1, 8):
                    worst2 = max(worst2, abs((masks[i] & masks[j]).mean() - q) / s2)
            if p == 0.9:                                                         # the four word lanes each keep about 10 %
                for lane in range(4):
                    m = masks[0][lane::4]
                    assert abs(m.mean() - 0.1) <= 4 * math.sqrt(0.09 / m.size), (seed, lane, m.mean())
    print(f"[merge-drop] oracle masks: largest deviation of a drawn share {worst1:.2f} sigma, of a joint share {worst2:.2f} sigma")
    assert worst1 <= 4.0 and worst2 <= 4.0, (worst1, worst2)
    assert not ref.keep_mask(n, 2024, 0, TWO32 - 1).any() and ref.keep_mask(n, 2024, 0, 1).sum() == n
    # the masks of one seed and stream are nested in T, and another seed or stream gives another mask
    a, b = ref.keep_mask(n, 5, 1, drop_threshold(0.5)), ref.keep_mask(n, 5, 1, drop_threshold(0.9))
    assert not (b & ~a).any() and (a != ref.keep_mask(n, 6, 1, drop_threshold(0.5))).any() and (a != ref.keep_mask(n, 5, 2, drop_threshold(0.5))).any()


def int_case(n, K, seed):
    """Integer-valued base and tasks (differences in -3 .. 3, many zeros and ties); K >= 2: on a tenth of the positions tau_1 = -tau_0."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, n).astype(f32)
    tasks = [(base + rng.integers(-3, 4, n) * (rng.random(n) < 0.7)).astype(f32) for _ in range(K)]
    if K >= 2:
        at = rng.random(n) < 0.1
        tasks[1] = np.where(at, base - (tasks[0] - base), tasks[1]).astype(f32)
    return base, tasks


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("mode", ["ties", "linear"])
def test_the_float32_oracle_is_the_float64_one_exactly_on_integers(mode, K):
    """Drop probabilities 0.5 and 0.75 (rescale 2 and 4, exact), power-of-two coefficients; in "ties" one magnitude per position and one
    probability for every task, so that the mean is that magnitude.  At T = 0 without rescale the oracle is merge_ref.apply_ref."""
    n = 4099
    base, tasks = int_case(n, K, 60 + K)
    ps = [0.5] * K if mode == "ties" else [0.5 if i % 2 == 0 else 0.75 for i in range(K)]
    if mode == "ties":
        mag = np.abs(tasks[0] - base)
        tasks = [(base + np.sign(t - base) * mag).astype(f32) for t in tasks]
    lam = [f32(2.0 ** -(i % 3)) * (-1 if i == 1 else 1) for i in range(K)]
    drop_thr, streams = [drop_threshold(p) for p in ps], list(range(K))
    for seed in SEEDS:
        for thr in ([merge_ref.select_ref(t, base, n // 5)[0] for t in tasks], [f32(0.0)] * K):
            for rescale in ([rescale_of(p) for p in ps], None):
                got, counts = ref.apply_drop_ref(base, tasks, thr, mode, lam, 0.5, drop_thr, rescale, streams, seed)
                want, mass, s = ref.apply_drop_ref64(base, tasks, thr, mode, lam, 0.5, drop_thr, rescale, streams, seed)
                assert got.dtype == f32 and np.array_equal(got.astype(np.float64), want), (mode, K, seed)
                assert counts["drawn"] == [int(ref.keep_mask(n, seed, i, drop_thr[i]).sum()) for i in range(K)]
                assert all(k <= d for k, d in zip(counts["kept"], counts["drawn"])) and all(w <= k for w, k in zip(counts["won"], counts["kept"]))
    thr = [merge_ref.select_ref(t, base, n // 5)[0] for t in tasks]
    got, counts = ref.apply_drop_ref(base, tasks, thr, mode, lam, 0.5, [0] * K, None, streams, 3)
    want, wcounts = merge_ref.apply_ref(base, tasks, thr, mode, lam, 0.5)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and counts["drawn"] == [n] * K
    assert {k: counts[k] for k in wcounts} == wcounts
    got, counts = ref.apply_drop_ref(base, tasks, thr, mode, lam, 0.5, [TWO32] * K, None, streams, 3)
    assert np.array_equal(got, base + f32(0.0)) and counts["drawn"] == [0] * K == counts["kept"] and counts["support"] == 0


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("mode", ["ties", "linear"])
def test_on_normal_data_the_float32_oracle_stays_within_its_rounding_bound(mode, K):
    """|out - out64| <= (K + 5) * 2^-24 * (|base| + |lam| * sum_i |rescale_i d_i|) per element: merge_ref's K + 4 and one more rounding, the
    product d_i * rescale_i.  In "ties" the positions with |s64| <= (K + 1) * 2^-23 * sum |rescale_i d_i| are left out -- the election is
    discontinuous there, and the rounded products move s by up to that much -- and their share may be at most 1e-4: a condition, not a
    measurement.  n = 100003, base N(0, 1), deltas N(0, 1) * 0.05 * 10^(-2 .. 0), density 0.2 and zeros, p = 0.9 and 0.5 mixed, lam = 0.7."""
    n = 100003
    rng = np.random.default_rng(500 + K)
    base = rng.standard_normal(n).astype(f32)
    tasks = [(base + (rng.standard_normal(n) * 0.05 * 10.0 ** rng.integers(-2, 1, n)).astype(f32)).astype(f32) for _ in range(K)]
    ps = [0.9 if i % 2 == 0 else 0.5 for i in range(K)]
    drop_thr, rescale, streams = [drop_threshold(p) for p in ps], [rescale_of(p) for p in ps], list(range(K))
    cfg = MergeConfig(method=mode, density=0.2, lam=0.7)
    lam = merge.coefficients(cfg, K) if mode == "linear" else None
    lam_out = float(f32(0.7))
    for thr in ([merge_ref.select_ref(t, base, merge.rank_of(0.2, n))[0] for t in tasks], [f32(0.0)] * K):
        got, counts = ref.apply_drop_ref(base, tasks, thr, mode, lam, lam_out, drop_thr, rescale, streams, 2024)
        want, mass, s = ref.apply_drop_ref64(base, tasks, thr, mode, lam, lam_out, drop_thr, rescale, streams, 2024)
        scale = max(abs(v) for v in lam) if mode == "linear" else lam_out
        bound = (K + 5) * 2.0 ** -24 * (np.abs(base.astype(np.float64)) + scale * mass)
        err = np.abs(got.astype(np.float64) - want)
        near = np.zeros(n, dtype=bool) if s is None else (mass > 0) & (np.abs(s) <= (K + 1) * 2.0 ** -23 * mass)
        excluded, use = float(near.mean()), ~near
        ratio = float((err[use] / bound[use]).max())
        print(f"[merge-drop] oracle {mode} K={K} thr0={float(thr[0]):.3g}: excluded share {excluded:.2e}, largest error / bound {ratio:.3f}")
        assert excluded <= 1e-4, excluded
        assert np.all(err[use] <= bound[use]), ratio


def test_fine_mix_ref_moves_bits():
    n = 2051
    rng = np.random.default_rng(4)
    clean, bd = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    special = np.array([0x80000000, 0x00000001, 0x7F800000, 0x7FC01234, 0xFFC00001], dtype=np.uint32).view(f32)
    clean[:5], bd[5:10] = special, special
    bd[20:30] = clean[20:30]
    for keep in (0.0, 0.3, 1.0):
        out, rec = ref.fine_mix_ref(clean, bd, keep, seed=9)
        mask = ref.keep_mask(n, 9, 0, ref.mix_threshold(keep))
        assert np.array_equal(out.view(np.uint32), np.where(mask, bd.view(np.uint32), clean.view(np.uint32)))
        assert rec["drawn"] == int(mask.sum()) and rec["numel"] == n and rec["drop_threshold"] == ref.mix_threshold(keep)
        with np.errstate(invalid="ignore"):
            assert rec["differing"] == int((mask & (bd != clean)).sum())
    assert np.array_equal(ref.fine_mix_ref(clean, bd, 1.0)[0].view(np.uint32), bd.view(np.uint32))
    assert np.array_equal(ref.fine_mix_ref(clean, bd, 0.0)[0].view(np.uint32), clean.view(np.uint32))
    assert abs(ref.fine_mix_ref(clean, bd, 0.3, seed=9)[1]["drawn_share"] - 0.3) <= 4 * math.sqrt(0.21 / n)


# ------------------------------------------------------------------------------------------------------------------------------- the tool
def test_the_tools_new_argument_errors():
    tool = os.path.join(ROOT, "tools", "merge_checkpoints.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--base", "B", "--out", "M"]
    for argv, msg in ((common + ["--ckpt", "A", "--method", "dare"], "invalid choice"),
                      (common + ["--ckpt", "A", "--drop", "1.0"], r"--drop must lie in \[0, 1\)"),
                      (common + ["--ckpt", "A", "--drop", "-0.1"], r"--drop must lie in \[0, 1\)"),
                      (common + ["--ckpt", "A", "--drop", "a"], "--drop takes a comma-separated list of finite numbers"),
                      (common + ["--ckpt", "A", "B", "C", "--drop", "0.9,0.5"], "--drop holds 2 numbers, --ckpt names 3 checkpoints"),
                      (common + ["--ckpt", "A", "--no-rescale"], "--no-rescale is read with --drop only"),
                      (common + ["--ckpt", "A", "--drop", "0.9", "--seed", "-1"], r"--seed must lie in \[0, 2\^64\)"),
                      (common + ["--ckpt", "A", "--mix-keep", "0.3"], "--mix-keep is read by --method mix only"),
                      (common + ["--ckpt", "A", "--method", "mix"], "--method mix needs --mix-keep"),
                      (common + ["--ckpt", "A", "--method", "mix", "--mix-keep", "1.5"], r"--mix-keep must lie in \[0, 1\]"),
                      (common + ["--ckpt", "A", "B", "--method", "mix", "--mix-keep", "0.3"], "--method mix takes exactly one --ckpt"),
                      (common + ["--ckpt", "A", "--method", "mix", "--mix-keep", "0.3", "--drop", "0.5"], "--drop is read by --method ties and --method linear"),
                      (common + ["--ckpt", "A", "--method", "mix", "--mix-keep", "0.3", "--scan", "0.5,2", "--dataset", "D"],
                       r"--scan takes keep shares in \[0, 1\]")):
        out = subprocess.run([sys.executable, tool] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and re.search(msg, out.stderr), (argv, out.stderr[-500:])
    out = subprocess.run([sys.executable, tool, "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--drop" in out.stdout and "--mix-keep" in out.stdout and "DARE" in out.stdout and "Fine-mixing" in out.stdout
