"""The seeded drop of checkpoint merging (DARE, Fine-mixing) restated for the tests (a helper module, not a test file; no GPU needed).

1. `keep_mask`: the keep bits of vd_merge_apply_drop for one task, from elem_ref.philox4x32_10 in integer arithmetic: element j is kept where
   word j & 3 of philox4x32_10((lo32(j >> 2), hi32(j >> 2), stream, 1), (lo32(seed), hi32(seed))) is >= T.
2. `apply_drop_ref`: the numpy float32 op sequence of vd_merge_apply_drop with its 3 K + 2 counts: merge_ref.trimmed gives the thresholded
   differences, the mask and the rescale follow, and the modes proceed as in merge_ref.apply_ref (whose bits it gives at T = 0 without rescale).
3. `apply_drop_ref64`: the same from the SAME float32 differences, thresholds and masks with everything after the trimming in float64.
4. `fine_mix_ref`: where(mask, backdoored, clean) on the bits, with the record merge.fine_mix returns."""
import numpy as np

import elem_ref
import merge_ref

f32 = np.float32
TWO32 = 1 << 32


def keep_mask(n, seed, stream, T):
    """bool [n]: element j of a task with stream id `stream` is kept.  0 <= T <= 2^32."""
    assert 0 <= T <= TWO32 and 0 <= seed < 1 << 64 and 0 <= stream < TWO32
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    full = lambda v: np.full(nq, v, dtype=np.uint64)                                     # noqa: E731
    r = elem_ref.philox4x32_10((q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), full(stream), full(1)), (full(seed & 0xFFFFFFFF), full(seed >> 32)))
    words = np.stack(r, axis=1).reshape(-1)[:n].astype(np.uint64)
    return words >= np.uint64(T)


def dropped(base, tasks, thr, drop_thr, rescale, streams, seed):
    """([K, n] float32 t_i = (|d_i| >= thr_i && keep_i) ? (rescale ? d_i * rescale_i : d_i) : +0.0, kept masks, drawn masks)."""
    t, keep_thr = merge_ref.trimmed(base, tasks, thr)
    n = t.shape[1]
    drawn = np.stack([keep_mask(n, seed, streams[i], drop_thr[i]) for i in range(len(tasks))]) if n else np.zeros(t.shape, dtype=bool)
    kept = keep_thr & drawn
    if rescale is not None:
        with np.errstate(over="ignore"):
            t = (t * np.asarray(rescale, dtype=f32)[:, None]).astype(f32)
    return np.where(kept, t, f32(0.0)).astype(f32), kept, drawn


def apply_drop_ref(base, tasks, thr, mode, lam, lam_out, drop_thr, rescale, streams, seed):
    """(out float32, counts) of vd_merge_apply_drop without VD_DROP_COPY.  rescale None: no VD_DROP_RESCALE.  counts: drawn, kept, won [K],
    support, conflict."""
    t, kept, drawn = dropped(base, tasks, thr, drop_thr, rescale, streams, seed)
    K, n = t.shape
    if mode == "linear":
        acc = np.zeros(n, dtype=f32)
        for i in range(K):
            acc = acc + f32(lam[i]) * t[i]
        out, entered = (base + acc).astype(f32), t != 0
    else:
        s = np.zeros(n, dtype=f32)
        for i in range(K):
            s = s + t[i]
        plus = s >= 0
        m, c = np.zeros(n, dtype=f32), np.zeros(n, dtype=np.int32)
        entered = np.zeros((K, n), dtype=bool)
        for i in range(K):
            entered[i] = (t[i] != 0) & ((t[i] > 0) == plus)
            m = np.where(entered[i], m + t[i], m).astype(f32)
            c = c + entered[i]
        tau = np.zeros(n, dtype=f32)
        np.divide(m, c.astype(f32), out=tau, where=c > 0)
        out = (base + f32(lam_out) * tau).astype(f32)
    counts = merge_ref.counts_of(t, kept, entered)
    counts["drawn"] = [int(v) for v in drawn.sum(1)]
    return out, counts


def stats_list(counts):
    """The 3 K + 2 int64 of vd_merge_apply_drop in their order."""
    return counts["drawn"] + counts["kept"] + counts["won"] + [counts["support"], counts["conflict"]]


def apply_drop_ref64(base, tasks, thr, mode, lam, lam_out, drop_thr, rescale, streams, seed):
    """(out float64, sum_i |rescale_i d_i| over the kept entries float64, s float64 (ties; None for linear)): the float32 differences,
    thresholds and masks, the rescale and everything after it in float64."""
    t32, kept, _ = dropped(base, tasks, thr, drop_thr, None, streams, seed)
    t = t32.astype(np.float64)
    if rescale is not None:
        t = t * np.asarray([float(f32(v)) for v in rescale])[:, None]
    K, n = t.shape
    b = base.astype(np.float64)
    mass = np.abs(t).sum(0)
    if mode == "linear":
        acc = np.zeros(n)
        for i in range(K):
            acc = acc + float(f32(lam[i])) * t[i]
        return b + acc, mass, None
    s = t.sum(0)
    plus = s >= 0
    m, c = np.zeros(n), np.zeros(n)
    for i in range(K):
        entered = (t[i] != 0) & ((t[i] > 0) == plus)
        m = np.where(entered, m + t[i], m)
        c = c + entered
    tau = np.zeros(n)
    np.divide(m, c, out=tau, where=c > 0)
    return b + float(f32(lam_out)) * tau, mass, s


def mix_threshold(keep):
    """T of fine_mix: 2^32 - floor(keep * 2^32)."""
    return TWO32 - int(np.floor(np.float64(keep) * np.float64(TWO32)))


def fine_mix_ref(clean, backdoored, keep, seed=0, stream=0):
    """(out float32 with the bits of where(mask, backdoored, clean), the record of merge.fine_mix)."""
    n = clean.size
    T = mix_threshold(keep)
    mask = keep_mask(n, seed, stream, T)
    out = np.where(mask, backdoored.view(np.uint32), clean.view(np.uint32)).astype(np.uint32).view(f32)
    with np.errstate(invalid="ignore"):
        differing = int((mask & (backdoored != clean)).sum())
    drawn = int(mask.sum())
    return out, {"keep": float(keep), "seed": seed, "drop_threshold": T, "drawn": drawn, "drawn_share": drawn / max(n, 1), "differing": differing,
                 "numel": n}
