"""Checkpoint merging restated for the tests (a helper module, not a test file; no GPU needed).

1. `select_ref`: what vd_merge_select must give, from np.partition over the uint32 bits of the float32 |w - base|.
2. `apply_ref`: the numpy float32 op sequence of vd_merge_apply, operation by operation as include/villan_hip.h states it, with the integer
   counts (kept, won, support, conflict).
3. `apply_ref64`: the same merge from the SAME float32 differences d_i and thresholds -- so the trimming is identical -- with everything after
   the trimming in float64, and the per-element quantities the error bound of tests/test_merge_cpu.py is made of.
4. `family_case`: one seeded base and three seeded task checkpoints of a small network (a shared dense part plus private sparse spikes)."""
import numpy as np
import torch

import curve_ref

SMALL = curve_ref.SMALL
f32 = np.float32
INF_KEY = 0x7F800000


def keys_of(w, base):
    """The uint32 bits of |w - base|, one float32 subtraction."""
    return np.abs((w - base).astype(f32)).view(np.uint32)


def select_ref(w, base, k):
    """(threshold as float32, n_gt, n_eq, n_nonfinite) of the k-th largest key; k = 0: (+inf, 0, 0, n_nonfinite)."""
    keys = keys_of(w, base)
    n = keys.size
    assert 0 <= k <= n
    nonfinite = int((keys >= INF_KEY).sum())
    if k == 0:
        return f32(np.inf), 0, 0, nonfinite
    thr = np.partition(keys, n - k)[n - k]
    return np.array([thr], dtype=np.uint32).view(f32)[0], int((keys > thr).sum()), int((keys == thr).sum()), nonfinite


def trimmed(base, tasks, thr):
    """[K, n] float32: t_i = (|d_i| >= thr_i) ? d_i : +0.0 with d_i = tasks[i] - base, and the keep masks."""
    d = np.stack([(t - base).astype(f32) for t in tasks])
    with np.errstate(invalid="ignore"):
        keep = np.abs(d) >= np.asarray(thr, dtype=f32)[:, None]
    return np.where(keep, d, f32(0.0)).astype(f32), keep


def counts_of(t, keep, entered):
    nz = t != 0
    pos, neg = (t > 0).any(0), (t < 0).any(0)
    return {"kept": [int(v) for v in keep.sum(1)], "won": [int(v) for v in entered.sum(1)], "support": int(nz.any(0).sum()),
            "conflict": int((pos & neg).sum())}


def apply_ref(base, tasks, thr, mode, lam=None, lam_out=1.0):
    """(out float32, counts) of vd_merge_apply.  lam: the K float32 coefficients of "linear"."""
    t, keep = trimmed(base, tasks, thr)
    K, n = t.shape
    if mode == "linear":
        acc = np.zeros(n, dtype=f32)
        for i in range(K):
            acc = acc + f32(lam[i]) * t[i]
        return (base + acc).astype(f32), counts_of(t, keep, t != 0)
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
    return (base + f32(lam_out) * tau).astype(f32), counts_of(t, keep, entered)


def apply_ref64(base, tasks, thr, mode, lam=None, lam_out=1.0):
    """(out float64, sum_i |t_i| float64, s float64 (ties; None for linear)): the float32 d_i and thresholds, the rest in float64."""
    t32, _ = trimmed(base, tasks, thr)
    t = t32.astype(np.float64)
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


def g(seed):
    return torch.Generator().manual_seed(seed)


def task_vectors(n, seed, K=3, scale=0.02, spikes=0.002):
    """base-free task vectors: a shared dense part (what the fine-tunes have in common) plus, per task, private sparse spikes on a `spikes`
    share of the positions, ten times the dense scale."""
    gen = g(seed)
    shared = torch.randn(n, generator=gen) * scale
    out = []
    for _ in range(K):
        own = torch.randn(n, generator=gen) * scale * 0.5
        at = torch.rand(n, generator=gen) < spikes
        spike = torch.randn(n, generator=gen) * scale * 10.0
        out.append(shared + own + torch.where(at, spike, torch.zeros(n)))
    return out


def family_case(make, seed=11, K=3):
    """(a network on the CPU at a seeded base, base flat tensor, K task checkpoints base + tau_i) for a constructor `make(device=...)`."""
    net = make(device="cpu")
    net.reset_parameters(seed=seed)
    base = net.flat_param.detach().clone()
    return net, base, [(base + tv).contiguous() for tv in task_vectors(base.numel(), seed + 1, K)]
