"""What villandiffusion_amd.clp and vd_channel_lipschitz are held to, in numpy and torch on the CPU:

* `sigma_max64`: the largest singular value of every row of an f32 weight, the row seen as [Cin, T], by a float64 SVD;
* `gram_ordered_f32`: the Gram matrix in the kernel's stated f32 order -- lane l owns the channels l, l + 64, ... in ascending order, one
  partial per entry from +0 with the product and the sum rounded on their own, the 64 lanes added by the xor tree (offsets 32 ... 1) -- so the
  kernel's `gram` output can be compared bit for bit;
* `jacobi_lambda_max_f32`: the header's eigen stage restated in numpy float32 (the schedule and the formulas; no bitwise promise);
* `outliers`: CLP's rule, z = (x - mean) / std with the unbiased std over the rows that are not exactly zero, flagged where z > u;
* `uclc_ref`: the whole score of a network's layer from its state dict."""
import numpy as np
import torch

GRAM = 45
SWEEPS = 8
SKIP = np.float32(2.0 ** -30)
U = 2.0 ** -24
EIGEN_BOUND = 5760.5 * 2.0 ** -24            # what include/villan_hip.h derives for lambda_max


def entries(T):
    """The (i, j), i <= j, of a T x T Gram matrix in slot order: the upper triangle row by row."""
    return [(i, j) for i in range(T) for j in range(i, T)]


def slot(i, j):
    return i * 9 - i * (i - 1) // 2 + (j - i)


def chain(Cin):
    return (Cin + 63) // 64 + 6


def sigma_max64(w):
    """w: [rows, Cin, T] f32 (torch or numpy) -> [rows] float64."""
    a = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.linalg.svd(a, compute_uv=False)[:, 0]


def gram64(w):
    """[rows, T, T] float64 Gram of the f32 weights."""
    a = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.einsum("rci,rcj->rij", a, a)


def gram_abs64(w):
    a = np.abs(np.asarray(w, dtype=np.float32).astype(np.float64))
    return np.einsum("rci,rcj->rij", a, a)


def gram_ordered_f32(w):
    """w: [rows, Cin, T] f32 -> [rows, T (T + 1) / 2] f32, the kernel's order of operations."""
    a = np.asarray(w, dtype=np.float32)
    rows, Cin, T = a.shape
    steps = (Cin + 63) // 64
    pad = np.zeros((rows, steps * 64, T), dtype=np.float32)
    pad[:, :Cin] = a
    pad = pad.reshape(rows, steps, 64, T)
    have = (np.arange(steps * 64) < Cin).reshape(steps, 64)
    ent = entries(T)
    p = np.zeros((rows, 64, len(ent)), dtype=np.float32)
    for s in range(steps):
        for e, (i, j) in enumerate(ent):
            prod = (pad[:, s, :, i] * pad[:, s, :, j]).astype(np.float32)
            p[:, :, e] = np.where(have[s][None, :], (p[:, :, e] + prod).astype(np.float32), p[:, :, e])
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = (p + p[:, lanes ^ off, :]).astype(np.float32)
    assert (p == p[:, :1, :]).all()                          # every lane ends with the same bits
    return p[:, 0, :]


def full_from_slots(g, T=9):
    """[rows, T (T + 1) / 2] -> the symmetric [rows, T, T] in float64."""
    g = np.asarray(g, dtype=np.float64)
    G = np.zeros((g.shape[0], T, T))
    for e, (i, j) in enumerate(entries(T)):
        G[:, i, j] = g[:, e]
        G[:, j, i] = g[:, e]
    return G


def jacobi_lambda_max_f32(g45, sweeps=SWEEPS):
    """One row's 45 Gram slots (f32) -> (lambda_max in f32 by the header's schedule, rotations carried out, off-diagonal norm left over
    relative to lambda_max)."""
    f = np.float32
    a = np.zeros((9, 9), dtype=np.float32)
    for e, (i, j) in enumerate(entries(9)):
        a[i, j] = a[j, i] = g45[e]
    m = a.diagonal().max()
    if m == 0:
        return f(0), 0, 0.0
    ex = int(np.floor(np.log2(float(m))))
    a = np.ldexp(a, -ex).astype(np.float32)
    done = 0
    for _ in range(sweeps):
        for p in range(8):
            for q in range(p + 1, 9):
                apq = a[p, q]
                if not abs(apq) > SKIP:
                    continue
                done += 1
                app, aqq = a[p, p], a[q, q]
                theta = f(f(aqq - app) / f(f(2) * apq))
                t = f(np.copysign(f(1), theta) / f(abs(theta) + np.sqrt(f(f(theta * theta) + f(1)))))
                c = f(f(1) / np.sqrt(f(f(t * t) + f(1))))
                s = f(t * c)
                tau = f(s / f(f(1) + c))
                h = f(t * apq)
                a[p, p], a[q, q] = f(app - h), f(aqq + h)
                a[p, q] = a[q, p] = f(0)
                for k in range(9):
                    if k in (p, q):
                        continue
                    x, y = a[k, p], a[k, q]
                    a[k, p] = a[p, k] = f(x - f(s * f(y + f(tau * x))))
                    a[k, q] = a[q, k] = f(y + f(s * f(x - f(tau * y))))
    lam = a.diagonal().max()
    off = float(np.sqrt(((a.astype(np.float64) - np.diag(a.diagonal().astype(np.float64))) ** 2).sum())) / float(lam)
    return f(np.ldexp(lam, ex)), done, off


def outliers(x, u):
    """x: [rows] UCLC -> (z [rows] float64 torch, flagged [rows] bool): the statistics over the rows that are not exactly zero (unbiased std,
    as torch.std), strict z > u; zero rows get z = -inf; fewer than 2 live rows or std == 0: z = 0, nothing is flagged."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    live = x != 0
    z = torch.full_like(x, -float("inf"))
    z[live] = 0.0
    if int(live.sum()) >= 2:
        std = torch.std(x[live])
        if float(std) > 0:
            z[live] = (x[live] - x[live].mean()) / std
    return z, z > u


def scale_source(state, name):
    """The GroupNorm weight that normalises the layer's output directly: the ResnetBlock pair conv1 -> norm2."""
    if not name.endswith(".conv1.weight"):
        return None
    src = name[:-len("conv1.weight")] + "norm2.weight"
    return src if src in state and state[src].numel() == state[name].shape[0] else None


def uclc_ref(state, name, scale):
    """float64 [rows]: sigma_max of every row of state[name] seen as [Cin, T], times |gamma| of its scale source (scale == "gamma")."""
    w = state[name].detach().float()
    s = sigma_max64(w.reshape(w.shape[0], w.shape[1], -1).numpy())
    src = scale_source(state, name)
    if scale == "gamma" and src is not None:
        s = s * np.abs(state[src].detach().float().numpy().astype(np.float64))
    return s


def score_bound(Cin):
    """The issue's bound of |UCLC - UCLC_ref| / UCLC_ref: the Gram by Weyl's inequality with tr G <= 9 lambda_max, the eigen stage, the square
    root and the scale product."""
    return 0.5 * (9 * (chain(Cin) + 1) * U + EIGEN_BOUND) + 2 * U
