"""float64 references, hard inputs, case lists and bounds for the attention tests (a helper module, not a test file; no GPU needed).

Layout as in the kernels: qkv [B, 3C, N] (q | k | v, head h = channels [h d, (h + 1) d) of each), scores keys-major,
S[b, h, j, i] = scale * sum_c k[c, j] q[c, i], softmax over j, out[c, i] = sum_j v[c, j] P[j, i].

Hard inputs.  q and k of `mixed_qkv` lie on the grid of multiples of 1/4 in [-8, 8]: bf16 holds every such value, so the split-precision
products see hi = x, lo = 0, and a d-term sum of products (multiples of 1/16, |sum| <= 512 * 64 = 2^15) is exact in float32 in any
order.  Whatever arithmetic a kernel uses, the scores it sees are therefore the exact ones up to the single rounding of scale * s.  (The
range is [-8, 8] because a 32-channel head has to hold a shift of +70 and a ramp that spans 100 at scale = 1 / sqrt(32) at once.)
The keys of a (batch, head) slice carry four channel groups (placed by a seeded permutation of the head's channels) and every query
column picks one of five patterns through the channels it weights -- pattern and dominating key from `column_patterns`, which
follows neither the 32-column wave layout nor the 64-column blocks:

  code   4 r channels, +-8: seven "beacon" keys carry the seven non-zero even-weight words of length 4, every other key 0000.
         peaked:     q = the word of beacon m(i): that key beats every other by 256 r scale >= 30.  The beacons sit at
                     j = (2 m + 1) N / 14, so some maxima arrive in the last key block.
  const  n_const channels, k = 8.
         tied:       q = 8 there, 0 elsewhere: every key scores the same ~ +70, P = 1 / N.
  ramp   n_ramp channels k = level(j) / 64 - 8 (coarse) and one channel (level mod 16) / 4 - 2 (fine); level(j) rises 0 .. 1023,
         85 % of it within the first quarter of the keys.
         ascending:  q = +8 / +qf (and +8 on const): the score rises with j by ~ 113 in all, from ~ +12 to ~ +125, so every key
                     block's maximum exceeds the previous one's, and exp(score) without the maximum taken off overflows float32.
         descending: q = -8 / -qf (and -8 on const): the maximum (~ -12) is at j = 0 and every key past the first quarter is > 89
                     below it: its probability underflows float32.
  noise  the remaining channels, k random on the grid.
         shifted:    q = 8 on const, +-1/4 or +-1/2 on noise: scores ~ +70 with O(1) differences.

v and dout stay randn.  For the bare softmax kernels `softmax_scores` writes the same five column patterns (and randn * 3) into S;
the reference is computed from those float32 values.

PROP_BLOCK(N) = min(256, N / 4) is the key-block size the property checks use: the flash kernels' 256-key block, and a quarter of the
keys where everything is one block."""
import math

import torch

PATTERNS = ("peaked", "tied", "ascending", "descending", "shifted")
GRID_LIM = 8.0
TOL_P, TOL_OUT, TOL_FLASH_OUT, TOL_GRAD = 2e-5, 2e-5, 3e-5, 5e-5     # the suite's max|a - b| / max|b| tolerances (test_hip_kernels.py)
F32_MIN_NORMAL = 1.1754943508222875e-38

# ---------------------------------------------------------------------------------------------------------------- case lists
SOFTMAX_NS = (1, 2, 3, 5, 16, 63, 64, 65, 100, 128, 129, 192, 255, 256, 257, 320, 1000)
SOFTMAX_NBS = (1, 3)
SOFTMAX_KINDS = ("randn3", "mixed")                       # randn * 3, and the five patterns mixed across the columns
SOFTMAX_BWD_SCALE = 0.1767766952966369                    # 1 / sqrt(32)
SMALL_SHAPES = ((256, 16), (64, 64), (128, 32), (129, 32), (68, 60), (69, 60), (512, 16), (256, 64), (96, 49), (32, 4), (8, 1))
SMALL_BS = (1, 5)
SMALL_HARD_SHAPES = ((256, 16), (512, 16), (256, 64))
CORE_HARD = tuple((2, 3, d) for d in (32, 64, 256))       # (B, heads, d) at N = 256
FLASH_CASES = (("mixed", 2, 3, 256), ("mixed", 2, 3, 768), ("mixed", 2, 3, 1024), ("randn", 2, 3, 768))


def prop_block(N):
    return min(256, max(N // 4, 1))


def f32(x):
    """The float32 value of a Python float, as a Python float (what a kernel receives for `scale`)."""
    return float(torch.tensor(x, dtype=torch.float32))


def rel(a, b):
    """max |a - b| / max |b| (the suite's metric)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ----------------------------------------------------------------------------------------------------------- f64 references
def attention_f64(qkv, dout, heads, scale):
    """Multi-head attention and its gradients in float64 from the float32 inputs and the float32 value of `scale`.
    Returns S, P, dS [B, heads, N(j), N(i)], lse [B, heads, N], out [B, C, N], dq, dk, dv [B, C, N]; dS carries `scale`
    (dS = scale P (dP - sum_j P dP), as attn_core_bwd writes it), all in closed form."""
    B, C3, N = qkv.shape
    C = C3 // 3
    d = C // heads
    sc = f32(scale)
    q, k, v = (qkv[:, t * C:(t + 1) * C].double().reshape(B, heads, d, N) for t in range(3))
    do = dout.double().reshape(B, heads, d, N)
    S = torch.einsum("bhcj,bhci->bhji", k, q) * sc
    m = S.amax(2, keepdim=True)
    E = torch.exp(S - m)
    Z = E.sum(2, keepdim=True)
    P = E / Z
    lse = (m + torch.log(Z)).squeeze(2)
    out = torch.einsum("bhcj,bhji->bhci", v, P)
    dP = torch.einsum("bhcj,bhci->bhji", v, do)
    dS = sc * P * (dP - (P * dP).sum(2, keepdim=True))
    dq = torch.einsum("bhcj,bhji->bhci", k, dS)
    dk = torch.einsum("bhci,bhji->bhcj", q, dS)
    dv = torch.einsum("bhci,bhji->bhcj", do, P)
    r = lambda t: t.reshape(B, C, N)  # noqa: E731
    return dict(S=S, P=P, lse=lse, dS=dS, out=r(out), dq=r(dq), dk=r(dk), dv=r(dv))


def attention_torch_f32(qkv, dout, heads, scale):
    """The same quantities from plain torch float32 on the CPU (einsum, softmax, logsumexp, autograd): the arithmetic whose own error
    the bounds are measured from, and which has to pass every tolerance the kernels are held to."""
    B, C3, N = qkv.shape
    C = C3 // 3
    d = C // heads
    x = qkv.detach().clone().float().requires_grad_(True)
    q, k, v = (x[:, t * C:(t + 1) * C].reshape(B, heads, d, N) for t in range(3))
    S = torch.einsum("bhcj,bhci->bhji", k, q) * f32(scale)
    S.retain_grad()
    P = torch.softmax(S, dim=2)
    out = torch.einsum("bhcj,bhji->bhci", v, P).reshape(B, C, N)
    out.backward(dout.float())
    g = x.grad
    return dict(S=S.detach(), P=P.detach(), lse=torch.logsumexp(S.detach(), dim=2), dS=S.grad * f32(scale), out=out.detach(),
                dq=g[:, :C], dk=g[:, C:2 * C], dv=g[:, 2 * C:])


def softmax_col_f64(S):
    """Column softmax of S [nb, N(j), N(i)] over j, in float64 from the values given."""
    S = S.double()
    E = torch.exp(S - S.amax(1, keepdim=True))
    return E / E.sum(1, keepdim=True)


def softmax_col_bwd_f64(P, dP, scale):
    """dS = scale P (dP - sum_j P dP) in float64 from the float32 P, dP and the float32 value of scale."""
    P, dP = P.double(), dP.double()
    return f32(scale) * P * (dP - (P * dP).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------------- bounds
def ulp32(x):
    """The spacing of float32 at |x| (a Python float)."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x else 2.0 ** -149


def lse_bound(S32):
    """Absolute bound for lse on hard inputs: 4 x the worst error of torch's float32 logsumexp of the float32 scores S32 [..., N(j), N(i)]
    against float64 of the same values, with a floor of 4 float32 ulps of max |lse| (a kernel adds one rounding of the scaled score and a
    fast log / exp).  Returns (bound, the measured torch error)."""
    l64 = torch.logsumexp(S32.double(), dim=-2)
    err = float((torch.logsumexp(S32.float(), dim=-2).double() - l64).abs().max())
    return max(4 * err, 4 * ulp32(float(l64.abs().max()))), err


def p_elem_err(P, P_ref):
    """Worst elementwise relative error of P on the entries with P_ref >= 1e-3."""
    P, P_ref = P.detach().double().cpu(), P_ref.detach().double().cpu()
    mask = P_ref >= 1e-3
    return float(((P - P_ref).abs() / P_ref)[mask].max()) if bool(mask.any()) else 0.0


def p_elem_bound(P_torch32, P_ref):
    """Elementwise relative bound for P where P_ref >= 1e-3: 8 x torch's own float32 error on those entries (the fast exponential rounds
    its argument, |x| <= 7 there, where torch's is correctly rounded to ~1 ulp).  Returns (bound, the measured torch error)."""
    err = p_elem_err(P_torch32, P_ref)
    return 8 * err, err


def colsum_bound(N):
    """Bound for |sum_j P[j, i] - 1| of a float32 column softmax.  The normaliser is a float32 sum of N positive terms in chains of N / 4
    (one per wave) plus 3 combining adds, each add off by at most 2^-24 of the running sum: (N / 4 + 3) 2^-24.  The rest is per element and
    at worst systematic: the fast exponential's rounded argument on the entries that matter (|x| <= 16: 16 log2(e) = 23 half-ulps), the
    exp2 itself and the two roundings of the normalisation: 29 half-ulps allowed."""
    return (N / 4 + 32) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- hard inputs
def column_patterns(N, s=0):
    """(pattern index into PATTERNS, beacon index 0..6) of every query column of slice s: any five consecutive columns hold all
    five patterns, and the order shifts by one every five columns and with the slice."""
    i = torch.arange(N)
    return (3 * i + i // 5 + s) % 5, (i + i // 5 + 2 * s) % 7


def beacons(N):
    assert N >= 14
    return [((2 * m + 1) * N) // 14 for m in range(7)]


def ramp_level(N):
    """level(j) in 0 .. 1023, non-decreasing: 0 .. 869 over the first quarter of the keys (strictly rising), 870 .. 1023 over the rest."""
    j = torch.arange(N)
    q4 = max(N // 4, 1)
    return torch.where(j < q4, (j * 870) // q4, 870 + ((j - q4) * 154) // max(N - q4, 1))


def groups(d, scale):
    """Channel counts (code, ramp, const, noise) and the fine weight qf for a head of d channels."""
    n_code = 4 * math.ceil(30 / (256 * scale))
    n_ramp = math.ceil(105 / (128 * scale))
    n_const = max(1, round(70 / (64 * scale)))
    n_noise = d - n_code - n_ramp - 1 - n_const
    assert n_noise >= 4, f"a head of {d} channels cannot hold the pattern groups"
    return n_code, n_ramp, n_const, n_noise, min(n_ramp / 2, GRID_LIM)


_WORDS = [w for w in range(1, 16) if bin(w).count("1") % 2 == 0]          # the seven non-zero even-weight words of length 4


def mixed_slice(d, N, scale, s, gen):
    """q, k [d, N] (float32, on the grid) of slice s: the five patterns mixed across the query columns."""
    n_code, n_ramp, n_const, n_noise, qf = groups(d, scale)
    perm = torch.randperm(d, generator=gen)
    c_code, c_ramp, c_fine, c_const, c_noise = torch.split(perm, [n_code, n_ramp, 1, n_const, n_noise])
    q, k = torch.zeros(d, N), torch.zeros(d, N)
    bits = lambda w: torch.tensor([8.0 if (w >> t) & 1 else -8.0 for t in range(4)]).repeat(n_code // 4)  # noqa: E731
    k[c_code] = bits(0)[:, None]
    for m, j in enumerate(beacons(N)):
        k[c_code, j] = bits(_WORDS[m])
    lvl = ramp_level(N)
    k[c_ramp] = (torch.div(lvl, 16, rounding_mode="floor") / 4.0 - 8.0)[None]
    k[c_fine] = ((lvl % 16) / 4.0 - 2.0)[None]
    k[c_const] = 8.0
    k[c_noise] = torch.randint(-32, 33, (n_noise, N), generator=gen) / 4.0
    pat, bm = column_patterns(N, s)
    qn = torch.tensor([-0.5, -0.25, 0.25, 0.5])[torch.randint(0, 4, (n_noise, N), generator=gen)]
    for i in range(N):
        p = PATTERNS[int(pat[i])]
        if p == "peaked":
            q[c_code, i] = bits(_WORDS[int(bm[i])])
        elif p in ("ascending", "descending"):
            sgn = 1.0 if p == "ascending" else -1.0
            q[c_ramp, i] = 8.0 * sgn
            q[c_fine, i] = qf * sgn
            q[c_const, i] = 8.0 * sgn
        else:
            q[c_const, i] = 8.0
            if p == "shifted":
                q[c_noise, i] = qn[:, i]
    return q, k


def mixed_qkv(B, heads, d, N, seed):
    """qkv [B, 3 heads d, N]: every (batch, head) slice from mixed_slice (slice index b heads + h), v = randn."""
    gen = torch.Generator().manual_seed(seed)
    C = heads * d
    scale = f32(1 / math.sqrt(d))
    qkv = torch.randn(B, 3 * C, N, generator=gen)
    for b in range(B):
        for h in range(heads):
            q, k = mixed_slice(d, N, scale, b * heads + h, gen)
            qkv[b, h * d:(h + 1) * d] = q
            qkv[b, C + h * d:C + (h + 1) * d] = k
    return qkv


def randn_qkv(B, C, N, seed, gain=1.3):
    return torch.randn(B, 3 * C, N, generator=torch.Generator().manual_seed(seed)) * gain


def randn_like_out(B, C, N, seed):
    return torch.randn(B, C, N, generator=torch.Generator().manual_seed(seed))


def softmax_patterns(N, b):
    i = torch.arange(N)
    return (3 * i + i // 5 + b + 1) % 5


def softmax_scores(kind, nb, N, seed):
    """float32 scores S [nb, N(j), N(i)] for the bare softmax kernels.  kind: "randn3" (randn * 3), "mixed" (column i of item b holds
    PATTERNS[(3 i + i / 5 + b + 1) mod 5]: column 0 of item 0 is tied and column 1 shifted, so that even N = 2 has columns whose dS is
    not degenerate and the relative-to-max metric keeps its meaning) or one of PATTERNS (that pattern in every column; for the
    property checks).
      peaked      35 at key (7 i + 3 + b) mod N, the others uniform in [-2, 2]
      tied        every key 12.5
      ascending   -60 .. +60, linear in j with a little positive jitter kept below one step (the running maximum moves on every row)
      descending  +60 .. -60: the last quarter's probabilities underflow float32
      shifted     70 + randn"""
    gen = torch.Generator().manual_seed(seed)
    if kind == "randn3":
        return torch.randn(nb, N, N, generator=gen) * 3
    j = torch.arange(N, dtype=torch.float32)[:, None]
    i = torch.arange(N)
    step = 120.0 / max(N - 1, 1)
    ramp = -60.0 + step * j + 0.5 * step * torch.rand(N, N, generator=gen)
    S = torch.empty(nb, N, N)
    for b in range(nb):
        cols = {"peaked": torch.rand(N, N, generator=gen) * 4 - 2, "tied": torch.full((N, N), 12.5), "ascending": ramp,
                "descending": -ramp, "shifted": 70 + torch.randn(N, N, generator=gen)}
        cols["peaked"][(7 * i + 3 + b) % N, i] = 35.0
        if kind == "mixed":
            pat = softmax_patterns(N, b)
            for t, name in enumerate(PATTERNS):
                S[b][:, pat == t] = cols[name][:, pat == t]
        else:
            S[b] = cols[kind]
    return S


# ----------------------------------------------------------------------------------------------------- the checks, as figures
def attention_figures(got, ref, t32, keys, hard, tol_out=TOL_OUT):
    """[(name, value, bound, torch's own figure or None)] for the quantities named in `keys`: what a test prints and asserts.  `got`
    is a kernel's (or torch float32's) result, `ref` attention_f64's, `t32` attention_torch_f32's (the bounds that are measured come
    from it).  lse: the absolute bound on hard inputs, the suite's 2e-5 relative-to-max otherwise."""
    figs = []
    for key in keys:
        if key == "lse" and hard:
            bound, terr = lse_bound(t32["S"])
            figs.append(("lse abs", float((got["lse"].detach().double().cpu() - ref["lse"]).abs().max()), bound, terr))
        elif key == "lse":
            figs.append(("lse", rel(got["lse"], ref["lse"]), 2e-5, None))
        elif key == "P":
            figs.append(("P", rel(got["P"], ref["P"]), TOL_P, None))
            bound, terr = p_elem_bound(t32["P"], ref["P"])
            figs.append(("P elem (P_ref >= 1e-3)", p_elem_err(got["P"], ref["P"]), bound, terr))
        elif key == "out":
            figs.append(("out", rel(got["out"], ref["out"]), tol_out, None))
        else:
            figs.append((key, rel(got[key], ref[key]), TOL_GRAD, None))
    return figs


def softmax_figures(P, dS, S32, P_ref, dS_ref):
    """The same for the bare column softmax: P, dS from a kernel (or torch); P_ref = softmax_col_f64(S32), dS_ref = softmax_col_bwd_f64."""
    N = S32.shape[-1]
    bound, terr = p_elem_bound(torch.softmax(S32.float(), dim=1), P_ref)
    return [("P", rel(P, P_ref), TOL_P, None),
            ("P elem (P_ref >= 1e-3)", p_elem_err(P, P_ref), bound, terr),
            ("|sum_j P - 1|", float((P.detach().double().cpu().sum(1) - 1).abs().max()), colsum_bound(N), None),
            ("dS", rel(dS, dS_ref), TOL_GRAD, None)]


def report(what, figs):
    """Print every figure as a [parity] line, then assert them all."""
    for name, val, bound, terr in figs:
        print(f"[parity] {what} {name}: {val:.3e} (bound {bound:.3e}" + (f", torch f32 {terr:.3e})" if terr is not None else ")"))
    bad = [f"{name}: {val:.3e} > {bound:.3e}" for name, val, bound, _ in figs if not val <= bound]
    assert not bad, f"{what}: " + "; ".join(bad)
