"""Float64 references, hard inputs, per-slab metrics, bounds and the case table of the GroupNorm edge tests (a helper module, not a
test file; it imports no GPU code, so the CPU tests can check the references and the table on their own).

What vd_norm.hip computes, for x [B, C, H, W] in G groups of cpg = C / G channels (one (image, group) "slab" = cpg * HW contiguous floats):

* forward:  mean, rstd = (var + eps)^-1/2 per slab (biased variance), z = (x - mean) * rstd * gamma_c + beta_c, y = z or silu(z);
* backward, GIVEN the float32 mean / rstd of the forward:  xh = (x - mean) * rstd, dz = dy * silu'(z) (or dy),
  dbeta[b, c] = sum_p dz, dgamma[b, c] = sum_p dz * xh, m1 = mean_slab(gamma dz), m2 = mean_slab(gamma dz xh),
  dx = rstd * (gamma dz - m1 - xh m2) + extra + extra2, rowsum[b, c] = sum_p dx;
* statistics only:  ss[b, c] = (gamma_c rstd, beta_c - mean gamma_c rstd).

The references evaluate exactly these formulas in float64 from the float32 operands the kernel reads.  The metric for images is per
slab -- max |a - b| / max |b| over the slab, then the worst slab -- so that a wrong group cannot hide behind a group of larger scale;
the [B, C] rows are taken per image, mean and rstd element by element."""
import torch
import torch.nn.functional as F

EPS = 1e-6
TOL_FWD = 1e-5          # the suite's tolerances (test_hip_kernels.test_groupnorm_silu): y, mean, rstd
TOL_BWD = 3e-5          # dx, the dgamma / dbeta rows, the row sums
TORCH_FACTOR = 4        # a different summation order, rsqrtf and the fast sigmoid against torch's float32
KINDS = ("plain", "offset", "outlier", "flat")
MEAN_COND_MAX = 32.0    # see make_input


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _mean_condition(x, G):
    """The worst mean|x| / |mean| over the slabs whose mean is not exactly zero: the factor by which a float32 sum's error (a few ulps
    of mean|x|, whatever the order) is magnified in the RELATIVE error of the mean."""
    xg = x.double().view(x.shape[0], G, -1)
    m, a = xg.mean(-1), xg.abs().mean(-1)
    nz = m != 0
    return float((a[nz] / m[nz].abs()).max()) if bool(nz.any()) else 0.0


def make_input(kind, B, C, H, W, G, seed=0):
    """The seeded float32 input of a kind:
    plain    randn * 2 + 0.5 (what test_groupnorm_silu uses);
    offset   randn + 100: a mean 100 times the spread (cancellation in x - mean, large shift beta - mean * scale);
    outlier  0.1 * randn with pixel (0, 0) of every channel set to 50: the variance is one pixel's;
    flat     plain with image 0 all zeros: zero variance, rstd = eps^-1/2 = 1000, a mean of exactly 0.
    On `offset` the measured torch term decides the bound of y, and for a reason that is arithmetic, not a kernel's: any float32 mean of values
    near 100 is off by about an ulp of 100 (7.6e-6; measured 1.2e-5 for the kernels, as for torch), and y = x * s + (beta - mean * s) with
    s = gamma * rstd carries that error times s, plus half an ulp of the shift itself (|shift| up to 313 for an 8-element slab, whose rstd
    reaches 2.4).  For that slab, with max |y| = 1.04, the kernels measure 3.9e-5 where torch float32 measures 2.0e-5; on the other
    slabs tested (196 elements and more) both stay under 6e-6, inside the suite's 1e-5.
    mean is checked element by element RELATIVE to itself, which no float32 summation can promise for a slab whose mean nearly cancels (an
    8-element plain slab has mean 0.5 +- 0.7).  So the seed is advanced (seed, seed + 1000, ...) until every slab has mean|x| / |mean| <=
    MEAN_COND_MAX: the floor of 1e-5 then is 5 float32 ulps of mean|x|.  This looks at the input alone."""
    assert kind in KINDS, kind
    for k in range(200):
        r = torch.randn(B, C, H, W, generator=gen(seed + 1000 * k))
        if kind == "offset":
            x = r + 100.0
        elif kind == "outlier":
            x = 0.1 * r
            x[:, :, 0, 0] = 50.0
        else:
            x = r * 2 + 0.5
            if kind == "flat":
                x[0] = 0.0
        if _mean_condition(x, G) <= MEAN_COND_MAX:
            return x
    raise AssertionError(f"no well-conditioned {kind} input for {(B, C, H, W, G)}")


def make_params(C, seed=1):
    """(gamma, beta) float32: randn * 0.5 + 1, randn * 0.5 (as test_groupnorm_silu)."""
    return torch.randn(C, generator=gen(seed)) * 0.5 + 1, torch.randn(C, generator=gen(seed + 1)) * 0.5


def make_grads(shape, seed=3):
    """(dy, extra, extra2) float32 randn."""
    return tuple(torch.randn(shape, generator=gen(seed + i)) for i in range(3))


# ------------------------------------------------------------------------------------------------------------- float64 references
def _bc(v, B, G, cpg):
    """per-(image, group) values [B * G] or [B, G] -> [B, C, 1, 1]"""
    return v.reshape(B, G, 1).expand(B, G, cpg).reshape(B, G * cpg, 1, 1)


def stats_f64(x, G, eps=EPS):
    """(mean, rstd) [B * G] in float64 from the float32 input."""
    xg = x.double().view(x.shape[0], G, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    return mean.flatten(), (var + eps).rsqrt().flatten()


def fwd_f64(x, gamma, beta, G, silu, eps=EPS):
    """(y, mean, rstd) in float64."""
    B, C = x.shape[:2]
    mean, rstd = stats_f64(x, G, eps)
    z = (x.double() - _bc(mean, B, G, C // G)) * _bc(rstd, B, G, C // G) * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1)
    return (z * torch.sigmoid(z) if silu else z), mean, rstd


def ss_f64(x, gamma, beta, G, eps=EPS):
    """ss [B, C, 2] of vd_groupnorm_stats in float64."""
    B, C = x.shape[:2]
    mean, rstd = stats_f64(x, G, eps)
    sc = gamma.double().view(1, C) * _bc(rstd, B, G, C // G).view(B, C)
    return torch.stack([sc, beta.double().view(1, C) - _bc(mean, B, G, C // G).view(B, C) * sc], -1)


def bwd_f64(dy, x, mean, rstd, gamma, beta, G, silu, extra=None, extra2=None):
    """The backward formula in float64 from the mean / rstd [B * G] the kernel is given (float32 in the GPU tests: the reference reads
    what the kernel reads) -> (dx + extra + extra2, dgamma rows [B, C], dbeta rows [B, C], row sums of that dx [B, C])."""
    B, C, H, W = x.shape
    cpg = C // G
    ga, be = gamma.double().view(1, C, 1, 1), beta.double().view(1, C, 1, 1)
    m, r = _bc(mean.double(), B, G, cpg), _bc(rstd.double(), B, G, cpg)
    xh = (x.double() - m) * r
    dz = dy.double()
    if silu:
        z = xh * ga + be
        sg = torch.sigmoid(z)
        dz = dz * (sg * (1 + z * (1 - sg)))
    dbeta, dgamma = dz.sum((2, 3)), (dz * xh).sum((2, 3))
    n = cpg * H * W
    m1 = _bc((dz * ga).view(B, G, -1).sum(-1) / n, B, G, cpg)
    m2 = _bc((dz * ga * xh).view(B, G, -1).sum(-1) / n, B, G, cpg)
    dx = r * (dz * ga - m1 - xh * m2)
    for e in (extra, extra2):
        if e is not None:
            dx = dx + e.double()
    return dx, dgamma, dbeta, dx.sum((2, 3))


def partial_stats_f64(part, gamma, beta, HW, G, eps=EPS):
    """vd_groupnorm_stats_from_partials in float64: part [B, tiles, C, 2] = per-tile (sum, sum of squares) of every channel
    -> (ss [B, C, 2], mean [B * G], rstd [B * G]); the variance is E[x^2] - mean^2, clamped at 0, as the kernel forms it."""
    B, _, C, _ = part.shape
    cpg = C // G
    s = part.double().sum(1).view(B, G, cpg, 2).sum(2)                              # [B, G, 2]
    n = cpg * HW
    mean = s[..., 0] / n
    rstd = ((s[..., 1] / n - mean * mean).clamp(min=0) + eps).rsqrt()
    sc = gamma.double().view(1, C) * _bc(rstd, B, G, cpg).view(B, C)
    ss = torch.stack([sc, beta.double().view(1, C) - _bc(mean, B, G, cpg).view(B, C) * sc], -1)
    return ss, mean.flatten(), rstd.flatten()


# ------------------------------------------------------------------------------------------------------ plain torch float32
def torch_f32_fwd(x, gamma, beta, G, silu, eps=EPS):
    """(y, mean, rstd) as plain torch float32 computes them."""
    y = F.group_norm(x, G, gamma, beta, eps)
    xg = x.view(x.shape[0], G, -1)
    return (F.silu(y) if silu else y), xg.mean(-1).flatten(), (xg.var(-1, unbiased=False) + eps).rsqrt().flatten()


def torch_f32_bwd(dy, x, gamma, beta, G, silu, extra=None, extra2=None, eps=EPS):
    """(dx + extra + extra2, dgamma rows, dbeta rows, row sums) from float32 autograd, image by image (the rows are per image)."""
    dxs, dgs, dbs = [], [], []
    for b in range(x.shape[0]):
        xb = x[b:b + 1].clone().requires_grad_()
        g_, b_ = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        y = F.group_norm(xb, G, g_, b_, eps)
        (F.silu(y) if silu else y).backward(dy[b:b + 1])
        dxs.append(xb.grad)
        dgs.append(g_.grad)
        dbs.append(b_.grad)
    dx = torch.cat(dxs)
    for e in (extra, extra2):
        if e is not None:
            dx = dx + e
    return dx, torch.stack(dgs), torch.stack(dbs), dx.sum((2, 3))


# -------------------------------------------------------------------------------------------------------------------- metrics
def _worst_ratio(num, den):
    """max over entries of num / den, where an entry with den == 0 counts 0 if num == 0 too (an exactly-zero reference reproduced
    exactly) and inf otherwise."""
    num, den = num.double(), den.double()
    ok = den > 0
    r = torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))))
    return float(r.max())


def slab_err(a, b, G):
    """Images [B, C, H, W]: max |a - b| / max |b| per (image, group) slab, the worst slab."""
    B = b.shape[0]
    a, b = a.detach().double().cpu().reshape(B, G, -1), b.detach().double().cpu().reshape(B, G, -1)
    return _worst_ratio((a - b).abs().amax(-1), b.abs().amax(-1))


def row_err(a, b):
    """Rows [B, C]: max |a - b| / max |b| per image, the worst image."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return _worst_ratio((a - b).abs().amax(-1), b.abs().amax(-1))


def elem_err(a, b):
    """mean / rstd: the worst |a - b| / |b| element by element."""
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return _worst_ratio((a - b).abs(), b.abs())


def bound(floor, torch_err):
    """max(the suite's tolerance, TORCH_FACTOR x what plain torch float32 loses on the same case under the same metric)."""
    return max(floor, TORCH_FACTOR * torch_err)


class Reference:
    """Everything one (case, kind, silu) needs, computed once on the CPU: inputs, float64 results, torch float32's errors and the bounds.
    errs / bounds are dicts over the outputs: y, mean, rstd; then per residual variant v in (0 none, 1 extra, 2 extra + extra2):
    dx{v}, dgamma, dbeta (the same rows for every variant) and rowsum (variant 2)."""

    def __init__(self, dims, kind, silu, seed=0):
        B, C, H, W, G = dims
        self.dims, self.kind, self.silu, self.G = dims, kind, silu, G
        self.x = make_input(kind, B, C, H, W, G, seed)
        self.gamma, self.beta = make_params(C)
        self.dy, self.extra, self.extra2 = make_grads(self.x.shape)
        self.y, self.mean, self.rstd = fwd_f64(self.x, self.gamma, self.beta, G, silu)
        self.mean32, self.rstd32 = self.mean.float(), self.rstd.float()          # what the backward kernel is fed
        ty, tm, tr = torch_f32_fwd(self.x, self.gamma, self.beta, G, silu)
        self.torch_err = {"y": slab_err(ty, self.y, G), "mean": elem_err(tm, self.mean), "rstd": elem_err(tr, self.rstd)}
        self.floor = {"y": TOL_FWD, "mean": TOL_FWD, "rstd": TOL_FWD}
        self.bwd = {}
        if C // G > 64:                                                        # the backward refuses more than 64 channels per group
            return
        for v, (e1, e2) in enumerate(((None, None), (self.extra, None), (self.extra, self.extra2))):
            dx, dg, db, rs = bwd_f64(self.dy, self.x, self.mean32, self.rstd32, self.gamma, self.beta, G, silu, e1, e2)
            tdx, tdg, tdb, trs = torch_f32_bwd(self.dy, self.x, self.gamma, self.beta, G, silu, e1, e2)
            self.bwd[v] = (dx, dg, db, rs)
            self.torch_err[f"dx{v}"] = slab_err(tdx, dx, G)
            self.floor[f"dx{v}"] = TOL_BWD
            if v == 0:
                self.torch_err.update(dgamma=row_err(tdg, dg), dbeta=row_err(tdb, db))
                self.floor.update(dgamma=TOL_BWD, dbeta=TOL_BWD)
            if v == 2:
                self.torch_err["rowsum"] = row_err(trs, rs)
                self.floor["rowsum"] = TOL_BWD

    def bound(self, what):
        """(bound, torch float32's own error) of an output."""
        return bound(self.floor[what], self.torch_err[what]), self.torch_err[what]

    def check(self, what, err, label=""):
        """Print the [parity] line (kernel error, torch's error, bound), then assert."""
        bnd, terr = self.bound(what)
        print(f"[parity] gn {self.dims} {self.kind} silu={int(self.silu)} {label} {what}: err={err:.3e} torch_f32={terr:.3e} bound={bnd:.3e}")
        assert err <= bnd, f"{self.dims} {self.kind} silu={self.silu} {label} {what}: {err:.3e} > {bnd:.3e} (torch float32: {terr:.3e})"


# ----------------------------------------------------------------------------------------------------------------- case table
def _fw(n):
    return f"gn_fwd_wave_kernel<{n}>"


def _fr(nv, nth=256):
    return f"gn_fwd_reg_kernel<{nv}, {nth}>"


def _bw(n):
    return f"gn_bwd_wave_kernel<{n}>"


def _br(nv, nth):
    return f"gn_bwd_reg_kernel<{nv}, {nth}>"


def _fc(nv):
    return f"gn_chunk1_fwd_kernel<{nv}>"


FWD_GENERIC, BWD_GENERIC, BWD_CHUNK1 = "gn_fwd_kernel", "gn_bwd_kernel", "gn_chunk1_bwd_kernel<8>"
FWD_TWO = "gn_chunk_stats_kernel<{}>+gn_chunk_apply_kernel"
BWD_TWO = "gn_chunk_bwd_stats_kernel+gn_chunk_bwd_apply_kernel"
ROWSUM = "gn_chunk_rowsum_kernel"               # the chunked backward adds it when row sums are asked for
FROM_PARTIALS = "gn_stats_from_part_kernel"
REFUSED = None

# (B, C, H, W, G): (forward kernel, its chunks per group S, backward kernel, its S) as ops.groupnorm_plan must report them when the
# tensors are 16-byte aligned and the workspace is what ops passes.  slab = C / G * H * W floats, L = H * W / 4 float4 per channel.
CASES = {
    (3, 6, 2, 2, 3): (_fw(1), 0, _bw(1), 0),                  # slab 8, L = 1; 9 slabs: the last workgroup holds one (gid >= total)
    (3, 3, 4, 4, 3): (_fw(1), 0, _bw(1), 0),                  # one channel per group; 9 slabs
    (1, 4, 8, 8, 1): (_fw(1), 0, _bw(1), 0),                  # slab 256: the upper end of <1>; one slab in a four-slab workgroup
    (3, 2, 16, 16, 1): (_fw(2), 0, _br(1, 256), 0),           # slab 512: the upper end of <2>; L = 64 leaves the one-wave backward
    (2, 6, 12, 12, 3): (_fw(2), 0, BWD_GENERIC, 0),           # slab 288, L = 36: not a power of two
    (3, 10, 8, 8, 2): (_fw(2), 0, _bw(2), 0),                 # slab 320 = 5 channels of L = 16: a second row with 16 of 64 lanes; 6 slabs
    (1, 16, 8, 8, 1): (_fw(4), 0, _bw(4), 0),                 # slab 1024: the upper end of the one-wave kernels
    (1, 64, 4, 4, 1): (_fw(4), 0, _bw(4), 0),                 # 64 channels per group in one wave
    (2, 1, 32, 32, 1): (_fw(4), 0, _br(1, 256), 0),           # slab 1024 as one channel, L = 256
    (2, 1, 2, 514, 1): (_fr(2), 0, BWD_GENERIC, 0),           # slab 1028: one float4 over a full row of 256; L = 257
    (2, 2, 32, 32, 1): (_fr(2), 0, _br(2, 256), 0),           # slab 2048: the upper end of <2>
    (2, 2, 2, 1022, 2): (_fr(2), 0, BWD_GENERIC, 0),          # slab 2044, non-square: the last row of <2> one float4 short
    (2, 2, 2, 1026, 2): (_fr(4), 0, BWD_GENERIC, 0),          # slab 2052: one float4 past <2>
    (1, 4, 32, 32, 1): (_fr(4), 0, _br(4, 256), 0),           # slab 4096: the upper end of <4>
    (1, 1, 2, 2050, 1): (_fr(8), 0, BWD_GENERIC, 0),          # slab 4100: one float4 past <4>
    (1, 64, 8, 8, 1): (_fr(4), 0, _br(4, 256), 0),            # 64 channels per group with L = 16 in the block kernel
    (1, 8, 32, 32, 1): (_fr(8), 0, _br(4, 512), 0),           # slab 8192
    (1, 12, 32, 32, 1): (_fr(12), 0, _br(6, 512), 0),         # slab 12288
    (1, 14, 32, 32, 1): (_fr(7, 512), 0, _br(7, 512), 0),     # slab 14336
    (1, 64, 16, 16, 1): (_fr(7, 1024), 0, _br(7, 1024), 0),   # slab 16384: 64 channels per group with L = 64
    (2, 7, 64, 64, 1): (_fr(7, 1024), 0, _br(7, 1024), 0),    # slab 28672: GN_REG_MAX exactly
    (2, 64, 16, 32, 1): (_fc(8), 64, BWD_CHUNK1, 64),         # slab 32768 in 64 chunks of 128 float4: fewer than the 256 threads
    (1, 32, 34, 34, 1): (_fc(8), 32, BWD_CHUNK1, 32),         # slab 36992: chunks of 289 float4
    (1, 7, 64, 68, 1): (_fc(8), 7, BWD_CHUNK1, 7),            # slab 30464: an odd number of chunks
    (1, 2, 128, 128, 1): (_fc(16), 2, BWD_CHUNK1, 4),         # slab 32768: forward chunks of 16384 floats, backward of 8192
    (1, 4, 96, 96, 1): (_fc(16), 4, BWD_CHUNK1, 8),           # slab 36864: 2304 float4 in <16>, partly filled
    (1, 2, 124, 124, 1): (_fc(16), 2, BWD_CHUNK1, 4),         # slab 30752: chunks of 3844 / 1922 float4
    (1, 4, 20, 461, 1): (FWD_GENERIC, 0, BWD_GENERIC, 0),     # slab 36880: the backward's halving ends at 4610 floats, so no workspace at all
    (3, 12, 7, 7, 3): (FWD_GENERIC, 0, BWD_GENERIC, 0),       # H * W = 49: the scalar branches
    (2, 8, 28, 28, 2): (_fr(4), 0, BWD_GENERIC, 0),           # slab 3136, L = 196 (MNIST-sized): the backward's vector branch
    (1, 130, 4, 4, 2): (_fr(2), 0, REFUSED, 0),               # 65 channels per group: forward only
    (1, 40, 256, 256, 1): (FWD_GENERIC, 0, BWD_GENERIC, 0),   # slab 2.6 M (10 MB): the backward would need 320 > 256 chunks, so no workspace
}

# one case per kernel family for the four input kinds.  None with one channel per group: the dx of such a group sums to zero, so its row
# sums are the residuals' alone, while on a flat image the terms are 1000 times larger -- a cancelling sum, whatever the kernel
KIND_CASES = ((3, 6, 2, 2, 3), (1, 64, 4, 4, 1), (2, 2, 32, 32, 1), (1, 14, 32, 32, 1), (2, 7, 64, 64, 1), (2, 64, 16, 32, 1),
              (1, 2, 128, 128, 1), (3, 12, 7, 7, 3), (2, 8, 28, 28, 2))
# two register-sized cases and a chunkable one (B = 2 each) for the unaligned runs
UNALIGNED_CASES = ((2, 2, 32, 32, 1), (2, 7, 64, 64, 1), (2, 64, 16, 32, 1))
# vd_groupnorm_stats beyond the table: 256 channels per group in one wave (four trips of its ss loop) and in the block kernel
STATS_EXTRA = {(2, 256, 2, 2, 1): _fw(4), (1, 256, 4, 4, 1): _fr(4)}


def is_chunked(name):
    return name is not None and name.startswith("gn_chunk")


def stats_cases():
    """Table cases vd_groupnorm_stats accepts (at most 256 channels per group, an aligned slab of at most 28672 floats): it takes the forward's kernel."""
    out = {d: names[0] for d, names in CASES.items() if names[0].startswith(("gn_fwd_wave", "gn_fwd_reg")) and d[1] // d[4] <= 256}
    out.update(STATS_EXTRA)
    return out


def child_cases():
    """With VD_GN_CHUNK1_OFF=1 VD_GN_WAVE_OFF=1: the chunked cases take the two-launch kernels, the one-wave cases the smallest block
    kernels -> {dims: (forward, S, backward, S)} of the cases that change."""
    out = {}
    for d, (f, fs, b, bs) in CASES.items():
        f2 = FWD_TWO.format(f[f.index("<") + 1:-1]) if is_chunked(f) else (_fr(1) if f.startswith("gn_fwd_wave") else f)
        b2 = BWD_TWO if is_chunked(b) else (_br(1, 256) if b is not None and b.startswith("gn_bwd_wave") else b)
        if (f2, b2) != (f, b):
            out[d] = (f2, fs, b2, bs)
    return out


def all_expected_names():
    """Every kernel of vd_norm.hip a case of the edge tests launches: the default run, the child run, the statistics entry points."""
    names = {ROWSUM, FROM_PARTIALS}
    for table in (CASES, child_cases()):
        for f, _, b, _ in table.values():
            names.update(f.split("+"))
            if b is not None:
                names.update(b.split("+"))
    names.update(stats_cases().values())
    return names
