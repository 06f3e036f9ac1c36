"""The elementwise hot-path kernels of vd_elem.hip at their grid caps, tails and flags, against the references of tests/elem_ref.py.

Bit-exact (torch.equal) against float32 sequences: q-sample (VP, VE), lincomb (1 .. 6 sources), postprocess (both layouts), rowscale, add_strided /
add_flat (the vector kernel and every way of falling to the scalar one, on the same data), scale_, sched_step (the whole flag grid, x0_out, and
the Philox contract: in-kernel noise == the explicit z of ops.randn), randn's slice property, adam_step (p, m AND v after each of three steps,
five configurations, the skip path) and adam_ema_step at the cap.  Against float64 with derived bounds, printed as [parity] lines with value /
bound: l2norm_sq, the three losses, batch_l2norm, both embeddings, SiLU forward and backward elementwise, and randn against Philox4x32-10
restated in integer arithmetic.  The references, the inputs and "plain torch float32 passes these very bounds" are pinned in
test_elem_ref_cpu.py.

Every output sits in an exact-size buffer between sentinel words that must survive each launch; every read-only float input is followed by
NaN (and, where the wrapper takes a batch stride, surrounded by it).

Launches reached (egrid() arithmetic: ceil(n / (256 per_thread)) blocks, at most 4096; T = 2^20 threads at the cap).  The sizes of
elem_ref.py give: 1 / 2 / 4096 blocks with a ragged wrap for the per-element kernels (T + 257 items -> 4098 blocks asked, 4096 given, 257
threads go round twice); randn / sched_step at T + 301 quads likewise; scale_ at 4T + 1027 (egrid(n, 4): 4098 -> 4096, every thread four or five
rounds); adam at 8T + 2051 (egrid(n, 8): 4098 -> 4096 blocks for 2T + 512 items, three rounds for the first 512 threads, and block 0's 3-float
tail); l2norm_sq there 2049 -> 1024 blocks (all 1024 partial slots written, finish_sum_kernel reads them all); the loss at 4 x 65536 exactly
1024 blocks with no wrap and at 5 x 66603 1024 blocks with a wrap (1301 asked)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elem_ref as E  # noqa: E402
import exact_ref as X  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402

DEV = X.DEV
T = E.T
g = E.g
ADAM = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def src(t):
    """A contiguous device copy of the float tensor t followed by NaN."""
    v, _ = X.nan_vector(t.detach().float().flatten())
    return v.view(t.shape)


class Out:
    """An exact-size guarded output of the given shape (GuardedFlat), NaN-filled (or `fill`) before the launch; pre: floats of sentinel in front
    (a multiple of 4 keeps the 16-byte alignment)."""

    def __init__(self, *shape, fill=float("nan"), pre=64, init=None):
        self.g = X.GuardedFlat(math.prod(shape), pre=pre, fill=fill)
        self.t = self.g.view.view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ok(self, what):
        assert self.g.intact(), f"{what}: wrote outside its output"
        return self.t

    def cpu(self, what):
        return self.ok(what).cpu()


def unchanged(view, ref, what):
    assert torch.equal(view.cpu(), ref.detach().float().view(view.shape)), f"{what}: a read-only input was written"


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------- q-sample
@pytest.mark.parametrize("B,chw", E.QSAMPLE_SHAPES)
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_qsample_bit_exact_beyond_the_cap(sde, B, chw):
    Tn = 1000
    x0, R, eps = (torch.randn(B, chw, generator=g(i)) for i in range(3))
    R[::2] = 0
    tabs = [torch.rand(Tn, generator=g(10 + i)) * 2 - (0.5 if i == 3 else 0.0) for i in range(4)]            # a, s, step, coef
    t = torch.tensor([Tn - 1, 0, Tn - 1, 17, 17][:B])                                                        # 0, T - 1 and repeats
    ta = tabs[0] if sde == "vp" else None
    xt_ref, y_ref = E.qsample_f32(x0, R, eps, t, ta, tabs[1], tabs[2], tabs[3])
    d = [src(v) for v in (x0, R, eps)]
    dt = [None if ta is None else src(ta)] + [src(v) for v in tabs[1:]]
    xt, y = Out(B, chw), Out(B, chw)
    ops.qsample_backdoor(*d, t.to(DEV), *dt, xt.t, y.t)
    what = f"qsample {sde} B={B} chw={chw}"
    assert torch.equal(xt.cpu(what), xt_ref) and torch.equal(y.cpu(what), y_ref), what
    for v, r in zip(d, (x0, R, eps)):
        unchanged(v, r, what)


# --------------------------------------------------------------------------------------------- lincomb, postprocess, rowscale, scale_
@pytest.mark.parametrize("n", E.SIZES_SCALAR)
def test_lincomb_one_to_six_sources(n):
    xs = [torch.randn(n, generator=g(i)) for i in range(6)]
    cf = [0.5, -1.25, 2.0, 0.3, -0.7, 1.1]
    ds = [src(x) for x in xs]
    for k in range(1, 7):
        out = Out(n)
        ops.lincomb(out.t, ds[:k], cf[:k])
        assert torch.equal(out.cpu(f"lincomb n={n} n_src={k}"), E.lincomb_f32(xs[:k], cf[:k])), (n, k)
    for v, r in zip(ds, xs):
        unchanged(v, r, "lincomb source")


@pytest.mark.parametrize("B,C,H,W", E.POSTPROCESS_SHAPES)
def test_postprocess_both_layouts(B, C, H, W):
    x = torch.randn(B, C, H, W, generator=g(0)) * 1.5
    xd = src(x)
    for nhwc in (False, True):
        out = Out(*((B, H, W, C) if nhwc else (B, C, H, W)))
        ops.postprocess(xd, out.t, 0.5, 0.5, 0.0, 1.0, nhwc)
        assert torch.equal(out.cpu(f"postprocess {(B, C, H, W)} nhwc={nhwc}"), E.postprocess_f32(x, 0.5, 0.5, 0.0, 1.0, nhwc)), (B, C, H, W, nhwc)
    unchanged(xd, x, "postprocess x")


@pytest.mark.parametrize("n", E.SIZES_SCALAR)
def test_rowscale_multiply_and_divide(n):
    B, inner = E.rows(n)
    x, s = torch.randn(B, inner, generator=g(0)), torch.randn(B, generator=g(1)) + 2.5
    xd, sd = src(x), src(s)
    for divide in (False, True):
        out = Out(B, inner)
        ops.rowscale(xd, sd, out.t, divide=divide)
        assert torch.equal(out.cpu(f"rowscale n={n} divide={divide}"), E.rowscale_f32(x, s, divide)), (n, divide)
    unchanged(xd, x, "rowscale x"), unchanged(sd, s, "rowscale s")


@pytest.mark.parametrize("n", E.SIZES_SCALE)
def test_scale_in_place_and_zero_over_nan(n):
    x = torch.randn(n, generator=g(0))
    out = Out(n, init=x)
    ops.scale_(out.t, 0.37)
    assert torch.equal(out.cpu(f"scale_ n={n}"), E.scale_f32(x, 0.37))
    x[::3], x[-1] = float("nan"), float("-inf")
    x[n // 2] = float("inf")
    out = Out(n, init=x)
    ops.scale_(out.t, 0.0)
    assert bool((out.ok(f"scale_ n={n} alpha=0").view(torch.int32) == 0).all()), "alpha = 0 must store +0 everywhere"


# ------------------------------------------------------------------------------------------------------------ add_strided / add_flat
# (B, C, H) of [B, C, H, 1] images, inner = C H: one f32x4 item; five images of 257 items; T + 257 items in three images (4T + 1028 floats)
ADD_VEC_SHAPES = ((1, 4, 1), (5, 4, 257), (3, 4, (T + 257) // 3))
# the same with inner % 4 != 0: E.SIZES_SCALAR floats in all
ADD_SCALAR_SHAPES = ((1, 1, 1), (1, 257, 1), (3, (T + 257) // 3, 1))


def _add_case(s, d0, dst_pre, dst_post, src_pre, src_post, what):
    """dst (+)= src on guarded buffers laid out by the given channel paddings -> [result with accumulate off, on] (CPU)."""
    B, C, H, _ = s.shape
    sd = X.nan_slice(s, pre=src_pre, post=src_post)
    go = X.GuardedOut(B, C, H, 1, pre=dst_pre, post=dst_post)
    res = []
    for acc in (False, True):
        dst = go.fresh(d0 if acc else None)
        ops.add_strided(dst, sd, accumulate=acc)
        assert go.intact(), f"{what} accumulate={acc}: wrote outside its output slice"
        res.append(dst.cpu())
        assert torch.equal(res[-1], E.add_f32(d0, s, acc)), f"{what} accumulate={acc}"
    unchanged(sd, s, what)
    return res


@pytest.mark.parametrize("B,C,H", ADD_VEC_SHAPES)
def test_add_strided_vector_kernel_and_every_fall_to_the_scalar_one(B, C, H):
    """H is odd, so a channel padding that is no multiple of 4 breaks exactly one of the vector kernel's conditions: dst / src padded by (4, 4)
    channels: the vector kernel; dst (4, 1) / src (4, 1): a batch stride of 9 H floats (one image: its stride is never used, the vector kernel
    stays); dst (1, 3) / src (1, 3): the view starts H floats, i.e. 1 or 3 floats, past a 16-byte boundary.  Same data, same bits."""
    assert H % 2 == 1 and C % 4 == 0
    s, d0 = torch.randn(B, C, H, 1, generator=g(0)), torch.randn(B, C, H, 1, generator=g(1))
    what = f"add_strided B={B} inner={C * H}"
    base = _add_case(s, d0, 4, 4, 4, 4, what + " vector")
    for name, pads in (("dst stride % 4", (4, 1, 4, 4)), ("src stride % 4", (4, 4, 4, 1)), ("dst misaligned", (1, 3, 4, 4)), ("src misaligned", (4, 4, 1, 3))):
        got = _add_case(s, d0, *pads, f"{what} {name}")
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), name


@pytest.mark.parametrize("B,C,H", ADD_SCALAR_SHAPES)
def test_add_strided_scalar_kernel_inner_not_a_multiple_of_four(B, C, H):
    s, d0 = torch.randn(B, C, H, 1, generator=g(0)), torch.randn(B, C, H, 1, generator=g(1))
    assert (C * H) % 4 != 0
    _add_case(s, d0, 4, 4, 8, 8, f"add_strided B={B} inner={C * H} scalar")


@pytest.mark.parametrize("n", E.SIZES_VEC + E.SIZES_SCALAR)
def test_add_flat_vector_and_scalar(n):
    s, d0 = torch.randn(n, generator=g(0)), torch.randn(n, generator=g(1))
    sd = src(s)
    res = []
    for pre in (64, 65):                                         # 65: the output starts one float past a 16-byte boundary -> the scalar kernel
        for acc in (False, True):
            out = Out(n, pre=pre, init=d0 if acc else None)
            ops.add_flat(out.t, sd, accumulate=acc)
            res.append(out.cpu(f"add_flat n={n} pre={pre} accumulate={acc}"))
            assert torch.equal(res[-1], E.add_f32(d0, s, acc)), (n, pre, acc)
    assert torch.equal(res[0], res[2]) and torch.equal(res[1], res[3])
    unchanged(sd, s, "add_flat src")


# ------------------------------------------------------------------------------------------------------------------ sched_step, randn
def _randn(n, seed, off):
    out = Out(n)
    ops.randn(out.t, seed, off)
    return out.ok(f"randn n={n} seed={seed} offset={off}")


@pytest.mark.parametrize("n", E.SIZES_QUADS)
def test_sched_step_flag_grid_and_philox_contract(n):
    """{clip 0, 1} x {c_e 0, != 0} x {c_z 0, != 0} x {x0_out None, given}: out and x0_out bit-equal to the float32 sequence; c_z = 0 does not
    depend on seed, offset or z (a NaN z is never read); c_z != 0 with z = None is bit-equal to the explicit z = ops.randn(n, seed, offset)."""
    x, e, z = (torch.randn(n, generator=g(i)) * 1.5 for i in range(3))
    xd, ed, zd, znan = src(x), src(e), src(z), torch.full((n,), float("nan"), device=DEV)
    seed, off = 2 ** 32 + 7, 2 ** 32 - 5
    zr = _randn(n, seed, off)
    zr_cpu = zr.cpu()
    co = dict(c_eps=0.6, c_div=0.8, c_x0=0.45, c_x=0.55)
    for clip in (0.0, 1.0):
        for c_e in (0.0, 0.3):
            for c_z in (0.0, 0.25):
                ref, x0_ref = E.sched_step_f32(x, e, z, co["c_eps"], co["c_div"], clip, co["c_x0"], co["c_x"], c_e, c_z)
                refr, _ = E.sched_step_f32(x, e, zr_cpu, co["c_eps"], co["c_div"], clip, co["c_x0"], co["c_x"], c_e, c_z)
                for want_x0 in (False, True):
                    what = f"sched_step n={n} clip={clip} c_e={c_e} c_z={c_z} x0_out={want_x0}"
                    runs = [(zd, 0, 0, ref), (None, seed, off, refr)] if c_z else [(None, 1, 2, ref), (None, seed, off, ref), (znan, 0, 0, ref)]
                    for zz, sd_, of_, want in runs:
                        out, x0 = Out(n), Out(n)
                        ops.sched_step(xd, ed, out.t, clip=clip, c_e=c_e, c_z=c_z, z=zz, x0_out=x0.t if want_x0 else None, seed=sd_, offset=of_, **co)
                        assert torch.equal(out.cpu(what), want), what + (" (in-kernel noise)" if zz is None and c_z else "")
                        if want_x0:
                            assert torch.equal(x0.cpu(what + " x0"), x0_ref), what + " x0"
                        else:
                            assert bool(torch.isnan(x0.ok(what + " x0")).all()), what + ": x0_out = None was written"
    unchanged(xd, x, "sched_step x"), unchanged(ed, e, "sched_step eps"), unchanged(zd, z, "sched_step z")


@pytest.mark.parametrize("n", E.SIZES_QUADS)
@pytest.mark.parametrize("off", [1, 1000])
def test_randn_offset_is_a_slice_of_the_stream(off, n):
    for seed in (1234, 2 ** 32 + 7):
        assert torch.equal(_randn(n, seed, off), _randn(4 * off + n, seed, 0)[4 * off:]), (seed, off, n)


@pytest.mark.parametrize("n,seed,off", [(1023, s, o) for s, o in E.RANDN_IDENTITY] + [(E.SIZES_QUADS[-1], 1234, 0)])
def test_randn_is_philox4x32_10(n, seed, off):
    """An identity gate, 1e-3 absolute on every element: a wrong word of the stream moves a value by O(1), the fast log and sincos by ~1e-5 |z|."""
    got = _randn(n, seed, off).cpu().double()
    E.report(f"randn seed={seed} offset={off} n={n}", [("|z - randn_ref|", float((got - E.randn_ref(n, seed, off)).abs().max()), E.TOL_RANDN)])


# ------------------------------------------------------------------------------------------------------------------------------ Adam
class AdamState:
    """p, m, v in exact-size guarded buffers; the gradient followed by NaN; partial filled to the brim (1024) and a one-float norm."""

    def __init__(self, n, p0, m0, v0):
        self.n = n
        self.p, self.m, self.v = Out(n, init=p0), Out(n, init=m0), Out(n, init=v0)
        self.partial, self.nsq = Out(1024), Out(1)

    def norm_sq(self, gd):
        ops.l2norm_sq(gd, self.partial.t, self.nsq.t)
        self.partial.ok("l2norm_sq partial")
        return self.nsq.ok("l2norm_sq out")

    def cpu(self, what):
        return tuple(b.cpu(f"{what} {k}") for k, b in zip("pmv", (self.p, self.m, self.v)))


def _unit(n, seed, norm):
    x = torch.randn(n, generator=g(seed))
    return x * (norm / float(x.double().norm()))


def _adam_run(n, config):
    """Three steps of `config` -> nothing; asserts p, m, v == adam_emulate bit for bit after each step."""
    p0 = torch.randn(n, generator=g(0))
    m0, v0, step0, inv_scale, use_norm, weights = torch.zeros(n), torch.zeros(n), 1, 1.0, True, True
    norms = (3.0, 0.5, 0.25)                                     # the first step is clipped (norm 3 > max_norm 1), the others are not
    if config == "none":
        use_norm = False
    elif config == "scaled":
        inv_scale = 1.0 / 1024
    elif config == "late":
        step0, m0, v0 = 100000, torch.randn(n, generator=g(1)) * 0.01, torch.rand(n, generator=g(2)) * 1e-4
    elif config == "trigger":
        weights = False
    st = AdamState(n, p0, m0, v0)
    p, m, v = p0, m0, v0
    for i in range(3):
        gr = _unit(n, 10 + i, norms[i]) * (1024.0 if config == "scaled" else 1.0)
        gd = src(gr)
        gs = E.grad_scale(float(st.norm_sq(gd)) if use_norm else None, 1.0, inv_scale)
        assert gs is not None
        if use_norm and n > 1:
            assert (float(gs) < inv_scale) == (i == 0), "the first step is clipped, the others are not"
        epoch = ops.WEIGHTS_EPOCH
        ops.adam_step(st.p.t, gd, st.m.t, st.v.t, st.nsq.t if use_norm else None, 1.0, inv_scale, step=step0 + i, weights=weights, **ADAM)
        assert ops.WEIGHTS_EPOCH == epoch + int(weights)
        p, m, v = E.adam_emulate(p, gr, m, v, gs, step=step0 + i, **ADAM)
        what = f"adam_step {config} n={n} step {step0 + i}"
        gp, gm, gv = st.cpu(what)
        unchanged(gd, gr, what + " g")
        dm, dv, dp = (int((a != b).sum()) for a, b in ((gm, m), (gv, v), (gp, p)))
        print(f"[parity] {what}: elements that differ from the float32 emulation: m {dm}, v {dv}, p {dp} of {n}")
        assert dm == 0 and dv == 0, what + ": m / v are individually rounded + - x and must be exact"
        assert dp == 0, what + ": p"


@pytest.mark.parametrize("n", E.SIZES_ADAM[:-1])
@pytest.mark.parametrize("config", ["clip", "none", "scaled", "late", "trigger"])
def test_adam_step_p_m_v_bit_exact(config, n):
    """clip: a clipped first step, then unclipped ones; none: norm_sq = None; scaled: inv_scale = 1 / 1024 on gradients scaled up by 1024; late:
    step = 100 000 (both bias corrections saturated) on non-zero moments; trigger: weights = False leaves ops.WEIGHTS_EPOCH alone.  The gradient
    scale of the emulation is grad_scale of the device's own norm_sq, read back.

    Observed on an MI355X: m, v and p all come out bit for bit, at every size and step: the device's sqrtf and divisions are the correctly
    rounded sequences.  The one disagreement ever seen (p alone, 1 element in 4000) was the host's: torch.sqrt of a float32 CPU tensor is not
    correctly rounded, so adam_emulate takes the root in float64 and rounds it.  p is therefore gated exactly, like m and v."""
    _adam_run(n, config)


def test_adam_step_p_m_v_bit_exact_at_the_cap():
    """8T + 2051: egrid(n, 8) capped at 4096 blocks, three grid-stride rounds, block 0 of the capped grid does the 3-float tail."""
    _adam_run(E.SIZES_ADAM[-1], "clip")


def _skip_case(n, gr, nsq_value, what):
    """Two calls with a non-finite norm: p, m, v bit-unchanged, the counter at exactly 2; a third with skipped = None: no fault, unchanged."""
    p0, m0, v0 = torch.randn(n, generator=g(0)), torch.randn(n, generator=g(1)) * 0.01, torch.rand(n, generator=g(2)) * 1e-4
    st = AdamState(n, p0, m0, v0)
    gd = src(gr)
    if nsq_value is None:
        nsq = st.norm_sq(gd)
        assert not math.isfinite(float(nsq)), what + ": the norm must come out non-finite"
    else:
        nsq = st.nsq.t.fill_(nsq_value)
    assert E.grad_scale(float(nsq), 1.0, 1.0) is None
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k, skipped in enumerate((count, count, None)):
        ops.adam_step(st.p.t, gd, st.m.t, st.v.t, nsq, 1.0, 1.0, step=1 + k, skipped=skipped, **ADAM)
    torch.cuda.synchronize()
    assert int(count) == 2, f"{what}: counted {int(count)} skips for two counted calls"
    for got, want, name in zip(st.cpu(what), (p0, m0, v0), "pmv"):
        assert bits_equal(got, want), f"{what}: {name} changed"


@pytest.mark.parametrize("kind", ["inf", "nan", "overflow"])
def test_adam_skip_leaves_p_m_v_alone_and_counts_once(kind):
    n = 2051
    if kind == "overflow":                                       # finite gradients of 1e20: their squares overflow
        _skip_case(n, torch.full((n,), 1e20), None, "adam skip overflow")
    else:
        _skip_case(n, torch.randn(n, generator=g(3)), float(kind), f"adam skip {kind}")


def test_adam_skip_on_a_nan_in_the_tail_at_the_cap():
    """The only NaN is the last element of the 3-float tail at n = 8T + 2051: block 0 of l2norm_sq's capped grid must read it."""
    n = E.SIZES_ADAM[-1]
    gr = torch.randn(n, generator=g(3))
    gr[-1] = float("nan")
    _skip_case(n, gr, None, "adam skip NaN tail")


def test_adam_ema_step_at_the_cap_gives_adam_steps_bits():
    n, omd = E.SIZES_ADAM[-1], 1e-3
    p0, m0, v0 = torch.randn(n, generator=g(0)), torch.randn(n, generator=g(1)) * 0.01, torch.rand(n, generator=g(2)) * 1e-4
    e0, gr = torch.randn(n, generator=g(4)), _unit(n, 5, 3.0)
    a, b, ema, gd = AdamState(n, p0, m0, v0), AdamState(n, p0, m0, v0), Out(n, init=e0), src(gr)
    nsq = a.norm_sq(gd)
    ops.adam_step(a.p.t, gd, a.m.t, a.v.t, nsq, 1.0, 1.0, step=7, **ADAM)
    ops.adam_ema_step(b.p.t, gd, b.m.t, b.v.t, ema.t, nsq, 1.0, 1.0, step=7, one_minus_decay=omd, **ADAM)
    for x, y, name in zip((a.p, a.m, a.v), (b.p, b.m, b.v), "pmv"):
        assert bits_equal(x.ok("adam_step " + name), y.ok("adam_ema_step " + name)), name
    pn = b.p.t.cpu()
    assert torch.equal(ema.cpu("adam_ema_step ema"), e0 + (pn - e0) * E.f32(omd))
    assert not torch.equal(pn, p0)


# ----------------------------------------------------------------------------------------------------- against float64: norms, losses
@pytest.mark.parametrize("n", E.SIZES_ADAM)
@pytest.mark.parametrize("kind", ["randn", "ill"])
def test_l2norm_sq_at_every_size(kind, n):
    x = E.l2norm_input(n, kind)
    xd, partial, out = src(x), Out(1024), Out(1)
    ops.l2norm_sq(xd, partial.t, out.t)
    partial.ok("l2norm_sq partial")
    E.report(f"l2norm_sq {kind} n={n}", E.l2norm_figures(float(out.ok("l2norm_sq out")), x))
    unchanged(xd, x, "l2norm_sq g")


@pytest.mark.parametrize("B,chw", E.LOSS_SHAPES)
@pytest.mark.parametrize("kind", E.LOSS_KINDS)
def test_loss_fwd_bwd_at_the_block_cap(kind, B, chw):
    for neg in (False, True):
        pred, y, ps = E.loss_inputs(B, chw, neg)
        pd, yd, psd = src(pred), src(y), None if ps is None else src(ps)
        for gscale in (1.0, 0.5):
            what = f"loss {kind} B={B} chw={chw} pscale={'neg' if neg else 'none'} gscale={gscale}"
            dpred, loss, partial, loss2 = Out(B, chw), Out(1), Out(1024), Out(1)
            ops.mse_fwd_bwd(pd, yd, dpred.t, loss.t, partial.t, pscale=psd, gscale=gscale, kind=kind)
            partial.ok(what + " partial")
            E.report(what, E.loss_figures(float(loss.ok(what + " loss")), dpred.ok(what + " dpred"), *E.loss_f64(pred, y, ps, gscale, kind)))
            ops.mse_fwd_bwd(pd, yd, None, loss2.t, partial.t, pscale=psd, gscale=gscale, kind=kind)          # dpred = None: the same loss bits
            assert bits_equal(loss2.ok(what + " loss (no dpred)"), loss.t) and partial.g.intact(), what + ": dpred = None changed the loss"
        unchanged(pd, pred, "loss pred"), unchanged(yd, y, "loss y")


@pytest.mark.parametrize("inner", E.BATCH_NORM_INNERS)
@pytest.mark.parametrize("B", E.BATCH_NORM_BS)
def test_batch_l2norm(B, inner):
    x = torch.randn(B, inner, generator=g(30))
    xd, out = src(x), Out(B)
    ops.batch_l2norm(xd, out.t)
    E.report(f"batch_l2norm B={B} inner={inner}", E.batch_l2norm_figures(out.ok("batch_l2norm"), x))
    unchanged(xd, x, "batch_l2norm x")


# ------------------------------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("B,half", E.TEMB_SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_timestep_embedding_both_orders(flip, B, half):
    t, freqs = E.temb_inputs(B, half)
    td, fd, emb = src(t), src(freqs), Out(B, 2 * half)
    ops.timestep_embedding(td, fd, emb.t, flip)
    E.report(f"timestep_embedding B={B} half={half} flip={flip}", E.temb_figures(emb.ok("timestep_embedding"), t, freqs, flip))


@pytest.mark.parametrize("B,half", E.FOURIER_SHAPES)
def test_fourier_embedding(B, half):
    t, W = E.fourier_inputs(B, half)
    td, Wd, emb = src(t), src(W), Out(B, 2 * half)
    ops.fourier_embedding(td, Wd, emb.t)
    E.report(f"fourier_embedding B={B} half={half}", E.fourier_figures(emb.ok("fourier_embedding"), t, W))


# ------------------------------------------------------------------------------------------------------------------------------ SiLU
@pytest.mark.parametrize("n", E.SIZES_SCALAR)
def test_silu_elementwise_on_the_grid_and_at_the_cap(n):
    z, dy, dx0 = E.silu_inputs(n, seed=20)
    zd, dyd = src(z), src(dy)
    y, dx, dxa = Out(n), Out(n), Out(n, init=dx0)                  # dx starts NaN-filled: accumulate = False must leave no NaN
    ops.silu_fwd(zd, y.t)
    ops.silu_bwd(dyd, zd, dx.t, accumulate=False)
    ops.silu_bwd(dyd, zd, dxa.t, accumulate=True)
    figs = E.silu_fwd_figures(y.ok("silu_fwd"), z) + E.silu_bwd_figures(dx.ok("silu_bwd"), z, dy) + E.silu_bwd_figures(dxa.ok("silu_bwd acc"), z, dy, dx0)
    assert not bool(torch.isnan(dx.t).any()) and not bool(torch.isnan(y.t).any())
    E.report(f"silu n={n}", figs)
    unchanged(zd, z, "silu x"), unchanged(dyd, dy, "silu dy")
