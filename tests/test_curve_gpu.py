"""Mode Connectivity Repair on the GPU: the two kernels of vd_curve.hip bit for bit against their numpy float32 op sequences (every size, aligned
bases and single buffers one float past alignment, sentinels around every output), the three sums exactly on integers and within their derived
bound on real data, and the training step (`curve.CurveAdam`, `curve.curve_step`): four optimiser steps against the oracle of
tests/curve_ref.py beside the plain step's, the gradient norm (the direct check on cm), the point the network holds, the launches, resume,
the cuts at the ends, the loss scan, the other two families, and the tools in child processes."""
import copy
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
import curve_ref  # noqa: E402
import oracle.schedulers_ref as R  # noqa: E402
from oracle.loss_ref import SDE_LDM, SDE_VE, LossFnRef  # noqa: E402
from oracle.schedulers_ref import ScoreSdeVeSchedulerRef  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import anchor, curve, lib, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.curve import Curve, CurveConfig  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.schedulers import get_cosine_schedule_with_warmup_lambda  # noqa: E402
from villandiffusion_amd.trainer import FusedAdam  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = curve_ref.SMALL
SENTINEL = 123.5
GRID_CAP, BLOCK, FPT = ops.curve_plan(1 << 40)
# scalar tail only (< 4), one item + tail, a workgroup boundary with tails, grid-stride with a tail; one n on each side of the grid cap, asked of
# vd_curve_plan: the largest n every thread of the capped grid serves with its own four items, and the first n at which a thread strides on
SIZES = [1, 2, 3, 4, 5, 7, 2048, 2049, 2051, 100003, GRID_CAP * BLOCK * FPT - 1, GRID_CAP * BLOCK * FPT + 1]
# which buffers lie one float past 16-byte alignment: (out, wa, wm, wb)
ALIGN = {"aligned": (0, 0, 0, 0), "out+4B": (1, 0, 0, 0), "wm+4B": (0, 0, 1, 0)}
f32 = np.float32


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """Every test of this file gives back what it took before the next one starts: the size sweeps and the flat copies of the networks leave
    some hundred MB in the caching allocator.  Whatever runs next starts from a quiet device."""
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


def ints(n, gen, lo, hi):
    return torch.randint(lo, hi + 1, (n,), generator=gen).float()


def normals(n, gen):
    x = torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-3, 1, (1,), generator=gen))
    x[x == 0] = 1.0                                                            # finite data without (negative) zeros
    return x


# ------------------------------------------------------------------------------------------------------------------- 1. the kernels
def test_the_plan_caps_the_grid_at_the_partial_buffer():
    assert (BLOCK, FPT) == (256, 16) and GRID_CAP <= 1024
    assert ops.curve_plan(SIZES[-2])[0] == GRID_CAP == ops.curve_plan(SIZES[-1])[0] and ops.curve_plan(SIZES[-2] - BLOCK * FPT)[0] == GRID_CAP - 1


@pytest.mark.parametrize("align", list(ALIGN))
@pytest.mark.parametrize("n", SIZES)
def test_curve_point_is_the_numpy_sequence_bit_for_bit(n, align):
    """Integers with coefficients that are powers of two (every operation exact, the order pinned all the same), then normal data with the
    float32 coefficients of t = 0.3; the midpoint call with wm aliased to wa; (1, 0, 0) and (0, 0, 1) give back the ends' bits; a repeat
    gives the same bits; the sentinels around out stay and the inputs keep their bits."""
    so, sa, sm, sb = ALIGN[align]
    gen = g(1000 + n)
    for kind in ("int", "normal"):
        if kind == "int":
            wa, wm, wb = (ints(n, gen, -8, 8) for _ in range(3))
            co = (0.25, 0.5, 0.25)
        else:
            wa, wm, wb = (normals(n, gen) for _ in range(3))
            co = curve.coefficients("bezier", 0.3)
        (ba, va), (bm, vm), (bb, vb) = shifted(wa, sa), shifted(wm, sm), shifted(wb, sb)
        bo, vo = shifted(torch.zeros(n), so)
        na, nm, nb = wa.numpy(), wm.numpy(), wb.numpy()

        def run(co_, mid=None):
            vo.fill_(SENTINEL)
            ops.curve_point(vo, va, vm if mid is None else mid, vb, *co_, weights=False)
            torch.cuda.synchronize()
            assert untouched(bo, so, n), (n, align, kind, co_)
            return bits(vo)

        want = torch.from_numpy(curve_ref.point_ref(na, nm, nb, *co))
        got = run(co)
        assert torch.equal(got, bits(want)), (n, align, kind)
        assert torch.equal(run(co), got)                                      # two runs, the same bits
        if kind == "int":
            assert torch.equal(want, 0.25 * wa + 0.5 * wm + 0.25 * wb)
        assert torch.equal(run((0.5, 0.0, 0.5), mid=va), bits(torch.from_numpy(curve_ref.point_ref(na, na, nb, 0.5, 0.0, 0.5))))      # wm is wa
        if kind == "normal":
            assert torch.equal(run((1.0, 0.0, 0.0)), bits(wa)) and torch.equal(run((0.0, 0.0, 1.0)), bits(wb))
        for (buf, v), host, sh in (((ba, va), wa, sa), ((bm, vm), wm, sm), ((bb, vb), wb, sb)):
            assert torch.equal(bits(v), bits(host)) and untouched(buf, sh, n)  # the inputs are read only


def test_curve_point_through_the_wrapper_counts_as_a_write_of_weights_only_when_told():
    a = torch.ones(8, device=DEV)
    out = torch.empty(8, device=DEV)
    e = ops.WEIGHTS_EPOCH
    ops.curve_point(out, a, a, a, 0.25, 0.5, 0.25, weights=False)
    assert ops.WEIGHTS_EPOCH == e
    ops.curve_point(out, a, a, a, 0.25, 0.5, 0.25)
    assert ops.WEIGHTS_EPOCH == e + 1 and bool((out == 1).all())


def test_refusals_through_ctypes_on_device_buffers():
    h = lib.load()
    n = 64
    out, wa, wm, wb = (torch.zeros(n, device=DEV) for _ in range(4))
    partial, out3 = torch.zeros(3 * 1024, device=DEV), torch.ones(3, device=DEV)
    Pp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    ok = dict(out=Pp(out), wa=Pp(wa), wm=Pp(wm), wb=Pp(wb), n=n, ca=0.25, cm=0.5, cb=0.25)
    call = lambda a: h.vd_curve_point(a["out"], a["wa"], a["wm"], a["wb"], a["n"], a["ca"], a["cm"], a["cb"], st)
    for bad in (dict(n=-1), dict(out=None), dict(wa=None), dict(wm=None), dict(wb=None), dict(out=Pp(wa)), dict(out=Pp(wm)), dict(out=Pp(wb)),
                dict(out=C.c_void_p(wb.data_ptr() + 16)), dict(wa=C.c_void_p(out.data_ptr() + 4 * (n - 1))),
                dict(ca=nan), dict(cm=inf), dict(cb=-inf), dict(cb=nan)):
        assert call(dict(ok, **bad)) == -22, bad
    assert call(dict(ok, wm=Pp(wa))) == 0 and call(dict(ok, wa=Pp(wb), wm=Pp(wb))) == 0      # the inputs may be one another
    out.fill_(7.0)
    assert call(dict(ok, n=0)) == 0                                          # n = 0: no launch, nothing written
    okg = dict(wa=Pp(wa), wm=Pp(wm), wb=Pp(wb), n=n, partial=Pp(partial), out3=Pp(out3))
    callg = lambda a: h.vd_curve_geometry(a["wa"], a["wm"], a["wb"], a["n"], a["partial"], a["out3"], st)
    for bad in (dict(n=-1), dict(wa=None), dict(wm=None), dict(wb=None), dict(partial=None), dict(out3=None), dict(partial=Pp(wa)),
                dict(out3=Pp(wm)), dict(out3=C.c_void_p(wb.data_ptr() + 4 * (n - 3))), dict(out3=Pp(partial)),
                dict(wb=C.c_void_p(partial.data_ptr() + 4 * 3071))):
        assert callg(dict(okg, **bad)) == -22, bad
    assert callg(dict(okg, wm=Pp(wa))) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(out3.abs().sum()) == 0.0


def geometry_int_data(n, seed):
    """wa, wm, wb in {-1, 0, 1} (differences in -2 .. 2, squares <= 4), one float in four non-zero past 2^18 floats: every operation is exact
    and every sum stays below 2^24."""
    gen = g(seed)
    out = [ints(n, gen, -1, 1) for _ in range(3)]
    if n > (1 << 18):
        out = [v * (torch.randint(0, 4, (n,), generator=gen) == 0) for v in out]
    return out


def geometry_scratch():
    pb = torch.full((3 * 1024 + 4,), SENTINEL, device=DEV)
    ob = torch.full((8,), SENTINEL, device=DEV)
    return pb, pb[:3 * 1024], ob, ob[:3]


@pytest.mark.parametrize("shift", [(0, 0, 0), (0, 1, 0), (1, 1, 1)], ids=["aligned", "wm+4B", "all+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_curve_geometry_on_integers_is_exact(n, shift):
    wa, wm, wb = geometry_int_data(n, 700 + n)
    bufs = [shifted(v, s) for v, s in zip((wa, wm, wb), shift)]
    pb, partial, ob, out3 = geometry_scratch()
    ops.curve_geometry(bufs[0][1], bufs[1][1], bufs[2][1], partial, out3)
    torch.cuda.synchronize()
    want = curve_ref.geometry_f64(wa.numpy(), wm.numpy(), wb.numpy())
    assert want.max() < 2 ** 24 and [float(v) for v in out3.cpu()] == [float(v) for v in want], (n, shift, out3.cpu(), want)
    assert bool((pb[3 * 1024:] == SENTINEL).all()) and bool((ob[3:] == SENTINEL).all())
    for (buf, v), host, s in zip(bufs, (wa, wm, wb), shift):
        assert torch.equal(bits(v), bits(host)) and untouched(buf, s, n)
    assert n < 100 or want.min() > 0


_WORST = {"ratio": 0.0}


@pytest.mark.parametrize("n", [5, 2051, 100003, SIZES[-2], SIZES[-1]])
def test_curve_geometry_on_real_data_the_bound_of_the_longest_chain_and_the_numpy_order(n):
    """Each sum against float64 (float64 differences and squares of the same float32 inputs): |error| <= (chain + 2) * 2^-24 * sum of the terms,
    chain = the longest chain of additions include/villan_hip.h states for the launch shape vd_curve_plan reports, + 2 for the roundings of the
    difference and of the square.  The three floats are also the numpy restatement of the two stages bit for bit; a base one float past
    alignment and a repeat give the same bits.  Largest error / bound measured on MI355X: 0.067 (n = 2051)."""
    gen = g(n)
    wa, wb = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1
    wm = 0.5 * (wa + wb) + torch.randn(n, generator=gen) * 5e-3
    grid, block, _ = ops.curve_plan(n)
    chain = curve_ref.chain(n, grid, block)
    assert chain == -(-((n + 3) // 4) // (grid * 256)) + -(-grid // 256) + 18
    got = []
    for shift in ((0, 0, 0), (1, 0, 1), (0, 0, 0)):
        bufs = [shifted(v, s) for v, s in zip((wa, wm, wb), shift)]
        pb, partial, ob, out3 = geometry_scratch()
        ops.curve_geometry(bufs[0][1], bufs[1][1], bufs[2][1], partial, out3)
        torch.cuda.synchronize()
        got.append(out3.cpu().clone())
        assert all(torch.equal(bits(v), bits(h)) and untouched(b, s, n) for (b, v), h, s in zip(bufs, (wa, wm, wb), shift))
    assert torch.equal(bits(got[0]), bits(got[1])) and torch.equal(bits(got[0]), bits(got[2]))
    want = curve_ref.geometry_f64(wa.numpy(), wm.numpy(), wb.numpy())
    for s in range(3):
        err, bound = abs(float(got[0][s].double()) - want[s]), (chain + 2) * 2.0 ** -24 * want[s]
        _WORST["ratio"] = max(_WORST["ratio"], err / bound)
        print(f"[curve] geometry sum {s} n={n}: chain {chain}, error {err:.3e}, bound {bound:.3e}, error / bound {err / bound:.3e} "
              f"(largest so far {_WORST['ratio']:.3e})")
        assert err <= bound, (n, s, err, bound)
    ref = curve_ref.geometry_ref(wa.numpy(), wm.numpy(), wb.numpy(), grid, block)
    assert torch.equal(bits(got[0]), bits(torch.from_numpy(ref))), (n, got[0], ref)


def test_curve_geometry_of_nothing_is_three_positive_zeros():
    pb, partial, ob, out3 = geometry_scratch()
    one = torch.ones(4, device=DEV)                 # (an empty tensor's data_ptr() is NULL, which is refused: the C call with real pointers)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.load().vd_curve_geometry(p(one), p(one), p(one), 0, p(partial), p(out3), st) == 0
    torch.cuda.synchronize()
    assert bits(out3).tolist() == [0, 0, 0] and bool((ob[3:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- 2. the training step
def dev_batch(i):
    x0, Rr, t, eps = curve_ref.batch_of(i)
    return x0.cuda(), Rr.cuda(), t.cuda(), eps.cuda()


LR = get_cosine_schedule_with_warmup_lambda(0, 20)          # the schedule of the oracle (and of the trainer): base 1e-3, no warm-up, 20 steps


def make_curve(conv_math=None, seed=curve_ref.SEED_A, swap=False, kind="bezier"):
    """The small UNet (at `seed`: the curve overwrites it) with the curve of tests/curve_ref.py between its two endpoints -> (net, lf, opt)."""
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=seed)
    if conv_math is not None:
        net.conv_math = conv_math
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    s = curve_ref.setup()
    ends = (s["B"], s["A"]) if swap else (s["A"], s["B"])
    cv = Curve(net, ends[0], ends[1], CurveConfig(kind=kind, seed=curve_ref.CURVE_SEED))
    return net, lf, curve.CurveAdam(cv, 1e-3)


def run_steps(net, lf, opt, first, last):
    out = []
    for i in range(first, last):
        x0, Rr, t, eps = dev_batch(i)
        out.append(curve.curve_step(net, opt, lf, x0, Rr, t, noise=eps, lr=1e-3 * LR(opt.step_count)))
    torch.cuda.synchronize()
    return out


def plain_steps(net, lf, batches, lr=1e-3):
    """The plain optimiser step the curve step is measured beside: the same eager loop with trainer.FusedAdam on the weights themselves."""
    opt = FusedAdam(net, lr)
    lf.grad_scale = 1.0
    out = []
    for k, (x0, Rr, t, eps) in enumerate(batches):
        net.zero_grad()
        loss = lf.p_loss(net, x0.cuda(), Rr.cuda(), t.cuda(), noise=eps.cuda())
        loss.backward()
        opt.step(lr=lr * LR(k))
        net.zero_grad()
        torch.cuda.synchronize()
        out.append((float(loss.detach()), opt.grad_norm()))
    return out


_PLAIN = {}


def plain_error(conv_math, steps=curve_ref.STEPS):
    """The plain step's update L2 error from endpoint A against the plain oracle over the same batches, measured once per arithmetic."""
    key = (conv_math, steps)
    if key not in _PLAIN:
        o = curve_ref.oracle_run("plain", steps=steps)
        net = UNet2DModel(**SMALL)
        net.reset_parameters(seed=curve_ref.SEED_A)
        if conv_math is not None:
            net.conv_math = conv_math
        got = plain_steps(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), [curve_ref.batch_of(i) for i in range(steps)])
        for (l, _), l_ref in zip(got, o["losses"]):
            assert abs(l - l_ref) <= 1e-4 * abs(l_ref)
        _PLAIN[key] = curve_ref.update_error(net.flat_param, o["end"], o["start"])
    return _PLAIN[key]


@pytest.mark.parametrize("conv_math", ["bf16x3", "f32"])
def test_four_steps_follow_the_oracle_in_theta_in_the_gradient_norm_and_in_the_point_held(conv_math):
    """The update L2 error ||theta - theta_ref|| / ||theta_ref - theta_0|| against the oracle (functional_call at (ca A + cm theta) + cb B,
    autograd to theta, clip_grad_norm_, Adam), beside the plain step's against the plain oracle over the same batches; the gate is 1.5x the
    plain figure of the same run (the rule of the anchored and the masked fine-tune: the gradient passes are the same kernels).
    After every step opt.grad_norm() is within 1e-4 of the oracle's pre-clip norm of theta's gradient -- the direct check on cm -- and
    flat_param is Curve.point(t) recomputed, bit for bit.  Measured on MI355X: bf16x3 1.91e-4 beside the plain step's 4.10e-4, f32
    2.30e-5 beside 4.50e-5; gradient-norm errors at most 8.0e-6 and 2.6e-6; the oracle without cm 0.365 away."""
    s, o = curve_ref.setup(), curve_ref.oracle_run("curve")
    net, lf, opt = make_curve(conv_math=conv_math)
    cv = opt.curve
    assert opt.t == o["ts"][0] and torch.equal(bits(cv.theta), bits(s["theta0"])) and torch.equal(bits(cv.wa), bits(s["A"]))
    base = plain_error(conv_math)
    gate = 1.5 * base
    scratch = torch.empty_like(net.flat_param)
    norm_errs = []
    for i in range(curve_ref.STEPS):
        (loss,) = run_steps(net, lf, opt, i, i + 1)
        loss = float(loss)
        assert abs(loss - o["losses"][i]) <= 1e-4 * abs(o["losses"][i]), (i, loss, o["losses"][i])
        norm_errs.append(abs(opt.grad_norm() - o["norms"][i]) / o["norms"][i])
        assert opt.t == o["ts"][i + 1]
        cv.point(opt.t, out=scratch)
        assert torch.equal(bits(net.flat_param), bits(scratch)), i
        want = curve_ref.point_ref(s["A"].numpy(), cv.theta.cpu().numpy(), s["B"].numpy(), *curve.coefficients("bezier", opt.t))
        assert torch.equal(bits(scratch), bits(torch.from_numpy(want))), i
    assert opt.step_count == curve_ref.STEPS and int(opt.skipped) == 0 and float(net.flat_grad.abs().sum()) == 0.0 and lf.grad_scale == 1.0
    upd = curve_ref.update_error(cv.theta, o["end"], s["theta0"])
    teeth = curve_ref.update_error(curve_ref.oracle_run("forget_cm")["end"], o["end"], s["theta0"])
    print(f"[parity] {curve_ref.STEPS} curve optimiser steps ({conv_math}): update L2 error {upd:.3e}; plain step {base:.3e}; gate {gate:.3e}; "
          f"gradient-norm relative errors {['%.2e' % e for e in norm_errs]}; an oracle without cm lies {teeth:.3f} away")
    if conv_math == "bf16x3":
        assert teeth >= 10 * gate, (teeth, gate)                             # a forgotten cm would be this far out
    assert max(norm_errs) <= 1e-4, norm_errs
    assert upd <= gate, (upd, base)


def test_the_curve_step_is_the_plain_step_and_one_launch_more():
    """Launch for launch: the curve step is the plain eager step (forward, backward, norm, Adam) plus exactly one vd_curve_point launch, after
    the Adam kernel."""
    net, lf, opt = make_curve()
    pnet = UNet2DModel(**SMALL)
    pnet.reset_parameters(seed=curve_ref.SEED_A)
    plf, popt = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), FusedAdam(pnet, 1e-3)
    x0, Rr, t, eps = dev_batch(0)

    def plain():
        pnet.zero_grad()
        plf.p_loss(pnet, x0, Rr, t, noise=eps).backward()
        popt.step()
        pnet.zero_grad()

    names = {}
    for key, fn in (("plain", plain), ("curve", lambda: curve.curve_step(net, opt, lf, x0, Rr, t, noise=eps))):
        fn()
        ops.profile_start()
        fn()
        names[key] = [r["name"] for r in ops.profile_stop()]
    assert not any("curve" in n for n in names["plain"])
    assert [n for n in names["curve"] if "curve" in n] == ["curve_point (curve_point_kernel)"]
    extra = list(names["curve"])
    extra.remove("curve_point (curve_point_kernel)")
    assert extra == names["plain"]                                            # one launch more, nothing else
    k = names["curve"].index("curve_point (curve_point_kernel)")
    assert names["curve"][k - 1].startswith("adam_step") and names["curve"][k - 2].startswith("l2norm_sq")     # norm, Adam on the bend, the next point


def clone_state(sd):
    return {k: clone_state(v) if isinstance(v, dict) else (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in sd.items()}


def test_resume_continues_bit_for_bit_and_other_endpoints_or_another_kind_are_refused():
    net, lf, opt = make_curve()
    run_steps(net, lf, opt, 0, 2)
    st = clone_state({"optimizer": opt.state_dict(), "curve": opt.curve_state()})
    assert set(st["curve"]) >= {"theta", "t", "generator", "kind", "fingerprints"} and st["curve"]["t"] == opt.t
    assert st["curve"]["theta"].numel() == net.flat_numel and st["curve"]["fingerprints"] == list(opt.curve.fingerprints())
    assert sum(v.numel() for v in st["optimizer"].values() if torch.is_tensor(v)) == 2 * net.flat_numel       # the endpoints are not stored
    run_steps(net, lf, opt, 2, 4)
    net2, lf2, again = make_curve(seed=99)                                    # other weights: phi(t) overwrites them
    again.load_curve_state(st["curve"])
    again.load_state_dict(st["optimizer"])
    assert again.t == st["curve"]["t"] and again.step_count == 2
    run_steps(net2, lf2, again, 2, 4)
    for a, b in ((again.curve.theta, opt.curve.theta), (again.exp_avg, opt.exp_avg), (again.exp_avg_sq, opt.exp_avg_sq),
                 (net2.flat_param, net.flat_param)):
        assert torch.equal(bits(a), bits(b))
    assert again.t == opt.t and again.step_count == 4
    _, _, swapped = make_curve(swap=True)
    before = bits(swapped.curve.theta)
    with pytest.raises(ValueError, match="written between other endpoints"):
        swapped.load_curve_state(clone_state(st)["curve"])
    assert torch.equal(bits(swapped.curve.theta), before)                      # refused before anything was loaded
    with pytest.raises(ValueError, match="holds a 'bezier' curve; this optimiser trains a 'polychain' one"):
        make_curve(kind="polychain")[2].load_curve_state(clone_state(st)["curve"])


def test_the_cuts_at_the_ends_are_the_endpoints_and_curve_pt_round_trips(tmp_path):
    s = curve_ref.setup()
    net, lf, opt = make_curve(kind="polychain")
    cv = opt.curve
    run_steps(net, lf, opt, 0, 1)
    opt.hold(0.0)
    assert opt.t == 0.0 and torch.equal(bits(net.flat_param), bits(s["A"]))
    opt.hold(1)
    assert opt.t == 1.0 and torch.equal(bits(net.flat_param), bits(s["B"]))
    opt.hold(0.5)
    assert torch.equal(bits(net.flat_param), bits(cv.theta))                   # the polychain's corner is the bend itself
    geo = cv.geometry()
    assert geo["length"] == geo["leg_a"] + geo["leg_b"] and geo["bend_offset"] > 0
    chord = float((s["A"].double() - s["B"].double()).norm())
    assert abs(geo["chord"] - chord) <= 1e-5 * chord
    # curve.pt
    path = cv.save(str(tmp_path))
    assert path.endswith("curve.pt")
    d = torch.load(path, map_location="cpu")
    assert set(d) == {"theta", "kind", "numel", "layout_sha256", "family", "fingerprints"} and d["kind"] == "polychain"
    assert d["family"] == "UNet2DModel" and d["layout_sha256"] == anchor.layout_digest(net) and d["numel"] == net.flat_numel
    back = curve.load_curve(str(tmp_path), net, s["A"], s["B"])
    assert torch.equal(bits(back.theta), bits(cv.theta)) and back.kind == "polychain"
    with pytest.raises(ValueError, match="written between other endpoints: its end_a"):
        curve.load_curve(path, net, s["B"], s["A"])
    with pytest.raises(ValueError, match="holds a 'polychain' curve; the configuration asks for 'bezier'"):
        curve.load_curve(path, net, s["A"], s["B"], CurveConfig())
    other = UNet2DModel(**dict(SMALL, layers_per_block=2))
    with pytest.raises(ValueError, match=rf"of {net.flat_numel} floats; this UNet2DModel has {other.flat_numel}"):
        curve.load_curve(path, other, torch.zeros(other.flat_numel), torch.zeros(other.flat_numel))
    with pytest.raises(ValueError, match=rf"{net.flat_numel} floats .*got \(8,\)"):
        Curve(net, torch.zeros(8), s["B"])
    # a fresh curve starts on the chord's midpoint: no bend, the bezier's length is the chord.  bend_offset^2 = sa / 2 + sb / 2 - sc / 4 is
    # a difference of three float32 sums, each within (chain + 2) * 2^-24 < 2e-6 of its value, so what is left of it is below
    # 3/4 * 2e-6 * chord^2: bend_offset <= 1.3e-3 chord, and the length exceeds the chord by O(bend_offset^2 / chord)
    fresh = Curve(net, s["A"], s["B"]).geometry()
    assert fresh["bend_offset"] <= 1.3e-3 * fresh["chord"] and abs(fresh["length"] - fresh["chord"]) <= 1e-5 * fresh["chord"]
    assert abs(fresh["leg_a"] - 0.5 * fresh["chord"]) <= 1e-5 * fresh["chord"]


def test_curve_scan_at_the_ends_is_the_endpoints_loss_and_the_network_keeps_its_weights():
    s = curve_ref.setup()
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=17)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    cv = Curve(net, s["A"], s["B"])
    before = bits(net.flat_param)
    batches = [curve_ref.batch_of(k)[0] for k in range(2)]
    rows = curve.curve_scan(net, cv, lf, batches, [0.0, 0.5, 1.0], seed=5)
    assert torch.equal(bits(net.flat_param), before)
    assert [r["t"] for r in rows] == [0.0, 0.5, 1.0] and all(set(r) == {"t", "loss_clean"} and math.isfinite(r["loss_clean"]) for r in rows)

    def plainly(flat):
        twin = UNet2DModel(**SMALL)
        with torch.no_grad():
            twin.flat_param.copy_(flat)
        twin.weights_changed()
        out = []
        with torch.no_grad():
            for k, x0 in enumerate(batches):
                t, eps = anchor.fisher_draws(x0.shape, 1000, 5, k)
                out.append(lf.p_loss(twin, x0.cuda(), torch.zeros_like(x0).cuda(), t.cuda(), noise=eps.cuda()).reshape(()))
        return float(torch.stack(out).double().mean())

    assert rows[0]["loss_clean"] == plainly(s["A"]) and rows[2]["loss_clean"] == plainly(s["B"])
    assert rows[1]["loss_clean"] not in (rows[0]["loss_clean"], rows[2]["loss_clean"])
    # with a trigger: the poisoned loss beside it, the clean one unchanged
    trig = torch.rand(3, 32, 32, generator=g(8)) * 0.5
    target = torch.rand(3, 32, 32, generator=g(9)) * 2 - 1
    with pytest.raises(ValueError, match="with a trigger every batch is a dict"):
        curve.curve_scan(net, cv, lf, batches, [0.0], seed=5, trigger=trig)
    with pytest.raises(ValueError, match=r"t must lie in \[0, 1\]"):
        curve.curve_scan(net, cv, lf, batches, [0.0, 1.5], seed=5)
    rows_p = curve.curve_scan(net, cv, lf, [{"image": b, "target": target} for b in batches], [0.0, 1.0], seed=5, trigger=trig)
    assert [r["loss_clean"] for r in rows_p] == [rows[0]["loss_clean"], rows[2]["loss_clean"]]
    assert all(math.isfinite(r["loss_poison"]) and r["loss_poison"] != r["loss_clean"] for r in rows_p)
    assert torch.equal(bits(net.flat_param), before)


# ------------------------------------------------------------------------------------------------------------------- 3. the other families
@pytest.mark.parametrize("family", ["ve", "ldm"])
def test_the_other_families_follow_their_oracle_for_two_steps(family):
    """A small NCSN++ (SDE-VE) and the small latent UNet (SDE-LDM): two optimiser steps against the family's oracle under the same gate, 1.5x
    the family's plain trainer over the same batches; the gradient norm within 1e-3, these families' own gradient gate.  NCSN++'s fixed
    Fourier features are the same in both endpoints (as in two checkpoints of one model) and take no gradient.

    The plain trainer starts from phi(t0), the very weights the curve trainer takes its first gradient at: the same kernels on the same data.
    Between two independent initialisations that point is another network than either end (its weights have about half their variance), and
    the update error of two Adam steps depends on where it is taken: with the plain trainer started from endpoint A instead, the first
    version of this test, the figures on MI355X were ve 1.643e-3 beside 1.060e-3 (1.55x) and ldm 1.432e-3 beside 8.930e-4 (1.60x), with the
    gradient norms within 2.1e-5 and flat_param bit-equal to the recomputed point -- the convolutions' error at another point, not the curve's.
    That figure is still printed."""
    gen = g(7)
    if family == "ve":
        cfg = dict(fam.SMALL_PP, layers_per_block=1)
        make = lambda **k: NCSNppModel(**cfg, **k)
        ref, lref = fam._pp.NCSNppRef(**cfg), LossFnRef(ScoreSdeVeSchedulerRef(**fam.VE_SCHED), SDE_VE, psi=0)
        lf_of = lambda: LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0)
        draw = lambda: (torch.rand(4, 3, 16, 16, generator=gen), torch.tensor(fam.VE_T))
        frozen = ("time_proj.weight",)
    else:
        make = lambda **k: UNet2DModel(**fam.SMALL_LDM, **k)
        ref, lref = UNet2DModelRef(**fam.SMALL_LDM), LossFnRef(R.DDPMSchedulerRef(), SDE_LDM, psi=1)
        lf_of = lambda: LossFn(S.DDPMScheduler(), "SDE-LDM", psi=1)
        draw = lambda: (torch.randn(4, 3, 8, 8, generator=gen), torch.tensor(fam.LDM_T))
        frozen = ()
    batches = []
    for _ in range(2):
        x0, t = draw()
        Rr = torch.rand(x0.shape, generator=gen) * 0.5
        Rr[::2] = 0
        batches.append((x0, Rr, t, torch.randn(x0.shape, generator=gen)))
    a, b = make(device="cpu"), make(device="cpu")
    a.reset_parameters(seed=5)
    b.reset_parameters(seed=6)
    A, B = a.flat_param.detach().clone(), b.flat_param.detach().clone()
    for name in frozen:
        off, n, _ = a._offs[name]
        B[off:off + n] = A[off:off + n]
    offs = dict(a._offs)
    theta0 = torch.from_numpy(curve_ref.point_ref(A.numpy(), A.numpy(), B.numpy(), 0.5, 0.0, 0.5))
    ccfg = CurveConfig(seed=1, t_min=0.2, t_max=0.8)
    o = curve_ref.FlatOracle(ref, lref, offs, theta0, ends=(A, B), cfg=ccfg, frozen=frozen)
    start = torch.from_numpy(curve_ref.point_ref(A.numpy(), theta0.numpy(), B.numpy(), *curve.coefficients(ccfg.kind, o.ts[0])))      # phi(t0)
    plain_oracles = {"phi(t0)": curve_ref.FlatOracle(ref, lref, offs, start, frozen=frozen), "A": curve_ref.FlatOracle(ref, lref, offs, A, frozen=frozen)}
    want = [o.step([mb]) for mb in batches]
    for po in plain_oracles.values():
        for mb in batches:
            po.step([mb])

    bases = {}
    for key, w0 in (("phi(t0)", start), ("A", A)):
        net = make()
        with torch.no_grad():
            net.flat_param.copy_(w0)
        net.weights_changed()
        plain_steps(net, lf_of(), batches)
        bases[key] = curve_ref.update_error(net.flat_param, plain_oracles[key].theta, w0)
    base = bases["phi(t0)"]
    net2, lf2 = make(), lf_of()
    opt = curve.CurveAdam(Curve(net2, A, B, ccfg), 1e-3)
    assert torch.equal(bits(opt.curve.theta), bits(theta0)) and opt.t == o.ts[0] and torch.equal(bits(net2.flat_param), bits(start))
    got = []
    for k, (x0, Rr, t, eps) in enumerate(batches):
        loss = curve.curve_step(net2, opt, lf2, x0, Rr, t, noise=eps, lr=1e-3 * LR(k))
        torch.cuda.synchronize()
        got.append((float(loss), opt.grad_norm()))
    upd = curve_ref.update_error(opt.curve.theta, o.theta, theta0)
    norm_errs = [abs(gn - wn) / wn for (_, gn), (_, wn) in zip(got, want)]
    print(f"[parity] 2 curve optimiser steps ({family}): update L2 error {upd:.3e}; plain step from phi(t0) {base:.3e}; gate {1.5 * base:.3e}; "
          f"(plain step from A {bases['A']:.3e}); gradient-norm relative errors {['%.2e' % e for e in norm_errs]}; t {o.ts}")
    for (l, _), (wl, _) in zip(got, want):
        assert abs(l - wl) <= 1e-4 * abs(wl), (family, l, wl)
    assert opt.t == o.ts[2] and int(opt.skipped) == 0 and opt.step_count == 2
    scratch = torch.empty_like(net2.flat_param)
    opt.curve.point(opt.t, out=scratch)
    assert torch.equal(bits(net2.flat_param), bits(scratch))
    for name in frozen:                                                       # the Fourier features: the same in A and B, untrained in theta
        off, n, _ = offs[name]
        assert torch.equal(bits(opt.curve.theta[off:off + n]), bits(theta0[off:off + n]))
    assert max(norm_errs) <= 1e-3, norm_errs      # (the per-parameter gradient gate of these families' own tests, which bounds the norm a fortiori)
    assert upd <= 1.5 * base, (upd, base)


# ------------------------------------------------------------------------------------------------------------------- 4. the tools
def test_the_tools_in_child_processes(tmp_path):
    root = tmp_path / "ckpts"
    nets = {}
    for name, seed in (("SMALL-A", 1), ("SMALL-B", 2)):
        net = UNet2DModel(**SMALL)
        net.reset_parameters(seed=seed)
        P.DDPMPipeline(net, S.DDPMScheduler()).save_pretrained(str(root / name))
        nets[name] = net
    env = dict(os.environ, PYTHONPATH=ROOT)

    def tool(name, *argv):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + list(argv), cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    trig = str(tmp_path / "trigger.pt")
    torch.save(torch.rand(3, 32, 32, generator=g(8)) * 0.5, trig)
    ends = ["--ckpt-a", str(root / "SMALL-A"), "--ckpt-b", str(root / "SMALL-B")]
    fixed, fixed2 = str(tmp_path / "FIXED"), str(tmp_path / "FIXED2")
    line = json.loads(tool("mcr_repair.py", *ends, "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "8", "--steps", "2", "--batch", "4", "--t", "0.3",
                           "--scan", "3", "--trigger", trig, "--target", "CORNER", "--seed", "1", "--lr", "1e-3", "--out", fixed).strip().splitlines()[-1])
    info = json.load(open(os.path.join(fixed, "mcr.json")))
    assert {"family", "kind", "steps", "t", "geometry_before", "geometry_after", "last_losses", "scan"} <= set(info)
    assert (info["family"], info["kind"], info["steps"], info["t"]) == ("vp", "bezier", 2, 0.3) and line["scan"] == info["scan"]
    assert len(info["last_losses"]) == 2 and all(math.isfinite(v) for v in info["last_losses"])
    assert [r["t"] for r in info["scan"]] == [0.0, 0.5, 1.0] and all(math.isfinite(r["loss_clean"]) and math.isfinite(r["loss_poison"]) for r in info["scan"])
    for key in ("geometry_before", "geometry_after"):
        assert set(info[key]) == {"leg_a", "leg_b", "chord", "bend_offset", "length"}
    assert info["geometry_before"]["bend_offset"] <= 1.3e-3 * info["geometry_before"]["chord"]      # (rounding of the three sums: see above)
    assert info["geometry_after"]["bend_offset"] > info["geometry_before"]["bend_offset"]            # two steps of lr 1e-3 bend it
    assert info["geometry_before"]["chord"] == info["geometry_after"]["chord"]
    a, b = nets["SMALL-A"], nets["SMALL-B"]
    cv = curve.load_curve(fixed, a, a.flat_param.detach().clone(), b.flat_param.detach().clone())
    scratch = torch.empty_like(a.flat_param)
    cv.point(0.3, out=scratch)
    assert torch.equal(bits(P.DiffusionPipeline.from_pretrained(fixed).unet.flat_param), bits(scratch))
    # re-cutting another point from curve.pt, without training
    tool("mcr_repair.py", *ends, "--curve", os.path.join(fixed, "curve.pt"), "--t", "0.4", "--out", fixed2)
    info2 = json.load(open(os.path.join(fixed2, "mcr.json")))
    assert (info2["steps"], info2["t"], info2["scan"], info2["kind"]) == (0, 0.4, None, "bezier") and info2["geometry_after"] == info["geometry_after"]
    cv.point(0.4, out=scratch)
    assert torch.equal(bits(P.DiffusionPipeline.from_pretrained(fixed2).unet.flat_param), bits(scratch))
    assert torch.equal(bits(torch.load(os.path.join(fixed2, "curve.pt"), map_location="cpu")["theta"]), bits(cv.theta))
    # swapped checkpoints are refused by the fingerprints
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mcr_repair.py"), "--ckpt-a", ends[3], "--ckpt-b", ends[1], "--curve",
                          os.path.join(fixed, "curve.pt"), "--t", "0.4", "--out", str(tmp_path / "FIXED3")], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode != 0 and "written between other endpoints" in out.stderr
    assert "curve_point" in tool("curve_step_ab.py", "--help") and "--rounds" in tool("curve_step_ab.py", "--help")
