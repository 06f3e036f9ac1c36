"""Anchored fine-tuning on the GPU: the two kernels of vd_anchor.hip bit for bit against their numpy float32 op sequences (every size at an
aligned base and one float past it, sentinels before and behind every output), the penalty sum exactly on integers and within its derived
bound on real data, and `Trainer(anchor=...)`: four optimiser steps against the oracle of tests/anchor_ref.py beside the plain trainer's, the
penalty readout, the absent keyword, gradient accumulation graphed and eager, the masked fine-tune, SAM, resume, the other two families;
`estimate_fisher` against the oracle's mean of squared autograd gradients; the tools and both drivers in child processes."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import anchor_ref  # noqa: E402
import anp_families_ref as fam  # noqa: E402
from oracle.loss_ref import SDE_VP, LossFnRef  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
import oracle.schedulers_ref as R  # noqa: E402
from villandiffusion_amd import actprune, anchor, lib, mitigation, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.anchor import AnchorConfig  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.trainer import EMAConfig, SAMConfig, Trainer  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = anchor_ref.SMALL
LAM = anchor_ref.LAM
SENTINEL = 123.5
GRID_CAP, BLOCK, FPT = ops.anchor_plan(1 << 40)
# scalar tail only (< 4), one item + tail, a workgroup boundary with tails, grid-stride with a tail; one n on each side of the grid cap, asked of
# vd_anchor_plan: the largest n every thread of the capped grid serves with its own four items, and the first n at which a thread strides on
SIZES = [1, 2, 3, 4, 5, 7, 2048, 2049, 2051, 100003, GRID_CAP * BLOCK * FPT - 1, GRID_CAP * BLOCK * FPT + 1]
f32 = np.float32


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


def scratch():
    """partial (1024 floats, a sentinel behind) and the penalty word (a sentinel behind)."""
    pb = torch.full((1028,), SENTINEL, device=DEV)
    ob = torch.full((5,), SENTINEL, device=DEV)
    return pb, pb[:1024], ob, ob[:1]


def ints(n, gen, lo, hi):
    return torch.randint(lo, hi + 1, (n,), generator=gen).float()


# ------------------------------------------------------------------------------------------------------------------- 1. the kernels
def test_the_plan_caps_the_grid_at_the_partial_buffer():
    assert (BLOCK, FPT) == (256, 16) and GRID_CAP <= 1024
    assert ops.anchor_plan(SIZES[-2])[0] == GRID_CAP == ops.anchor_plan(SIZES[-1])[0] and ops.anchor_plan(SIZES[-2] - BLOCK * FPT)[0] == GRID_CAP - 1


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_fisher_accum_is_the_numpy_sequence_bit_for_bit(n, shift):
    """Integers with s = 2^-2 (every operation exact, the order pinned all the same); real data with s = 1/3, three accumulations against the
    numpy recursion; a mixed pair of bases."""
    gen = g(n)
    F, gr = ints(n, gen, 0, 8), ints(n, gen, -8, 8)
    fb, fv = shifted(F, shift)
    gb, gv = shifted(gr, shift)
    ops.fisher_accum(fv, gv, 0.25)
    torch.cuda.synchronize()
    want = torch.from_numpy(anchor_ref.fisher_accum_ref(F.numpy(), gr.numpy(), 0.25))
    assert torch.equal(bits(fv), bits(want)) and torch.equal(bits(gv), bits(gr)) and untouched(fb, shift, n) and untouched(gb, shift, n)
    assert torch.equal(want, F + 0.25 * gr * gr)
    grs = [torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=gen)) for _ in range(3)]
    s = 1.0 / 3.0
    fb, fv = shifted(torch.zeros(n), shift)
    acc = np.zeros(n, dtype=f32)
    for k, gk in enumerate(grs):
        gb, gv = shifted(gk, shift if k != 1 else 1 - shift)        # the second accumulation from the other base: the scalar path, the same values
        ops.fisher_accum(fv, gv, s)
        acc = anchor_ref.fisher_accum_ref(acc, gk.numpy(), s)
        assert untouched(gb, shift if k != 1 else 1 - shift, n)
    torch.cuda.synchronize()
    assert torch.equal(bits(fv), bits(torch.from_numpy(acc))) and untouched(fb, shift, n)
    assert acc.dtype == f32 and float(acc.max()) > 0


def anchor_int_data(n, seed):
    """g in -8 .. 8, w and w0 in {-1, 0, 1} (d in -2 .. 2), F in {0, 1, 2} (one in four non-zero past 2^18 floats): every operation is exact with
    coef a power of two, every t * d is an integer <= 8 and every sum stays below 2^24."""
    gen = g(seed)
    gr, w, w0, F = ints(n, gen, -8, 8), ints(n, gen, -1, 1), ints(n, gen, -1, 1), ints(n, gen, 0, 2)
    if n > (1 << 18):
        F = F * (torch.randint(0, 4, (n,), generator=gen) == 0)
    return gr, w, w0, F


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_anchor_grad_on_integers_is_exact_in_g_and_in_the_penalty(n, shift):
    gr, w, w0, F = anchor_int_data(n, 500 + n)
    for ewc in (True, False):
        for with_pen in (True, False):
            bufs = [shifted(v, shift) for v in (gr, w, w0, F)]
            (gb, gv), (wb, wv), (w0b, w0v), (Fb, Fv) = bufs
            pb, partial, ob, out = scratch()
            ops.anchor_grad(gv, wv, w0v, Fv if ewc else None, 0.125, partial if with_pen else None, out if with_pen else None)
            torch.cuda.synchronize()
            want, t, d = anchor_ref.anchor_grad_ref(gr.numpy(), w.numpy(), w0.numpy(), F.numpy() if ewc else None, 0.125)
            assert torch.equal(bits(gv), bits(torch.from_numpy(want))), (n, shift, ewc, with_pen)
            assert all(torch.equal(bits(v), bits(h)) for (_, v), h in zip(bufs[1:], (w, w0, F)))      # w, w0, F untouched
            assert all(untouched(b, shift, n) for b, _ in bufs), (n, shift, ewc)
            if with_pen:
                pen = float((t.astype(np.float64) * d).sum())
                assert pen < 2 ** 24 and float(out) == pen, (n, shift, ewc, float(out), pen)
                assert bool((pb[1024:] == SENTINEL).all()) and bool((ob[1:] == SENTINEL).all())
            else:                                                              # pen NULL: neither the scratch nor the word is written
                assert bool((pb == SENTINEL).all()) and bool((ob == SENTINEL).all())
    assert n < 100 or not np.array_equal(want, gr.numpy())
    if shift:                                                                  # one operand off the common base: the scalar path, the same values
        (gb, gv), (_, wv), (_, w0v), (_, Fv) = shifted(gr, 0), shifted(w, 0), shifted(w0, 1), shifted(F, 0)
        pb, partial, ob, out = scratch()
        ops.anchor_grad(gv, wv, w0v, Fv, 0.125, partial, out)
        want, t, d = anchor_ref.anchor_grad_ref(gr.numpy(), w.numpy(), w0.numpy(), F.numpy(), 0.125)
        assert torch.equal(bits(gv), bits(torch.from_numpy(want))) and float(out) == float((t.astype(np.float64) * d).sum()) and untouched(gb, 0, n)


@pytest.mark.parametrize("n", [5, 2051, 100003, SIZES[-1]])
def test_anchor_grad_on_real_data_bits_in_g_and_the_bound_of_the_longest_chain(n):
    """g is the numpy float32 sequence bit for bit with an arbitrary coef.  The penalty against float64: |error| <= chain * 2^-24 * sum |t * d|
    over the float32 products the kernel adds, chain = the longest chain of additions include/villan_hip.h states for the launch shape
    vd_anchor_plan reports -- the first-order bound of a summation in which no partial sum passes through more additions than that.  The two
    bases and a repeat give the same bits."""
    gen = g(n)
    gr, w = torch.randn(n, generator=gen) * 1e-2, torch.randn(n, generator=gen) * 0.1
    w0, F = w + torch.randn(n, generator=gen) * 5e-3, torch.exp(1.5 * torch.randn(n, generator=gen))
    grid, block, _ = ops.anchor_plan(n)
    chain = anchor_ref.pen_chain(n, grid, block)
    assert chain == -(-((n + 3) // 4) // (grid * 256)) + -(-grid // 256) + 18
    for ewc in (True, False):
        want, t, d = anchor_ref.anchor_grad_ref(gr.numpy(), w.numpy(), w0.numpy(), F.numpy() if ewc else None, 0.37)
        terms = torch.from_numpy((t * d).astype(np.float64))                  # (t * d is the kernel's f32 product; the sum is what is bounded)
        got = []
        for shift in (0, 1, 0):
            (gb, gv), (_, wv), (_, w0v), (_, Fv) = (shifted(v, shift) for v in (gr, w, w0, F))
            pb, partial, ob, out = scratch()
            ops.anchor_grad(gv, wv, w0v, Fv if ewc else None, 0.37, partial, out)
            torch.cuda.synchronize()
            assert torch.equal(bits(gv), bits(torch.from_numpy(want))) and untouched(gb, shift, n), (n, shift, ewc)
            got.append(out.cpu())
        err, bound = abs(float(got[0].double()) - float(terms.sum())), anchor_ref.sum_bound(chain, terms)
        print(f"[anchor] penalty {'ewc' if ewc else 'l2sp'} n={n}: chain {chain}, error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (ewc, n, err, bound)
        assert torch.equal(bits(got[0]), bits(got[1])) and torch.equal(bits(got[0]), bits(got[2]))


@pytest.mark.parametrize("n", [3, 2051])
def test_at_the_anchor_the_gradient_keeps_its_bits_and_the_penalty_is_zero(n):
    gen = g(n)
    gr, w, F = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.rand(n, generator=gen) * 1e3
    for ewc in (True, False):
        for shift in (0, 1):
            (gb, gv), (_, wv), (_, w0v), (_, Fv) = (shifted(v, shift) for v in (gr, w, w.clone(), F))
            pb, partial, ob, out = scratch()
            ops.anchor_grad(gv, wv, w0v, Fv if ewc else None, 0.37, partial, out)
            torch.cuda.synchronize()
            want = anchor_ref.anchor_grad_ref(gr.numpy(), w.numpy(), w.numpy(), F.numpy() if ewc else None, 0.37)[0]
            assert torch.equal(bits(gv), bits(torch.from_numpy(want))) and float(out) == 0.0 and untouched(gb, shift, n)
            assert torch.equal(bits(gv), bits(gr))                            # g + coef * (F * 0) = g + 0 = g, bit for bit


def test_refusals_through_ctypes_on_device_buffers():
    h = lib.load()
    n = 64
    gr, w, w0, F = (torch.zeros(n, device=DEV) for _ in range(4))
    partial, out = torch.zeros(1024, device=DEV), torch.ones(1, device=DEV)
    Pp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(s=-1.0), dict(s=nan), dict(s=inf), dict(n=-1), dict(F=None), dict(g=None), dict(g=Pp(F))):
        a = dict(dict(F=Pp(F), g=Pp(gr), n=n, s=0.5), **bad)
        assert h.vd_fisher_accum(a["F"], a["g"], a["n"], a["s"], st) == -22, bad
    ok = dict(g=Pp(gr), w=Pp(w), w0=Pp(w0), F=Pp(F), n=n, coef=0.5, partial=Pp(partial), pen=Pp(out))
    for bad in (dict(coef=nan), dict(coef=inf), dict(n=-1), dict(g=None), dict(w=None), dict(w0=None), dict(partial=None), dict(w=Pp(gr)),
                dict(F=Pp(w0)), dict(pen=Pp(partial)), dict(w0=C.c_void_p(w.data_ptr() + 16))):
        a = dict(ok, **bad)
        assert h.vd_anchor_grad(a["g"], a["w"], a["w0"], a["F"], a["n"], a["coef"], a["partial"], a["pen"], st) == -22, bad
    assert h.vd_anchor_grad(Pp(gr), Pp(w), Pp(w0), None, n, 0.5, None, None, st) == 0           # L2-SP without a penalty: F, partial and pen NULL
    assert h.vd_anchor_grad(Pp(gr), Pp(w), Pp(w0), Pp(F), 0, 0.5, Pp(partial), Pp(out), st) == 0  # n = 0: the empty sum
    torch.cuda.synchronize()
    assert float(out) == 0.0 and float(gr.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- 2. the trainer
def batch_of(i):
    x0, Rr, t, eps = anchor_ref.batch_of(i)
    return {"target": x0.cuda(), "pixel_values": Rr.cuda()}, t.cuda(), eps.cuda()


def anchor_cfg(mode):
    s = anchor_ref.setup()
    return None if mode is None else AnchorConfig(lam=LAM, mode=mode, fisher=s["F"].clone() if mode == "ewc" else None)


def make_trainer(mode, seed=3, conv_math=None, w0=True, absent=False, lr=1e-3, **kw):
    """The small UNet at `seed` with the anchor of tests/anchor_ref.py (w0: its perturbed start; False: the weights at construction)."""
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=seed)
    if conv_math is not None:
        net.conv_math = conv_math
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    if absent:
        return Trainer(net, lf, lr=lr, total_steps=20, warmup_steps=0, **kw)
    aw = anchor_ref.setup()["w0"].clone() if (w0 and mode is not None) else None
    return Trainer(net, lf, lr=lr, total_steps=20, warmup_steps=0, anchor=anchor_cfg(mode), anchor_weights=aw, **kw)


def run_steps(tr, first, last):
    out = []
    for i in range(first, last):
        b, t, eps = batch_of(i)
        out.append(tr.train_step(b, t, noise=eps))
    torch.cuda.synchronize()
    return out


def start_state(net):
    return {k: net.flat_param[off:off + n].view(shape).detach().cpu().clone() for k, (off, n, shape) in net._offs.items()}


_PLAIN = {}


def plain_error(conv_math, accum=1, steps=4):
    """The plain trainer's update L2 error against the plain oracle over the same batches, measured once per arithmetic in this test run."""
    key = (conv_math, accum, steps)
    if key not in _PLAIN:
        o, s = anchor_ref.oracle_run(None, accum, steps), anchor_ref.setup()
        tr = make_trainer(None, conv_math=conv_math, grad_accum=accum)
        losses = run_steps(tr, 0, steps * accum)
        for i, l_ref in enumerate(o["losses"]):
            l = sum(float(x.detach()) for x in losses[i * accum:(i + 1) * accum]) / accum
            assert abs(l - l_ref) <= 1e-4 * abs(l_ref)
        _PLAIN[key] = anchor_ref.update_l2_error(start_state(tr.model), o["end"], s["start"])
    return _PLAIN[key]


@pytest.mark.parametrize("conv_math", ["bf16x3", "f32"])
@pytest.mark.parametrize("mode", anchor_ref.MODES)
def test_four_steps_follow_the_oracle_and_the_penalty_readout_is_the_oracles(mode, conv_math):
    """The update L2 error ||theta - theta_ref|| / ||theta_ref - theta_0|| against the oracle whose penalty is written in torch and differentiated
    by autograd, beside the plain trainer's against the plain oracle over the same batches.  The gate is 1.5x the plain trainer's figure of the
    same run: the added launch is elementwise f32, the convolutions' error dominates it; 1.5x is the margin the masked fine-tune uses.
    `anchor_penalty` after each step is the oracle's penalty at the weights that step started from, within the same relative figure.
    Measured on MI355X: bf16x3 L2-SP 2.14e-4, EWC 3.32e-4 beside the plain trainer's 4.09e-4; f32 1.57e-5, 2.70e-5 beside 4.51e-5; the penalty's
    relative error at most 8.0e-7."""
    s, o = anchor_ref.setup(), anchor_ref.oracle_run(mode)
    tr = make_trainer(mode, conv_math=conv_math)
    assert all(torch.equal(v, start_state(tr.model)[k]) for k, v in s["start"].items())
    base = plain_error(conv_math)
    gate = 1.5 * base
    pen_errs = []
    for i in range(4):
        (loss,) = run_steps(tr, i, i + 1)
        loss = float(loss.detach())
        assert abs(loss - o["losses"][i]) <= 1e-4 * abs(o["losses"][i]), (i, loss, o["losses"][i])
        pen_errs.append(abs(tr.anchor_penalty - o["penalties"][i]) / o["penalties"][i])
    assert tr.opt.step_count == tr.sched_step == 4 and int(tr.opt.skipped) == 0
    upd = anchor_ref.update_l2_error(start_state(tr.model), o["end"], s["start"])
    away = anchor_ref.update_l2_error(anchor_ref.oracle_run(None)["end"], o["end"], s["start"])
    print(f"[parity] 4 anchored optimiser steps ({mode}, {conv_math}): update L2 error {upd:.3e}; plain trainer {base:.3e}; gate {gate:.3e}; "
          f"penalty relative errors {['%.2e' % e for e in pen_errs]}; distance of the oracle's anchored trajectory from its plain one {away:.3f}")
    assert away >= 0.1                                                        # a missing penalty would be this far out
    assert upd <= gate, (upd, base)
    assert max(pen_errs) <= gate, (pen_errs, gate)


def test_anchor_none_is_the_trainer_without_the_keyword_launch_for_launch():
    none, absent, on = make_trainer(None), make_trainer(None, absent=True), make_trainer("ewc")
    assert none.anchor is None and none.anchor_penalty is None and "anchor" not in none.state_dict()
    names = {}
    for key, tr in (("none", none), ("absent", absent), ("on", on)):
        run_steps(tr, 0, 1)
        ops.profile_start()
        run_steps(tr, 1, 2)
        names[key] = [r["name"] for r in ops.profile_stop()]
    assert names["none"] == names["absent"] and not any("anchor" in n for n in names["none"])
    assert [n for n in names["on"] if "anchor" in n] == ["anchor_grad (anchor_grad_kernel)"]
    extra = list(names["on"])
    extra.remove("anchor_grad (anchor_grad_kernel)")
    assert extra == names["none"]                                             # one launch more, nothing else
    k = names["on"].index("anchor_grad (anchor_grad_kernel)")
    assert names["on"][k + 1].startswith("l2norm_sq")                        # after the backward, before the norm
    assert torch.equal(bits(none.model.flat_param), bits(absent.model.flat_param))
    assert torch.equal(bits(none.opt.exp_avg), bits(absent.opt.exp_avg)) and torch.equal(bits(none.opt.exp_avg_sq), bits(absent.opt.exp_avg_sq))
    assert not torch.equal(bits(on.model.flat_param), bits(none.model.flat_param))


def test_gradient_accumulation_graphed_is_eager_and_the_penalty_is_added_once_per_optimiser_step():
    """grad_accum = 2: flat_grad at the sync step is the MEAN gradient (the loss gradient is pre-divided by 2), so coef = lambda is right; the
    launch sits outside the captured micro-step, so graphed and eager steps agree bit for bit; against the oracle with one penalty per step."""
    eager, graphed = make_trainer("ewc", grad_accum=2, graph_micro_step=False), make_trainer("ewc", grad_accum=2)
    assert eager.graph_micro_step is False and graphed.graph_micro_step is True and eager.loss_fn.grad_scale == 0.5
    calls = []
    real = ops.anchor_grad
    ops.anchor_grad = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        run_steps(eager, 0, 4)
        assert len(calls) == 2                                                # four micro-steps, two optimiser steps, two launches
        run_steps(graphed, 0, 4)
    finally:
        ops.anchor_grad = real
    assert len(calls) == 4 and len(graphed._graphs) == 1 and eager.opt.step_count == graphed.opt.step_count == 2
    assert torch.equal(bits(graphed.model.flat_param), bits(eager.model.flat_param))
    assert torch.equal(bits(graphed.opt.exp_avg_sq), bits(eager.opt.exp_avg_sq)) and graphed.anchor_penalty == eager.anchor_penalty
    s, o = anchor_ref.setup(), anchor_ref.oracle_run("ewc", accum=2, steps=2)
    upd, base = anchor_ref.update_l2_error(start_state(eager.model), o["end"], s["start"]), plain_error(None, accum=2, steps=2)
    pen = abs(eager.anchor_penalty - o["penalties"][1]) / o["penalties"][1]
    print(f"[parity] 2 anchored optimiser steps of 2 micro-batches (ewc): update L2 error {upd:.3e}; plain trainer {base:.3e}; penalty error {pen:.2e}")
    assert upd <= 1.5 * base and pen <= 1.5 * base, (upd, pen, base)


def prune_scores(net, seed=11):
    tab = actprune.activation_table(net)
    gen = g(seed)
    return {name: torch.rand(tab.slices[name].stop - tab.slices[name].start, generator=gen) + 0.5 for name in tab.names}


@pytest.mark.parametrize("accum", [1, 2], ids=["eager", "graphed-accum2"])
def test_with_keep_pruned_the_pruned_rows_stay_bit_zero(accum):
    """The anchor is the UNPRUNED start (plus the perturbation): the penalty's gradient on a pruned row is lambda * F * (0 - w0) != 0, so the mask
    launch has to follow the anchor launch at every sync -- also where the replayed micro-step has masked flat_grad already."""
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=3)
    mask = actprune.fine_prune(net, prune_scores(net), fraction=0.1)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    tr = Trainer(net, lf, lr=1e-3, total_steps=20, warmup_steps=0, keep_pruned=mask, ema=EMAConfig(decay=0.999), grad_accum=accum,
                 anchor=anchor_cfg("ewc"), anchor_weights=anchor_ref.setup()["w0"].clone())
    assert tr.graph_micro_step is (accum == 2)
    drop = torch.zeros(net.flat_numel, dtype=torch.bool)
    for off, rows, ln, _, n0, _ in tr._keep_tab.jobs:
        for j in (mask.keep[n0:n0 + rows] == 0).nonzero().reshape(-1).tolist():
            drop[off + j * ln:off + (j + 1) * ln] = True
    assert int(drop.sum()) > 0 and float((tr._anchor_w0.cpu()[drop] * tr._anchor_F.cpu()[drop]).abs().sum()) > 0      # the pull is there
    for k in range(3):
        run_steps(tr, k * accum, (k + 1) * accum)
        for buf in (tr.model.flat_param, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.opt.ema):
            assert bool((bits(buf)[drop] == 0).all()), k                      # +0.0, the sign bit included
    assert tr.opt.step_count == 3 and int(tr.opt.skipped) == 0 and tr.anchor_penalty > 0
    assert float(tr.opt.exp_avg.cpu()[~drop].abs().sum()) > 0


def test_with_sam_the_penalty_is_added_once_at_w_and_the_network_is_restored():
    both = make_trainer("l2sp", sam=SAMConfig(rho=0.05))
    sam_only = make_trainer(None, sam=SAMConfig(rho=0.05))
    before = bits(both.model.flat_param)
    seen = []
    real = both._anchor_grad
    both._anchor_grad = lambda: (seen.append(bits(both.model.flat_param)), real())[1]
    run_steps(both, 0, 1)
    run_steps(sam_only, 0, 1)
    assert len(seen) == 1 and torch.equal(seen[0], before)                    # the launch ran after the second pass, with the network back at w
    assert torch.equal(bits(both._sam_backup), before) and float(both.sam_loss_perturbed) == float(sam_only.sam_loss_perturbed)
    want = 0.5 * LAM * float(((torch.from_numpy(before.numpy().view(f32)).double() - anchor_ref.setup()["w0"].double()) ** 2).sum())
    assert abs(both.anchor_penalty - want) <= 1e-5 * want
    assert not torch.equal(bits(both.model.flat_param), bits(sam_only.model.flat_param)) and both.opt.step_count == 1
    frozen = make_trainer("l2sp", sam=SAMConfig(rho=0.05), lr=0.0)
    run_steps(frozen, 0, 2)
    assert torch.equal(bits(frozen.model.flat_param), before)                 # lr = 0: perturb and restore leave every bit


def clone_state(sd):
    return {k: clone_state(v) if isinstance(v, dict) else (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in sd.items()}


def test_resume_with_the_same_anchor_continues_bit_for_bit_and_a_mismatch_is_refused():
    tr = make_trainer("ewc")
    run_steps(tr, 0, 2)
    st, p2 = clone_state(tr.state_dict()), tr.model.flat_param.detach().clone()
    assert st["anchor"] == {"lam": LAM, "mode": "ewc"} and not any(torch.is_tensor(v) for v in st["anchor"].values())
    assert sum(v.numel() for v in st["optimizer"].values() if torch.is_tensor(v)) == 2 * tr.model.flat_numel       # neither w0 nor F is stored
    run_steps(tr, 2, 4)
    again = make_trainer("ewc", seed=99)                                      # other weights: they come from the checkpoint, w0 and F from the caller
    with torch.no_grad():
        again.model.flat_param.copy_(p2)
    again.load_state_dict(st)
    run_steps(again, 2, 4)
    assert torch.equal(bits(again.model.flat_param), bits(tr.model.flat_param)) and again.opt.step_count == 4
    assert again.anchor_penalty == tr.anchor_penalty
    # an anchor taken from the resumed weights instead is another run
    wrong = make_trainer("ewc", seed=99, w0=False)
    with torch.no_grad():
        wrong.model.flat_param.copy_(p2)
        wrong._anchor_w0.copy_(p2)
    wrong.load_state_dict(st)
    run_steps(wrong, 2, 4)
    assert not torch.equal(bits(wrong.model.flat_param), bits(tr.model.flat_param))
    plain = make_trainer(None)
    with pytest.raises(ValueError, match="written with an anchor but this trainer was built without"):
        plain.load_state_dict(st)
    with pytest.raises(ValueError, match="written without an anchor but this trainer was built with"):
        make_trainer("l2sp").load_state_dict(clone_state(plain.state_dict()))


@pytest.mark.parametrize("family", ["ve", "ldm"])
def test_the_other_families_gradient_after_the_launch_is_plain_plus_the_numpy_penalty_gradient(family):
    def build(anchored):
        gen = g(7)
        if family == "ve":
            net = NCSNppModel(**dict(fam.SMALL_PP, layers_per_block=1))
            lf = LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0)
            x0, t = torch.rand(4, 3, 16, 16, generator=gen), torch.tensor(fam.VE_T)
        else:
            net = UNet2DModel(**fam.SMALL_LDM)
            lf = LossFn(S.DDPMScheduler(), "SDE-LDM", psi=1)
            x0, t = torch.randn(4, 3, 8, 8, generator=gen), torch.tensor(fam.LDM_T)
        net.reset_parameters(seed=5)
        Rr = torch.rand(x0.shape, generator=gen) * 0.5
        Rr[::2] = 0
        eps = torch.randn(x0.shape, generator=gen)
        n = net.flat_numel
        F, w0 = anchor_ref.fisher_of(n, seed=21), net.flat_param.detach().cpu() + 0.005 * torch.randn(n, generator=g(22))
        a = AnchorConfig(lam=0.37, mode="ewc", fisher=F) if anchored else None
        tr = Trainer(net, lf, lr=1e-3, total_steps=20, warmup_steps=0, anchor=a, anchor_weights=w0 if anchored else None)
        return tr, ({"target": x0.cuda(), "pixel_values": Rr.cuda()}, t.cuda(), eps.cuda()), F, w0

    tr, (b, t, eps), F, w0 = build(True)
    plain, _, _, _ = build(False)
    seen, plain_seen = [], []
    real, real_step = tr._anchor_grad, plain.opt.step

    def spy():
        before, w = tr.model.flat_grad.detach().cpu().clone(), tr.model.flat_param.detach().cpu().clone()
        real()
        seen.append((before, w, tr.model.flat_grad.detach().cpu().clone()))

    tr._anchor_grad = spy
    plain.opt.step = lambda *a, **k: (plain_seen.append(plain.model.flat_grad.detach().cpu().clone()), real_step(*a, **k))[1]
    for _ in range(2):
        loss = tr.train_step(b, t, noise=eps)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
    plain.train_step(b, t, noise=eps)
    assert len(seen) == 2 and int(tr.opt.skipped) == 0 and tr.opt.step_count == 2
    for before, w, after in seen:
        want = anchor_ref.anchor_grad_ref(before.numpy(), w.numpy(), w0.numpy(), F.numpy(), 0.37)[0]
        assert torch.equal(bits(after), bits(torch.from_numpy(want))) and not torch.equal(bits(after), bits(before)), family
    assert torch.equal(bits(seen[0][0]), bits(plain_seen[0]))                 # step one: the gradient before the launch is the plain trainer's
    assert tr.anchor_penalty > 0


# ------------------------------------------------------------------------------------------------------------------- 3. the Fisher estimate
def test_estimate_fisher_against_the_oracles_mean_of_squared_autograd_gradients():
    """3 batches of 2 on the small UNet.  Gate: max|F - F_ref| / max F_ref <= 2.5 * max_k (max|g_k - g_ref,k| / max|g_ref,k|), the right side
    measured here against the same oracle (|a^2 - b^2| = |a - b| |a + b|); that gradient error itself stays below 1e-3, the per-parameter gate
    of tests/test_unet_gpu.py for this arithmetic (which bounds this global figure a fortiori).  Two runs give the same bits, the weights keep
    theirs, flat_grad is zero afterwards, and "mean" gives mean 1."""
    s = anchor_ref.setup()
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=3)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    lf.grad_scale = 0.25                                                      # a trainer's leftover: the estimate must not see it, and must put it back
    batches = [anchor_ref.batch_of(k, B=2)[0] for k in range(3)]
    before = bits(net.flat_param)
    F = anchor.estimate_fisher(net, lf, batches, seed=5, normalize="none")
    torch.cuda.synchronize()
    assert lf.grad_scale == 0.25 and torch.equal(bits(net.flat_param), before) and float(net.flat_grad.abs().sum()) == 0.0
    assert F.dtype == torch.float32 and tuple(F.shape) == (net.flat_numel,) and F.device.type == "cuda"
    again = anchor.estimate_fisher(net, lf, batches, seed=5, normalize="none")
    assert torch.equal(bits(F), bits(again))
    assert not torch.equal(bits(F), bits(anchor.estimate_fisher(net, lf, batches, seed=6, normalize="none")))      # other draws
    # the oracle, and the trainer's gradient per batch beside it
    ref = UNet2DModelRef(**SMALL)
    ref.load_state_dict(s["start"])
    lref = LossFnRef(R.DDPMSchedulerRef(), SDE_VP, psi=1)
    F_ref, g_err = torch.zeros(net.flat_numel, dtype=torch.float64), 0.0
    for k, x0 in enumerate(batches):
        t, eps = anchor.fisher_draws(x0.shape, 1000, 5, k)
        ref.zero_grad()
        lref.p_loss(ref, x0, torch.zeros_like(x0), t, noise=eps).backward()
        g_ref = torch.zeros(net.flat_numel, dtype=torch.float64)
        for name, p in ref.named_parameters():
            off, n, _ = net._offs[name]
            g_ref[off:off + n] = p.grad.reshape(-1).double()
        F_ref += g_ref ** 2 / 3
        net.zero_grad()
        lf.grad_scale = 1.0
        lf.p_loss(net, x0.cuda(), torch.zeros_like(x0).cuda(), t.cuda(), noise=eps.cuda()).backward()
        g_err = max(g_err, float((net.flat_grad.cpu().double() - g_ref).abs().max() / g_ref.abs().max()))
    net.zero_grad()
    err = float((F.cpu().double() - F_ref).abs().max() / F_ref.max())
    print(f"[anchor] Fisher over 3 batches of 2: max error / max {err:.3e}; worst gradient error / max {g_err:.3e}; gate {2.5 * g_err:.3e}")
    assert g_err <= 1e-3, g_err
    assert err <= 2.5 * g_err, (err, g_err)
    Fm = anchor.estimate_fisher(net, lf, batches, seed=5)                     # the default: "mean"
    assert abs(float(Fm.mean(dtype=torch.float64)) - 1.0) <= 4 * 2.0 ** -24
    assert torch.equal(bits(Fm), bits(anchor.normalize_fisher(F, "mean")))
    assert float(anchor.estimate_fisher(net, lf, batches, seed=5, normalize="max").max()) == 1.0


# ------------------------------------------------------------------------------------------------------------------- 4. end to end
def test_removal_loop_default_is_untouched_and_the_penalty_rises_from_zero(monkeypatch):
    """lambda = 0.1 with F <= 4: after a step of lr = 2e-4 the penalty's gradient, lambda * F * d <= 8e-5, stays far below the removal loss's
    per-element gradient, so the weights keep drifting and the penalty at the start of each step does not fall."""
    tau = torch.rand(3, 32, 32, generator=g(8))

    def fresh():
        net = UNet2DModel(**SMALL)
        net.reset_parameters(seed=1)
        return net

    calls = []
    real = ops.anchor_grad
    monkeypatch.setattr(ops, "anchor_grad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    kw = dict(steps=3, batch=4, lr=2e-4, seed=2)
    a, b = fresh(), fresh()
    ra = mitigation.remove_backdoor(a, S.DDIMScheduler(), tau, **kw)
    rb = mitigation.remove_backdoor(b, S.DDIMScheduler(), tau, anchor_lambda=None, fisher=None, **kw)
    assert calls == [] and ra.anchor_penalty is None and rb.anchor_penalty is None and ra.anchor_lambda is None
    assert torch.equal(bits(a.flat_param), bits(b.flat_param)) and ra.total == rb.total
    F = anchor_ref.fisher_of(a.flat_numel).clamp(max=4.0)
    for fisher in (None, F):
        c = fresh()
        calls.clear()
        rc = mitigation.remove_backdoor(c, S.DDIMScheduler(), tau, anchor_lambda=0.1, fisher=fisher, **kw)
        pen = rc.anchor_penalty
        assert len(calls) == 3 and len(pen) == 3 and pen[0] == 0.0 and pen[0] <= pen[1] <= pen[2] and pen[2] > 0 and rc.anchor_lambda == 0.1
        assert rc.total[0] == ra.total[0] and not torch.equal(bits(c.flat_param), bits(a.flat_param))
        d = (c.flat_param - rc.frozen.flat_param).double().cpu()
        # the last entry is the penalty at the START of the last step; the weights moved once more since
        assert 0.5 * 0.1 * float(((1.0 if fisher is None else fisher.double()) * d * d).sum()) >= pen[2]


def small_checkpoint(tmp_path):
    """-> (the network, its checkpoint directory, the environment of a child process that finds it as SMALL-BASE)."""
    base_net = UNet2DModel(**SMALL)
    base_net.reset_parameters(seed=1)
    root = tmp_path / "ckpts"
    ckpt = str(root / "SMALL-BASE")
    P.DDPMPipeline(base_net, S.DDPMScheduler()).save_pretrained(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT, VILLAN_CKPT_ROOT=str(root), VILLAN_CFG_OVERRIDES=json.dumps({"eval_sample_n": 2, "lr_warmup_steps": 0}))
    return base_net, ckpt, env


def test_both_drivers_train_and_resume_in_child_processes(tmp_path):
    base_net, ckpt, env = small_checkpoint(tmp_path)
    fisher = anchor.save_fisher(str(tmp_path / "fisher.pt"), anchor_ref.fisher_of(base_net.flat_numel), base_net, 3, 2, "mean")
    # one optimiser step per epoch (128 synthetic images at batch 128)
    code = ("import sys; sys.argv=[%r]+%r; import villandiffusion_amd.dataset as D;"
            "D.synthetic_images=(lambda f: (lambda n=60000, **k: f(n=128, **k)))(D.synthetic_images);"
            "import %s as V; V.main()")

    def drive(driver, argv):
        out = subprocess.run([sys.executable, "-c", code % (driver + ".py", argv, driver)], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    def pen_of(stdout):
        lines = [ln for ln in stdout.splitlines() if " anchor_pen " in ln]
        assert len(lines) == 1 and " loss " in lines[0], stdout[-1000:]
        return float(lines[0].split(" anchor_pen ")[1].split()[0])

    common = ["--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--poison_rate", "0.1", "--trigger", "BOX_14", "--target", "HAT",
              "--ckpt", "SMALL-BASE", "--fclip", "o", "-o", "--sched", "DDIM-SCHED", "--infer_steps", "2", "--save_image_epochs", "1",
              "--save_model_epochs", "1"]
    for driver, extra, mode in (("VillanDiffusion", ["--anchor_lambda", "0.5", "--anchor_fisher", fisher], "ewc"),
                                ("rm_backdoor_VillanDiffusion", ["--anchor_lambda", "0.25"], "l2sp")):
        res = str(tmp_path / driver)
        out = drive(driver, ["--mode", "train", "--result", res] + extra + common)
        run = os.path.join(res, os.listdir(res)[0])
        args = json.load(open(os.path.join(run, "args.json")))
        assert args["anchor_lambda"] == float(extra[1]) and args["anchor_ckpt"] == "SMALL-BASE" and args.get("anchor_fisher") == (fisher if mode == "ewc" else None)
        st = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
        assert st["optimizer"]["step"] == 1 and st["anchor"] == {"lam": float(extra[1]), "mode": mode}
        assert pen_of(out) == 0.0                                             # the first step starts at the anchor
        # resume reads the flags from args.json and reloads w0 from --anchor_ckpt, not from the resumed weights: its step starts AWAY from the anchor
        out2 = drive(driver, ["--mode", "resume", "--ckpt", run])
        st2 = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
        assert st2["anchor"] == st["anchor"] and st2["optimizer"]["step"] == 2
        assert pen_of(out2) > 0.0


def test_the_tools_in_child_processes(tmp_path):
    base_net, ckpt, env = small_checkpoint(tmp_path)

    def tool(name, *argv):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + list(argv), cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    # tools/estimate_fisher.py on a synthetic dataset
    fisher = str(tmp_path / "fisher.pt")
    line = json.loads(tool("estimate_fisher.py", "--ckpt", ckpt, "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "6", "--batch", "2", "--seed", "1",
                           "--out", fisher).strip().splitlines()[-1])
    assert (line["family"], line["n_clean"], line["batch"], line["n_batches"], line["normalize"], line["numel"]) == \
        ("vp", 6, 2, 3, "mean", base_net.flat_numel) and 0 < line["mean"] < line["max"] and 0 <= line["share_below_1e-12_max"] < 1
    F, meta = anchor.load_fisher(fisher, base_net, with_meta=True)
    assert meta["n_batches"] == 3 and meta["batch"] == 2 and meta["normalize"] == "mean" and abs(float(F.mean(dtype=torch.float64)) - 1) < 1e-6
    side = json.load(open(str(tmp_path / "fisher.json")))
    assert side["mean"] == line["mean"] and side["layout_sha256"] == anchor.layout_digest(base_net)

    # tools/remove_backdoor.py: anchored, and at its defaults
    trig = str(tmp_path / "trigger_inv.pt")
    tau = torch.rand(3, 32, 32, generator=g(8))
    torch.save(tau, trig)
    out_a, out_d = str(tmp_path / "repaired_anchored"), str(tmp_path / "repaired")
    rm = ["--ckpt", ckpt, "--trigger", trig, "--steps", "3", "--batch", "4", "--seed", "2"]
    tool("remove_backdoor.py", *rm, "--out", out_a, "--anchor_lambda", "0.1")
    info = json.load(open(os.path.join(out_a, "removal.json")))
    pen = info["anchor_penalty"]
    assert info["anchor_lambda"] == 0.1 and info["anchor_fisher"] is None and len(pen) == 3 and pen[0] == 0.0 and pen[0] <= pen[1] <= pen[2] and pen[2] > 0
    tool("remove_backdoor.py", "--ckpt", ckpt, "--trigger", trig, "--steps", "2", "--batch", "2", "--out", str(tmp_path / "repaired_ewc"),
         "--anchor_lambda", "0.1", "--anchor_fisher", fisher)
    ewc = json.load(open(str(tmp_path / "repaired_ewc" / "removal.json")))
    assert ewc["anchor_fisher"] == fisher and ewc["anchor_penalty"][0] == 0.0 and 0 < ewc["anchor_penalty"][1] < float("inf")
    tool("remove_backdoor.py", *rm, "--out", out_d)
    info_d = json.load(open(os.path.join(out_d, "removal.json")))
    assert not any(k.startswith("anchor") for k in info_d) and info_d["total"][0] == info["total"][0]
    twin = UNet2DModel(**SMALL)
    twin.flat_param.data.copy_(base_net.flat_param)
    twin.weights_changed()
    res = mitigation.remove_backdoor(twin, S.DDIMScheduler(), tau, steps=3, batch=4, lr=2e-4, seed=2)      # a call without the keyword
    fixed, anchored = P.DiffusionPipeline.from_pretrained(out_d), P.DiffusionPipeline.from_pretrained(out_a)
    assert info_d["shift"] == res.shift and torch.equal(bits(fixed.unet.flat_param), bits(twin.flat_param))
    assert not torch.equal(bits(anchored.unet.flat_param), bits(twin.flat_param))
