"""Sharpness-aware fine-tuning on the GPU: the four kernels of vd_sam.hip bit for bit on integers and within derived bounds on real data (every
size at an aligned base and one float past it, sentinels behind every output), their refusals, and `Trainer(sam=...)`: the bit-exact restore,
the eager path at rho = 0, four optimiser steps against the oracle of tests/sam_ref.py beside the plain trainer's, EMA, the loss split, the
other two families, resume, and the drivers in child processes."""
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

import anp_families_ref as fam  # noqa: E402
import sam_ref  # noqa: E402
import test_anp_families_gpu as anp_fam_tables  # noqa: E402
import test_anp_gpu as anp_tables  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import anp, lib, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.pipelines import DDPMPipeline  # noqa: E402
from villandiffusion_amd.trainer import EMAConfig, SAMConfig, Trainer, ema_decay_at  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = sam_ref.SMALL
EINVAL = -22
SENTINEL = 123.5
GRID_CAP, BLOCK, FPT = (lambda p: (p[0], p[1], p[2]))(ops.sam_plan(1 << 40))
# scalar tail only (< 4), one item + tail, a workgroup boundary with tails, grid-stride with a tail; one n on each side of the grid cap: the
# largest n every thread of the capped grid serves with its own four items, and the first n at which a thread strides on
SIZES = [1, 2, 3, 4, 5, 7, 2048, 2049, 2051, 100003, GRID_CAP * BLOCK * FPT - 1, GRID_CAP * BLOCK * FPT + 1]
MODES = ("sam", "asam")
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
    """partial (1024 floats, a sentinel behind) and the norm word (a sentinel behind)."""
    pb = torch.full((1028,), SENTINEL, device=DEV)
    ob = torch.full((5,), SENTINEL, device=DEV)
    return pb, pb[:1024], ob, ob[:1]


def integer_data(n, seed, lim):
    gen = g(seed)
    return torch.randint(-lim, lim + 1, (n,), generator=gen).float(), torch.randint(-lim, lim + 1, (n,), generator=gen).float()


# ------------------------------------------------------------------------------------------------------------------- 1. the flat kernels
def test_the_plan_caps_the_grid_at_the_partial_buffer():
    assert (BLOCK, FPT) == (256, 16) and GRID_CAP <= 1024
    assert ops.sam_plan(SIZES[-2])[0] == GRID_CAP == ops.sam_plan(SIZES[-1])[0] and ops.sam_plan(SIZES[-2] - BLOCK * FPT)[0] == GRID_CAP - 1


def perturb_ref(w, gr, mode, eta, rho, nsq):
    """The numpy float32 op sequence of vd_sam_perturb."""
    w, gr = w.numpy(), gr.numpy()
    c = f32(rho) / (np.sqrt(f32(nsq)) + f32(1e-12))
    if mode == "sam":
        return torch.from_numpy(w + c * gr)
    T = np.abs(w) + f32(eta)
    return torch.from_numpy(w + ((c * T) * T) * gr)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_perturb_is_the_numpy_sequence_bit_for_bit_on_integers(n, shift):
    """|w|, |g| <= 8, eta = 1/2, *norm_sq = 16, rho = 1/2, so c = 2^-3: every operation is exact, and the kernel's order is pinned all the same."""
    w, gr = integer_data(n, n, 8)
    nsq = torch.full((1,), 16.0, device=DEV)
    assert float(f32(0.5) / (np.sqrt(f32(16.0)) + f32(1e-12))) == 0.125
    for mode in MODES:
        for with_backup in (True, False):
            wb, wv = shifted(w, shift)
            gb, gv = shifted(gr, shift)
            bb, bv = shifted(torch.full((n,), -7.25), shift)
            ops.sam_perturb(wv, gv, bv if with_backup else None, nsq, 0.5, mode, 0.5)
            torch.cuda.synchronize()
            want = perturb_ref(w, gr, mode, 0.5, 0.5, 16.0)
            assert torch.equal(bits(wv), bits(want)), (n, shift, mode)
            assert torch.equal(bits(bv), bits(w if with_backup else torch.full((n,), -7.25))), (n, shift, mode)
            assert torch.equal(bits(gv), bits(gr))
            assert untouched(wb, shift, n) and untouched(gb, shift, n) and untouched(bb, shift, n), (n, shift, mode)
    assert not torch.equal(want, w) or n < 4
    # a mixed pair of bases takes the scalar path too, with the same values
    if shift:
        wb, wv = shifted(w, 0)
        gb, gv = shifted(gr, 1)
        ops.sam_perturb(wv, gv, None, nsq, 0.5, "asam", 0.5)
        assert torch.equal(bits(wv), bits(perturb_ref(w, gr, "asam", 0.5, 0.5, 16.0))) and untouched(wb, 0, n)


def norm_data(n, seed):
    """w in {-1, 0, 1}, g in {-2 .. 2} (one in four non-zero past 2^18 floats): every u^2 is a multiple of 1/4 and every sum stays below 2^22."""
    gen = g(seed)
    w = torch.randint(-1, 2, (n,), generator=gen).float()
    gr = torch.randint(-2, 3, (n,), generator=gen).float()
    if n > (1 << 18):
        gr = gr * (torch.randint(0, 4, (n,), generator=gen) == 0)
    return w, gr


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "+4B"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_sq_equals_the_integer_sum(n, shift):
    w, gr = norm_data(n, 1000 + n)
    for mode in MODES:
        u = gr.double() if mode == "sam" else (w.double().abs() + 0.5) * gr.double()
        want = float((u * u).sum())
        assert want < 2 ** 22 and want * 4 == int(want * 4)
        wb, wv = shifted(w, shift)
        gb, gv = shifted(gr, shift)
        pb, partial, ob, out = scratch()
        ops.sam_norm_sq(gv, None if mode == "sam" else wv, partial, out, mode, 0.5)
        torch.cuda.synchronize()
        assert float(out) == want, (n, shift, mode, float(out), want)
        assert bool((pb[1024:] == SENTINEL).all()) and bool((ob[1:] == SENTINEL).all()) and untouched(wb, shift, n) and untouched(gb, shift, n)
        assert torch.equal(bits(wv), bits(w)) and torch.equal(bits(gv), bits(gr))
    if n >= 4:                                                                # "sam" is ops.l2norm_sq's quantity
        gb, gv = shifted(gr, 0)
        pb, partial, ob, out = scratch()
        assert float(ops.l2norm_sq(gv, partial, out)) == float((gr.double() ** 2).sum())


@pytest.mark.parametrize("n", [2051, 100003, SIZES[-1]])
def test_norm_sq_on_real_data_is_within_the_bound_of_its_longest_chain(n):
    """Against float64: |error| <= chain * 2^-24 * sum |terms|, chain = the longest chain of additions include/villan_hip.h states for the
    launch shape vd_sam_plan reports.  The two bases give the same bits, and so does a repeat."""
    gen = g(n)
    w, gr = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 1e-2
    grid, block, _ = ops.sam_plan(n)
    chain = sam_ref.norm_chain(n, grid, block)
    assert chain == -(-((n + 3) // 4) // (grid * 256)) + -(-grid // 256) + 18
    for mode in MODES:
        eta = f32(0.01)
        u = gr.double() if mode == "sam" else (w.double().abs() + float(eta)) * gr.double()
        terms = u * u
        got = []
        for shift in (0, 1, 0):
            _, wv = shifted(w, shift)
            _, gv = shifted(gr, shift)
            pb, partial, ob, out = scratch()
            ops.sam_norm_sq(gv, wv, partial, out, mode, 0.01)
            got.append(out.cpu())
        err, bound = abs(float(got[0].double()) - float(terms.sum())), sam_ref.sum_bound(chain, terms)
        print(f"[sam] norm_sq {mode} n={n}: chain {chain}, error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (mode, n, err, bound)
        assert torch.equal(bits(got[0]), bits(got[1])) and torch.equal(bits(got[0]), bits(got[2]))


@pytest.mark.parametrize("n", [3, 2051])
def test_a_degenerate_norm_leaves_the_weights_alone_and_still_writes_the_backup(n):
    w, gr = torch.randn(n, generator=g(1)), torch.randn(n, generator=g(2))
    for bad in (float("inf"), float("nan"), 0.0, -0.0):
        for mode in MODES:
            for shift in (0, 1):
                wb, wv = shifted(w, shift)
                _, gv = shifted(gr, shift)
                bb, bv = shifted(torch.zeros(n), shift)
                ops.sam_perturb(wv, gv, bv, torch.full((1,), bad, device=DEV), 0.5, mode, 0.01)
                assert torch.equal(bits(wv), bits(w)) and torch.equal(bits(bv), bits(w)) and untouched(wb, shift, n) and untouched(bb, shift, n)
    # real data, a real norm: two runs give the same bits, and they are the numpy sequence's
    nsq = torch.full((1,), 0.37, device=DEV)
    for mode in MODES:
        runs = []
        for _ in range(2):
            _, wv = shifted(w, 0)
            _, gv = shifted(gr, 0)
            ops.sam_perturb(wv, gv, None, nsq, 0.05, mode, 0.01)
            runs.append(bits(wv))
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], bits(perturb_ref(w, gr, mode, 0.01, 0.05, float(nsq))))


# ------------------------------------------------------------------------------------------------------------------- 2. the neuron kernels
def big_table():
    """Jobs of 300, 1 and 700 rows: a thread of vd_sam_neuron_coef's one workgroup walks up to 2 + 1 + 3 rows."""
    jobs = [(0, 300, 7, -1, 0, 0), (2100, 1, 5, -1, 300, 75), (2108, 700, 3, -1, 301, 76)]
    return anp.NeuronTable(jobs, 1001, {f"job{k}": slice(j[4], j[4] + j[1]) for k, j in enumerate(jobs)})


TABLES = {"anp": lambda: anp_tables.synthetic_table()[0], "families": lambda: anp_fam_tables.synthetic_table()[0], "big": big_table}


def coef_ref(wsq, gsq, tab, rho, eta, nsq):
    """The numpy float32 op sequence of the elementwise parts of vd_sam_neuron_coef, from the norm the kernel wrote."""
    ln = np.concatenate([np.full(j[1], j[2], dtype=f32) for j in tab.jobs])
    T = np.sqrt(wsq.numpy() / ln) + f32(eta)
    c = f32(rho) / (np.sqrt(f32(nsq)) + f32(1e-12))
    return T, torch.from_numpy((c * T) * T)


@pytest.mark.parametrize("which", list(TABLES))
def test_neuron_coef_sum_is_within_its_bound_and_its_elementwise_parts_are_exact(which):
    tab = TABLES[which]()
    n = tab.n_neurons
    chain = sam_ref.coef_chain(tab.jobs)
    assert chain == sum((j[1] + 255) // 256 for j in tab.jobs) + 8
    wsq, gsq = torch.rand(n, generator=g(5)) * 40 + 1e-3, torch.rand(n, generator=g(6)) * 1e-2
    runs = []
    for _ in range(2):
        cb, coef = shifted(torch.zeros(n), 0)
        ob, out = shifted(torch.zeros(1), 0)
        ops.sam_neuron_coef(wsq.to(DEV), gsq.to(DEV), tab, coef, out, 0.5, 0.01)
        torch.cuda.synchronize()
        assert untouched(cb, 0, n) and untouched(ob, 0, 1)
        runs.append((bits(coef), bits(out)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    T, want = coef_ref(wsq, gsq, tab, 0.5, 0.01, float(out))
    assert torch.equal(bits(coef), bits(want))                                 # sqrt and the divisions are correctly rounded
    terms = torch.from_numpy(T * T).double() * gsq.double()                    # (T * T is the kernel's f32 product; the sum is what is bounded)
    err, bound = abs(float(out.double()) - float(terms.sum())), sam_ref.sum_bound(chain, terms)
    print(f"[sam] neuron_coef {which}: {n} neurons, chain {chain}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    for bad in (float("inf"), float("nan"), 0.0):                              # a norm that is inf, nan or 0: every coefficient is 0
        gz = torch.full((n,), bad)
        coef = torch.full((n,), 7.0, device=DEV)
        ops.sam_neuron_coef(wsq.to(DEV), gz.to(DEV), tab, coef, out, 0.5, 0.01)
        assert float(coef.abs().sum()) == 0.0 and (float(out) == bad or bad != bad)


@pytest.mark.parametrize("shifts", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "both+4B", "w+4B"])
@pytest.mark.parametrize("which", ["anp", "families"])
def test_neuron_axpy_is_exact_with_power_of_two_coefficients(which, shifts):
    """ANP's test tables: row lengths 3 .. 16128, aligned and unaligned rows.  Bias slots and the floats between the jobs keep their bits."""
    tab, numel = (anp_tables if which == "anp" else anp_fam_tables).synthetic_table()
    if which == "families":
        assert {3, 16128} <= {j[2] for j in tab.jobs}
    gen = g(11)
    w = torch.randint(-8, 9, (numel,), generator=gen).float()
    gr = torch.randint(-8, 9, (numel,), generator=gen).float()
    inside = torch.zeros(numel, dtype=torch.bool)
    for off, rows, ln, *_ in tab.jobs:
        inside[off:off + rows * ln] = True
    w[~inside] = float("nan")                                                 # gaps, bias slots and the tail: a NaN no kernel may replace
    coef = 2.0 ** torch.randint(-3, 3, (tab.n_neurons,), generator=gen).float() * (1 - 2 * torch.randint(0, 2, (tab.n_neurons,), generator=gen)).float()
    want = w.clone()
    for off, rows, ln, _, n0, _ in tab.jobs:
        want[off:off + rows * ln] = (w[off:off + rows * ln].view(rows, ln) + coef[n0:n0 + rows, None] * gr[off:off + rows * ln].view(rows, ln)).reshape(-1)
    w_d, g_d = anp_tables.on_device(w, shifts[1]), anp_tables.on_device(gr, shifts[0])
    ops.neuron_axpy(w_d, g_d, tab, coef.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(w_d), bits(want)) and torch.equal(bits(g_d), bits(gr))
    assert int(torch.isnan(want).sum()) == numel - tab.weight_floats and not torch.equal(bits(want), bits(w))


def test_refusals_through_ctypes():
    h = lib.load()
    n = 64
    w, gr, b = (torch.zeros(n, device=DEV) for _ in range(3))
    partial, out = torch.zeros(1024, device=DEV), torch.ones(1, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    ok_norm = dict(g=P(gr), w=P(w), n=n, mode=1, eta=0.01, partial=P(partial), out=P(out))
    for bad in (dict(mode=2), dict(mode=-1), dict(eta=-0.5), dict(eta=nan), dict(eta=inf), dict(n=-1), dict(g=None), dict(w=None), dict(partial=None),
                dict(out=None)):
        a = dict(ok_norm, **bad)
        assert h.vd_sam_norm_sq(a["g"], a["w"], a["n"], a["mode"], a["eta"], a["partial"], a["out"], st) == EINVAL, bad
    assert h.vd_sam_norm_sq(P(gr), None, n, 0, 0.01, P(partial), P(out), st) == 0        # mode 0 needs no w
    ok_p = dict(w=P(w), g=P(gr), b=P(b), n=n, mode=0, eta=0.01, rho=0.05, nsq=P(out))
    for bad in (dict(mode=2), dict(rho=-1.0), dict(rho=nan), dict(rho=inf), dict(eta=-1.0), dict(eta=nan), dict(n=-1), dict(w=None), dict(g=None),
                dict(nsq=None), dict(g=P(w)), dict(b=P(w)), dict(b=C.c_void_p(gr.data_ptr() + 16))):
        a = dict(ok_p, **bad)
        assert h.vd_sam_perturb(a["w"], a["g"], a["b"], a["n"], a["mode"], a["eta"], a["rho"], a["nsq"], st) == EINVAL, bad
    assert h.vd_sam_perturb(P(w), P(gr), None, n, 0, 0.01, 0.05, P(out), st) == 0         # backup may be NULL
    assert h.vd_sam_perturb(P(w), P(gr), P(b), 0, 0, 0.01, 0.05, P(out), st) == 0         # n = 0: nothing to do
    tab = big_table()
    table = tab.device_table(DEV)
    v = torch.ones(tab.n_neurons, device=DEV)
    ok_c = dict(wsq=P(v), gsq=P(v), table=P(table), jobs=tab.n_jobs, nn=tab.n_neurons, rho=0.5, eta=0.01, coef=P(torch.zeros_like(v)), nsq=P(out))
    for bad in (dict(rho=-1.0), dict(rho=nan), dict(eta=-1.0), dict(eta=inf), dict(wsq=None), dict(gsq=None), dict(table=None), dict(coef=None),
                dict(nsq=None), dict(jobs=0), dict(nn=0)):
        a = dict(ok_c, **bad)
        assert h.vd_sam_neuron_coef(a["wsq"], a["gsq"], a["table"], a["jobs"], a["nn"], a["rho"], a["eta"], a["coef"], a["nsq"], st) == EINVAL, bad
    big = torch.zeros(tab.extent, device=DEV)
    for bad in ((None, P(big)), (P(big), None), (P(big), P(big))):
        assert h.vd_neuron_axpy(bad[0], bad[1], P(table), tab.n_jobs, tab.total_blocks, P(v), st) == EINVAL
    assert h.vd_neuron_axpy(P(big), P(torch.zeros_like(big)), None, tab.n_jobs, tab.total_blocks, P(v), st) == EINVAL
    assert h.vd_neuron_axpy(P(big), P(torch.zeros_like(big)), P(table), tab.n_jobs, 0, P(v), st) == EINVAL
    assert h.vd_neuron_axpy(P(big), P(torch.zeros_like(big)), P(table), tab.n_jobs, tab.total_blocks, None, st) == EINVAL
    torch.cuda.synchronize()
    assert float(w.abs().sum()) == 0.0 and "vd_neuron_axpy" in lib.last_error()
    e0 = ops.WEIGHTS_EPOCH                                                    # the kernels that write weights bump nothing themselves
    ops.sam_perturb(w, gr, b, out, 0.05)
    ops.neuron_axpy(big, torch.zeros_like(big), tab, v)
    assert ops.WEIGHTS_EPOCH == e0


# ------------------------------------------------------------------------------------------------------------------- 3. the trainer
def batch_of(i, flags=False):
    x0, Rr, t, eps = sam_ref.batch_of(i)
    b = {"target": x0.cuda(), "pixel_values": Rr.cuda()}
    if flags:
        b["is_clean"] = torch.tensor([True, False, True, False], device=DEV)  # (R[::2] = 0: the even samples are the clean ones)
    return b, t.cuda(), eps.cuda()


def make_trainer(sam, seed=3, lr=1e-3, conv_math=None, lf=None, **kw):
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=seed)
    if conv_math is not None:
        net.conv_math = conv_math
    lf = lf if lf is not None else LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    return Trainer(net, lf, lr=lr, total_steps=20, warmup_steps=0, sam=sam, **kw)


def cfg_of(case):
    mode, rho, eta, layers = sam_ref.CASES[case]
    return SAMConfig(rho=rho, mode=mode, eta=eta, layers=layers)


def run_steps(tr, first, last, noise=True):
    out = []
    for i in range(first, last):
        b, t, eps = batch_of(i)
        out.append(tr.train_step(b, t, noise=eps if noise else None))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(sam_ref.CASES))
def test_restore_is_bit_exact_also_after_an_exception_in_the_second_pass(case):
    tr = make_trainer(cfg_of(case), lr=0.0)
    assert tr.graph_micro_step is False and tr.state_dict()["sam"] == {k: v for k, v in zip(("mode", "rho", "eta", "layers"), sam_ref.CASES[case])}
    before = bits(tr.model.flat_param)
    e0 = ops.WEIGHTS_EPOCH
    (loss,) = run_steps(tr, 0, 1)
    assert torch.equal(bits(tr.model.flat_param), before) and tr.opt.step_count == 1
    assert ops.WEIGHTS_EPOCH >= e0 + 3                                        # perturb, restore, Adam
    assert float(tr.sam_loss_perturbed) != float(loss.detach()) and float(tr.model.flat_grad.abs().sum()) == 0.0
    assert torch.equal(bits(tr._sam_backup), before)
    # an exception in pass 2: the network is back at w, nothing was stepped, and the next step is the one a fresh trainer takes
    tr = make_trainer(cfg_of(case))
    twin = make_trainer(cfg_of(case))
    lf, calls = tr.loss_fn, []
    real = lf.p_loss_by_keys

    def failing(*a, **k):
        calls.append(bits(tr.model.flat_param))
        if len(calls) == 2:
            raise ZeroDivisionError("pass 2")
        return real(*a, **k)

    lf.p_loss_by_keys = failing
    b, t, eps = batch_of(0)
    with pytest.raises(ZeroDivisionError):
        tr.train_step(b, t, noise=eps)
    lf.p_loss_by_keys = real
    assert torch.equal(calls[0], before) and not torch.equal(calls[1], before)   # pass 2 was about to run at w + e
    moved = calls[1] != calls[0]
    if case == "neuron":                                                      # only weight rows of the table moved
        inside = torch.zeros(tr.model.flat_numel, dtype=torch.bool)
        for off, rows, ln, *_ in tr._sam_tab.jobs:
            inside[off:off + rows * ln] = True
        assert not bool(moved[~inside].any()) and int(moved.sum()) > 0.9 * tr._sam_tab.weight_floats
    assert torch.equal(bits(tr.model.flat_param), before) and tr.opt.step_count == 0 and tr.sched_step == 0 and tr.micro == 0
    tr.model.zero_grad()
    run_steps(tr, 0, 2)
    run_steps(twin, 0, 2)
    assert torch.equal(bits(tr.model.flat_param), bits(twin.model.flat_param)) and not torch.equal(bits(twin.model.flat_param), before)


@pytest.mark.parametrize("case", list(sam_ref.CASES))
def test_the_eager_path_is_untouched_by_rho_zero(case):
    """SAMConfig(rho=0) is refused, so the launches are given rho = 0 through the trainer's private copy: norm, perturb (w + 0 g), the second
    pass and the restore all run, and four steps end on the bits of a plain eager trainer.  "sam" draws its own noise: a SAM step consumes
    the random stream as a plain step does."""
    own_noise = case == "sam"
    tr, plain = make_trainer(cfg_of(case)), make_trainer(None)
    assert plain.sam is None and plain.graph_micro_step is False and "sam" not in plain.state_dict()
    tr._sam_rho = 0.0
    for t_ in (tr, plain):
        t_.loss_fn.noise_seed = 4321
    la = run_steps(tr, 0, 4, noise=not own_noise)
    lb = run_steps(plain, 0, 4, noise=not own_noise)
    assert tr.loss_fn._noise_off == plain.loss_fn._noise_off and (tr.loss_fn._noise_off > 0) == own_noise
    assert [float(x.detach()) for x in la] == [float(x.detach()) for x in lb] and float(tr.sam_loss_perturbed) == float(la[-1].detach())
    assert torch.equal(bits(tr.model.flat_param), bits(plain.model.flat_param))
    assert bool((tr.opt.exp_avg == plain.opt.exp_avg).all()) and bool((tr.opt.exp_avg_sq == plain.opt.exp_avg_sq).all())   # (the sign of a zero may differ)
    assert tr.opt.step_count == plain.opt.step_count == 4 and int(tr.opt.skipped) == 0


_ORACLE, _PLAIN = {}, {}


def start_state(net):
    return {k: net.flat_param[off:off + n].view(shape).detach().cpu().clone() for k, (off, n, shape) in net._offs.items()}


def oracle_run(case):
    """Four optimiser steps of tests/sam_ref.py's step from the trainer's start (seed 3); computed once per case, shared read-only."""
    if case not in _ORACLE:
        twin = UNet2DModel(**SMALL, device="cpu")
        twin.reset_parameters(seed=3)
        ref = UNet2DModelRef(**SMALL)
        ref.load_state_dict(start_state(twin))
        if case == "plain":
            o = sam_ref.SamOnOracle(ref, None)
        else:
            mode, rho, eta, layers = sam_ref.CASES[case]
            o = sam_ref.SamOnOracle(ref, mode, rho, eta, rows=anp.neuron_table(twin, layers).slices)
        losses = [o.step(*sam_ref.batch_of(i)) for i in range(4)]
        _ORACLE[case] = dict(start=start_state(twin), losses=losses, end={k: v.detach().clone() for k, v in ref.named_parameters()})
    return _ORACLE[case]


def plain_error(conv_math):
    """The plain trainer's update L2 error over the same four batches, measured once per arithmetic in this test run."""
    if conv_math not in _PLAIN:
        o = oracle_run("plain")
        tr = make_trainer(None, conv_math=conv_math)
        losses = run_steps(tr, 0, 4)
        for l, (l_ref, _) in zip(losses, o["losses"]):
            assert abs(float(l) - l_ref) <= 1e-4 * abs(l_ref)
        _PLAIN[conv_math] = sam_ref.update_l2_error(start_state(tr.model), o["end"], o["start"])
    return _PLAIN[conv_math]


@pytest.mark.parametrize("conv_math", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", list(sam_ref.CASES))
def test_four_steps_follow_the_oracle(case, conv_math):
    """Loss of both passes within 1e-4 relative per step; the update L2 error ||theta - theta_ref|| / ||theta_ref - theta_0|| below the project's
    trajectory gate of 1e-3, and within 8x the plain trainer's over the same batches or 3e-4, whichever is larger (two passes each add their
    gradient error, and the second starts from weights that carry the first's; 8x is a margin, not an expectation).
    Measured on MI355X: bf16x3 sam 3.98e-4, asam 5.69e-4, neuron 2.92e-4 beside the plain trainer's 4.09e-4; f32 4.83e-5, 3.39e-5, 3.52e-5
    beside 4.51e-5 (this network at lr = 1e-3; tests/test_train_sample_gpu.py records 6e-5 and 1.2e-5 for the full network at lr = 2e-4)."""
    o = oracle_run(case)
    tr = make_trainer(cfg_of(case), conv_math=conv_math)
    assert all(torch.equal(v, start_state(tr.model)[k]) for k, v in o["start"].items())
    for i in range(4):
        b, t, eps = batch_of(i)
        loss = tr.train_step(b, t, noise=eps)
        l1, l2 = o["losses"][i]
        assert abs(float(loss) - l1) <= 1e-4 * abs(l1), (i, float(loss), l1)
        assert abs(float(tr.sam_loss_perturbed) - l2) <= 1e-4 * abs(l2), (i, float(tr.sam_loss_perturbed), l2)
        if i == 0:
            assert float(tr.sam_loss_perturbed) > float(loss) and l2 > l1      # the first ascent step goes uphill
    assert tr.opt.step_count == tr.sched_step == 4 and int(tr.opt.skipped) == 0
    upd = sam_ref.update_l2_error(start_state(tr.model), o["end"], o["start"])
    base = plain_error(conv_math)
    away = sam_ref.update_l2_error(oracle_run("plain")["end"], o["end"], o["start"])
    print(f"[parity] 4 SAM optimiser steps ({case}, {conv_math}): update L2 error {upd:.3e}; plain trainer {base:.3e}; "
          f"distance of the oracle's SAM trajectory from its plain one {away:.3e}")
    assert away > 0.1                                                         # a missing perturbation would be this far out
    assert upd < 1e-3, upd
    assert upd <= max(8 * base, 3e-4), (upd, base)


def test_two_identical_runs_give_identical_bits():
    for case in sam_ref.CASES:
        runs = []
        for _ in range(2):
            tr = make_trainer(cfg_of(case))
            run_steps(tr, 0, 2)
            runs.append((bits(tr.model.flat_param), bits(tr.sam_loss_perturbed), bits(tr.opt.exp_avg_sq)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), case


def test_ema_follows_the_cpu_recursion_under_sam():
    ecfg = EMAConfig(decay=0.999)
    tr = make_trainer(cfg_of("asam"), ema=ecfg)
    e = tr.opt.ema.detach().cpu().clone()
    assert torch.equal(e, tr.model.flat_param.cpu())
    for k in range(1, 4):
        run_steps(tr, k - 1, k)
        p = tr.model.flat_param.detach().cpu().numpy()
        e = torch.from_numpy(e.numpy() + (p - e.numpy()) * f32(1.0 - ema_decay_at(k, ecfg)))
    assert torch.equal(tr.opt.ema.cpu(), e) and tr.opt.ema_step == 3 and not torch.equal(e, tr.model.flat_param.cpu())
    twin = make_trainer(cfg_of("asam"))
    run_steps(twin, 0, 3)
    assert torch.equal(bits(twin.model.flat_param), bits(tr.model.flat_param))   # EMA does not disturb SAM
    with tr.ema_weights():
        assert torch.equal(tr.model.flat_param.cpu(), e)


def test_the_loss_split_is_the_first_passes():
    mk = lambda: LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, poison_weight=2.0, track_split=True)
    tr, plain = make_trainer(cfg_of("sam"), lf=mk()), make_trainer(None, lf=mk())
    b, t, eps = batch_of(0, flags=True)
    la, lb = tr.train_step(b, t, noise=eps), plain.train_step(b, t, noise=eps)
    torch.cuda.synchronize()
    assert float(la) == float(lb) and float(tr.sam_loss_perturbed) > float(la)
    assert torch.equal(bits(tr.loss_fn.last_split), bits(plain.loss_fn.last_split))
    assert torch.equal(bits(tr.loss_fn.last_sample_loss), bits(plain.loss_fn.last_sample_loss))
    assert tr.loss_fn.last_split.cpu().tolist()[1::2] == [2.0, 2.0]


@pytest.mark.parametrize("family", ["ve", "ldm"])
def test_the_other_families_run_and_restore_bit_exactly(family):
    for case in sam_ref.CASES:
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
        tr = Trainer(net, lf, lr=0.0, total_steps=20, warmup_steps=0, sam=cfg_of(case))
        before = bits(net.flat_param)
        loss = tr.train_step({"target": x0.cuda(), "pixel_values": Rr.cuda()}, t.cuda(), noise=eps.cuda())
        torch.cuda.synchronize()
        assert torch.equal(bits(net.flat_param), before), (family, case)
        l1, l2 = float(loss), float(tr.sam_loss_perturbed)
        assert np.isfinite(l1) and np.isfinite(l2) and l1 != l2 and int(tr.opt.skipped) == 0, (family, case, l1, l2)
        assert float(tr.opt.exp_avg.abs().sum()) > 0


def clone_state(sd):
    return {k: clone_state(v) if isinstance(v, dict) else (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in sd.items()}


def test_resume_and_states_of_either_kind():
    cfg = cfg_of("neuron")
    tr = make_trainer(cfg)
    run_steps(tr, 0, 2)
    st, p2 = clone_state(tr.state_dict()), tr.model.flat_param.detach().clone()
    assert st["sam"] == {"rho": 0.5, "mode": "neuron", "eta": 0.01, "layers": "conv"}
    run_steps(tr, 2, 4)
    again = make_trainer(cfg, seed=99)                                         # other weights: everything comes from the checkpoint
    with torch.no_grad():
        again.model.flat_param.copy_(p2)
    again.load_state_dict(st)
    run_steps(again, 2, 4)
    assert torch.equal(bits(again.model.flat_param), bits(tr.model.flat_param)) and again.opt.step_count == 4
    # SAM keeps no state between steps: a SAM state loads into a plain trainer and a plain state into a SAM trainer
    plain = make_trainer(None)
    plain.load_state_dict(st)
    assert plain.opt.step_count == 2 and torch.equal(bits(plain.opt.exp_avg), bits(st["optimizer"]["exp_avg"]))
    run_steps(plain, 2, 3)
    pst = clone_state(plain.state_dict())
    assert "sam" not in pst
    into = make_trainer(cfg_of("asam"))
    into.load_state_dict(pst)
    assert into.opt.step_count == 3 and into.sam.mode == "asam"
    run_steps(into, 3, 4)


# ------------------------------------------------------------------------------------------------------------------- 4. the drivers
def test_cli_sam_train_resume_and_the_removal_driver(tmp_path):
    base_net = UNet2DModel(**SMALL)
    base_net.reset_parameters(seed=1)
    root = tmp_path / "ckpts"
    DDPMPipeline(base_net, S.DDPMScheduler()).save_pretrained(str(root / "SMALL-BASE"))
    env = dict(os.environ, PYTHONPATH=ROOT, VILLAN_CKPT_ROOT=str(root), VILLAN_CFG_OVERRIDES=json.dumps({"eval_sample_n": 2, "lr_warmup_steps": 0}))
    code = ("import sys; sys.argv=[%r]+%r; import villandiffusion_amd.dataset as D;"
            "D.synthetic_images=(lambda f: (lambda n=60000, **k: f(n=256, **k)))(D.synthetic_images);"
            "import %s as V; V.main()")

    def drive(driver, argv):
        out = subprocess.run([sys.executable, "-c", code % (driver + ".py", argv, driver)], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    common = ["--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--poison_rate", "0.1", "--trigger", "BOX_14", "--target", "HAT",
              "--ckpt", "SMALL-BASE", "--fclip", "o", "-o", "--sched", "DDIM-SCHED", "--infer_steps", "2", "--save_image_epochs", "1",
              "--save_model_epochs", "1"]
    res = str(tmp_path / "res")
    out = drive("VillanDiffusion", ["--mode", "train", "--result", res, "--sam_rho", "0.05"] + common)
    run = os.path.join(res, os.listdir(res)[0])
    args = json.load(open(os.path.join(run, "args.json")))
    assert args["sam_rho"] == 0.05 and not {"sam_mode", "sam_eta", "sam_layers"} & set(args)
    assert json.load(open(os.path.join(run, "config.json")))["sam_rho"] == 0.05
    st = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    assert st["optimizer"]["step"] == 2 and st["sam"] == {"rho": 0.05, "mode": "sam", "eta": 0.01, "layers": "conv"}
    assert "epoch 0 step 2 loss" in out and os.path.exists(os.path.join(run, "samples", "final.png"))
    # the same run without the flag ends elsewhere: the flag reached the trainer
    plain_res = str(tmp_path / "plain")
    drive("VillanDiffusion", ["--mode", "train", "--result", plain_res] + common)
    plain = os.path.join(plain_res, os.listdir(plain_res)[0])
    pst = torch.load(os.path.join(plain, "ckpt", "trainer.pt"), map_location="cpu")
    assert "sam" not in pst and pst["optimizer"]["step"] == 2
    assert not torch.equal(pst["optimizer"]["exp_avg"], st["optimizer"]["exp_avg"])
    # resume reads the flags from args.json
    drive("VillanDiffusion", ["--mode", "resume", "--ckpt", run])
    st2 = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    assert st2["sam"] == st["sam"] and st2["optimizer"]["step"] > st["optimizer"]["step"]
    # the removal fine-tune with the neuron-adaptive mode
    rm_res = str(tmp_path / "rm")
    drive("rm_backdoor_VillanDiffusion", ["--mode", "train", "--result", rm_res, "--sam_rho", "0.5", "--sam_mode", "neuron", "--sam_layers", "all"] + common)
    rm = os.path.join(rm_res, os.listdir(rm_res)[0])
    rst = torch.load(os.path.join(rm, "ckpt", "trainer.pt"), map_location="cpu")
    assert rst["sam"] == {"rho": 0.5, "mode": "neuron", "eta": 0.01, "layers": "all"} and rst["optimizer"]["step"] == 2
    a = json.load(open(os.path.join(rm, "args.json")))
    assert (a["sam_rho"], a["sam_mode"], a["sam_layers"]) == (0.5, "neuron", "all") and "sam_eta" not in a
