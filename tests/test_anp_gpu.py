"""Adversarial Neuron Pruning (villandiffusion_amd.anp) on the GPU: the three neuron kernels on synthetic tables against their torch restatements,
anp_objective against the CPU oracle (tests/anp_ref.py), the ascent step's signs, the mask trajectory, "the model is left alone", and
tools/anp_defense.py in a child process."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_ref  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import anp, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_mitigation_gpu.py


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. the kernels on synthetic tables
SHAPES = ((3, 27), (1, 1), (7, 129), (32, 288), (5, 4608))


def synthetic_table():
    """Ten jobs: every (rows, row length) with and without a bias.  Weight offsets alternate between multiples of four floats and 1 / 2 / 3 past
    one, so rows start aligned and unaligned whatever the row length; five to eight unused floats lie between the pieces and 64 after the last."""
    jobs, cursor, neuron, block = [], 3, 0, 0
    for k, (rows, ln) in enumerate(s for s in SHAPES for _ in range(2)):
        off = (cursor + 3) // 4 * 4 + (k % 4 if k % 2 else 0)
        cursor = off + rows * ln + 5
        boff = -1
        if k % 2 == 0:
            boff, cursor = cursor, cursor + rows + 5
        jobs.append((off, rows, ln, boff, neuron, block))
        neuron += rows
        block += (rows + 3) // 4
    tab = anp.NeuronTable(jobs, neuron, {f"job{k}": slice(j[4], j[4] + j[1]) for k, j in enumerate(jobs)})
    assert tab.extent == cursor - 5 and any(j[0] % 4 for j in jobs) and any(j[0] % 4 == 0 for j in jobs)
    return tab, cursor + 64


def on_device(host, shift):
    """A device copy of `host` whose base pointer is `shift` floats past 16-byte alignment."""
    buf = torch.empty(host.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + host.numel()]
    v.copy_(host)
    return v


def scale_ref(w0, w_init, tab, mask, delta, xi):
    w = w_init.clone()
    for off, rows, ln, boff, n0, _ in tab.jobs:
        s = mask[n0:n0 + rows] if delta is None else mask[n0:n0 + rows] + delta[n0:n0 + rows]
        w[off:off + rows * ln] = (s[:, None] * w0[off:off + rows * ln].view(rows, ln)).reshape(-1)
        if boff >= 0:
            b = w0[boff:boff + rows]
            w[boff:boff + rows] = b if xi is None else (1.0 + xi[n0:n0 + rows]) * b
    return w


@pytest.mark.parametrize("shifts", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "both+4B", "w+4B"])
def test_neuron_scale_equals_its_torch_restatement(shifts):
    tab, numel = synthetic_table()
    n = tab.n_neurons
    gen = g(1)
    w0 = torch.randn(numel, generator=gen)
    mask, delta, xi = torch.rand(n, generator=gen), (torch.rand(n, generator=gen) * 2 - 1) * 0.4, (torch.rand(n, generator=gen) * 2 - 1) * 0.4
    sentinel = torch.full((numel,), float("nan"))
    w0_d = on_device(w0, shifts[0])
    for d, x in ((delta, xi), (None, xi), (delta, None), (None, None)):
        w_d = on_device(sentinel, shifts[1])
        assert w_d.data_ptr() % 16 == 4 * shifts[1]
        up = lambda v: None if v is None else v.to(DEV)
        ops.neuron_scale(w0_d, w_d, tab, mask.to(DEV), up(d), up(x))
        want = scale_ref(w0, sentinel, tab, mask, d, x)
        assert torch.equal(bits(w_d), bits(want))                 # bit for bit, the NaN sentinel in the gaps and the tail included
        assert int(torch.isnan(want).sum()) == numel - tab.weight_floats - tab.n_bias
    assert torch.equal(bits(w0_d), bits(w0))


def _grad(tab, gv, w0, shift, gmask=None, gxi=None, **kw):
    n = tab.n_neurons
    gm = torch.full((n,), float("nan"), device=DEV) if gmask is None else gmask.to(DEV)
    gx = torch.full((n,), float("nan"), device=DEV) if gxi is None else gxi.to(DEV)
    ops.neuron_grad(on_device(gv, shift), on_device(w0, shift), tab, gm, gx, **kw)
    return gm.cpu(), gx.cpu()


def test_neuron_grad_indexing_is_exact_on_integers():
    tab, numel = synthetic_table()
    gen = g(2)
    gv = torch.randint(-8, 9, (numel,), generator=gen).float()
    w0 = torch.randint(-8, 9, (numel,), generator=gen).float()             # |row sum| <= 4608 * 64 < 2^24: exact in f32 in any order
    want_m = torch.zeros(tab.n_neurons, dtype=torch.int64)
    want_x = torch.zeros(tab.n_neurons, dtype=torch.int64)
    has_bias = torch.zeros(tab.n_neurons, dtype=torch.bool)
    for off, rows, ln, boff, n0, _ in tab.jobs:
        want_m[n0:n0 + rows] = (gv[off:off + rows * ln].long() * w0[off:off + rows * ln].long()).view(rows, ln).sum(1)
        if boff >= 0:
            want_x[n0:n0 + rows] = gv[boff:boff + rows].long() * w0[boff:boff + rows].long()
            has_bias[n0:n0 + rows] = True
    for shift in (0, 1):
        gm, gx = _grad(tab, gv, w0, shift)
        assert torch.equal(gm, want_m.float())
        assert torch.equal(gx[has_bias], want_x[has_bias].float()) and bool(torch.isnan(gx[~has_bias]).all())      # bias-less jobs: untouched
    assert 0 < int(has_bias.sum()) < tab.n_neurons


def test_neuron_grad_accuracy_scale_accumulate_and_repeat():
    tab, numel = synthetic_table()
    gen = g(3)
    gv, w0 = torch.randn(numel, generator=gen), torch.randn(numel, generator=gen)
    gm, gx = _grad(tab, gv, w0, 0)
    worst = 0.0
    for off, rows, ln, boff, n0, _ in tab.jobs:
        a, b = gv[off:off + rows * ln].double().view(rows, ln), w0[off:off + rows * ln].double().view(rows, ln)
        err = (gm[n0:n0 + rows].double() - (a * b).sum(1)).abs()
        bound = anp_ref.grad_bound(ln, a, b)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"[parity] neuron_grad rows of {ln}: worst error / (min(n, 128) 2^-24 sum|g w0|) = {ratio:.3f}")
        assert bool((err <= bound).all())
        if boff >= 0:
            assert torch.equal(gx[n0:n0 + rows], gv[boff:boff + rows] * w0[boff:boff + rows])
    print(f"[parity] neuron_grad worst ratio {worst:.3f}")
    # fixed order: a second call, and a base pointer off alignment (scalar accesses), give equal bits
    again = _grad(tab, gv, w0, 0)
    odd = _grad(tab, gv, w0, 1)
    for other in (again, odd):
        assert torch.equal(bits(other[0]), bits(gm)) and torch.equal(bits(other[1]), bits(gx))
    # power-of-two scales are exact, and accumulate adds to what is there
    pre_m, pre_x = torch.randn(tab.n_neurons, generator=gen), torch.randn(tab.n_neurons, generator=gen)
    sm, sx = _grad(tab, gv, w0, 0, scale=0.25)
    assert torch.equal(bits(sm), bits(gm * 0.25)) and torch.equal(bits(sx), bits(gx * 0.25))
    am, ax = _grad(tab, gv, w0, 0, gmask=pre_m, gxi=pre_x, scale=-2.0, accumulate=True)
    has = ~torch.isnan(gx)
    assert torch.equal(am, pre_m + gm * -2.0) and torch.equal(ax[has], (pre_x + gx * -2.0)[has]) and torch.equal(ax[~has], pre_x[~has])
    # gxi is optional
    only = torch.full((tab.n_neurons,), float("nan"), device=DEV)
    ops.neuron_grad(on_device(gv, 0), on_device(w0, 0), tab, only, None)
    assert torch.equal(bits(only), bits(gm))


@pytest.mark.parametrize("n", [1, 63, 2912])
def test_neuron_step_equals_its_torch_restatement(n):
    gen = g(n)
    x = torch.rand(n, generator=gen)
    gv = torch.randn(n, generator=gen)
    gv[::3] = 0.0
    gv[1::6] = -0.0
    buf = torch.randn(n, generator=gen)
    # momentum: lr large enough that both clamps of [0, 1] are active
    xd, bd = x.to(DEV), buf.to(DEV)
    ops.neuron_step(xd, gv.to(DEV), bd, lr=0.7, momentum=0.9, lo=0.0, hi=1.0)
    wx, wb = anp_ref.step(x, gv, buf, 0.7, 0.9, 0.0, 1.0, False)
    assert torch.equal(bits(xd), bits(wx)) and torch.equal(bits(bd), bits(wb))
    if n > 1:
        assert float(wx.min()) == 0.0 and float(wx.max()) == 1.0 and 0.0 < float(wx.median()) < 1.0
    # sign, descending and (negative lr) ascending, zeros and -0.0 in the gradient; without the sign the plain gradient
    start = (torch.rand(n, generator=gen) * 2 - 1) * 0.4
    for lr, use_sign in ((0.4, True), (-0.4, True), (-0.25, False)):
        xd = start.to(DEV)
        ops.neuron_step(xd, gv.to(DEV), lr=lr, lo=-0.4, hi=0.4, use_sign=use_sign)
        want, _ = anp_ref.step(start, gv, None, lr, 0.0, -0.4, 0.4, use_sign)
        assert torch.equal(bits(xd), bits(want))
        assert torch.equal(want[gv == 0], start[gv == 0])                       # sign(+-0) = 0: no move
        if n > 1:
            lim = float(torch.tensor(0.4, dtype=torch.float32))
            assert float(want.min()) == -lim and float(want.max()) == lim


# ------------------------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**SMALL)
    tab = anp.neuron_table(UNet2DModel(**SMALL, device="cpu"), "all")
    n = tab.n_neurons
    gen = g(7)
    data = dict(clean=torch.rand(8, 3, 32, 32, generator=gen) * 2 - 1, noise=torch.randn(3, 4, 3, 32, 32, generator=gen),
                timesteps=torch.stack([torch.tensor([10, 300, 600, 950]), torch.randint(0, 1000, (4,), generator=gen),
                                       torch.randint(0, 1000, (4,), generator=gen)]),
                pert=(torch.rand(3, 2, n, generator=gen) * 2 - 1) * 0.4, mask=torch.rand(n, generator=gen) * 0.5 + 0.5)
    cache = {}

    def fresh(math_mode="bf16x3"):
        net = UNet2DModel(**SMALL)
        net.load_state_dict(ref.state_dict())
        net.conv_math = math_mode
        return net

    def oracle(case):
        """The reference of an objective case, computed once and shared."""
        if case not in cache:
            d = data
            args = (d["mask"], d["pert"][0, 0], d["pert"][0, 1]) if case == "random" else (torch.ones(n),)
            cache[case] = anp_ref.objective(ref, tab.slices, n, d["clean"][:4], d["timesteps"][0], d["noise"][0], *args)
        return cache[case]
    return ref, fresh, tab, data, oracle


@pytest.mark.parametrize("case", ["ones", "random"])
@pytest.mark.parametrize("math_mode", ["bf16x3", "f32"])
def test_anp_objective_matches_oracle(small, math_mode, case):
    ref, fresh, tab, d, oracle = small
    n = tab.n_neurons
    want_l, want_m, want_x = oracle(case)
    net = fresh(math_mode)
    before = net.flat_param.clone()
    flags = [p.requires_grad for p in net.parameters()]
    args = (d["mask"], d["pert"][0, 0], d["pert"][0, 1]) if case == "random" else (torch.ones(n),)
    loss, gmask, gxi = anp.anp_objective(net, S.DDPMScheduler(), d["clean"][:4], d["timesteps"][0], d["noise"][0], *args)
    assert torch.equal(net.flat_param, before) and [p.requires_grad for p in net.parameters()] == flags
    e_l = abs(float(loss) - float(want_l)) / abs(float(want_l))
    worst = {"gmask": (0.0, ""), "gxi": (0.0, "")}
    for key, got, want in (("gmask", gmask.cpu(), want_m), ("gxi", gxi.cpu(), want_x)):
        floor = 1e-4 * float(want.abs().max())
        for name, sl in tab.slices.items():
            # relative to the layer's largest entry, floored at 1e-4 of the whole vector's (the gate of test_unet_gpu.py, for its reason: to_k.bias
            # has an analytically ZERO gradient -- softmax is invariant to a per-query shift -- so its xi gradient is pure rounding noise)
            err = float((got[sl].double() - want[sl].double()).abs().max() / (want[sl].double().abs().max() + floor))
            if err > worst[key][0]:
                worst[key] = (err, name)
    print(f"[parity] anp_objective ({math_mode}, {case}): loss {float(loss):.6f} (oracle {float(want_l):.6f}, rel {e_l:.2e}); worst layer "
          f"gmask {worst['gmask'][0]:.2e} at {worst['gmask'][1]}, gxi {worst['gxi'][0]:.2e} at {worst['gxi'][1]}")
    assert e_l <= 1e-5 and worst["gmask"][0] <= 1e-3 and worst["gxi"][0] <= 1e-3


def test_ascent_step_signs_match_the_oracle(small):
    """delta after one step's ascent equals the oracle's wherever the oracle's gradient is not near zero (> 1e-2 of its layer's largest: ten
    times the gradient gate); the excluded share stays under 10 %."""
    ref, fresh, tab, d, _ = small
    n = tab.n_neurons
    kw = dict(steps=1, batch=4, anp_eps=0.4, anp_steps=1, anp_alpha=0.2, lr=0.2, momentum=0.9)
    want = anp_ref.learn(ref, tab.slices, n, d["clean"], timesteps=d["timesteps"], noise=d["noise"], perturbation=d["pert"], **kw)
    res = anp.learn_neuron_mask(fresh(), S.DDPMScheduler(), d["clean"], layers="all", timesteps=d["timesteps"][:1], noise=d["noise"][:1],
                                perturbation=d["pert"][:1], **kw)
    firm = torch.zeros(n, dtype=torch.bool)
    for name, sl in tab.slices.items():
        firm[sl] = want["gd"][sl].abs() > 1e-2 * want["gd"][sl].abs().max()
    share = 1.0 - float(firm.float().mean())
    mismatch = int((res.last_delta[firm] != want["delta"][firm]).sum())
    print(f"[parity] ascent signs: {share:.1%} of {n} neurons excluded (oracle gradient within 1e-2 of zero on its layer's scale); "
          f"{mismatch} mismatches on the rest, {int((res.last_delta != want['delta']).sum())} in all")
    assert share <= 0.10
    assert mismatch == 0
    lim = float(torch.tensor(0.4, dtype=torch.float32))
    assert float(res.last_delta.abs().max()) <= lim and float(res.last_xi.abs().max()) <= lim
    assert len(res.natural) == len(res.robust) == 1 and abs(res.natural[0] - want["natural"][0]) <= 1e-5 * want["natural"][0]


def test_mask_trajectory_follows_the_restated_loop(small):
    """anp_eps = 0, momentum = 0, three steps: per layer |m - m_ref| <= 2 * lr * sum_s 1e-3 * max_j |g_s,j| -- first order from the gradient gate,
    doubled for the feedback of mask differences into later steps; the maxima are the oracle's.  lr = 2: masks near 1 are 2^-24 = 6e-8 apart, and
    at the default 0.2 the bound of the layers with the smallest gradients (5e-8 for these inputs) is below that spacing -- it would test how m
    rounds, not how its gradient was computed.  At lr = 2 the smallest bound is eight spacings and the mask moves by up to 0.19."""
    ref, fresh, tab, d, _ = small
    n = tab.n_neurons
    kw = dict(steps=3, batch=4, anp_eps=0.0, anp_steps=1, anp_alpha=0.2, lr=2.0, momentum=0.0)
    want = anp_ref.learn(ref, tab.slices, n, d["clean"], timesteps=d["timesteps"], noise=d["noise"], **kw)
    res = anp.learn_neuron_mask(fresh(), S.DDPMScheduler(), d["clean"], layers="all", timesteps=d["timesteps"], noise=d["noise"], **kw)
    got = res.flat()
    worst = (0.0, "")
    for name, sl in tab.slices.items():
        assert torch.equal(res.masks[name], got[sl])
        bound = 2 * kw["lr"] * sum(1e-3 * float(gm[sl].abs().max()) for gm in want["gm"])
        ratio = float((got[sl] - want["mask"][sl]).abs().max()) / bound
        if ratio > worst[0]:
            worst = (ratio, name)
    moved = float((want["mask"] - 1.0).abs().max())
    print(f"[parity] mask trajectory: worst |m - m_ref| / bound {worst[0]:.3f} at {worst[1]}; the oracle's mask moved up to {moved:.3e} from 1")
    assert worst[0] <= 1.0 and moved > 0.0
    assert res.robust == [] and len(res.natural) == 3
    assert abs(res.natural[0] - want["natural"][0]) <= 1e-5 * want["natural"][0]          # step 0: the same mask, the loss gate


def test_learn_neuron_mask_invariants_and_determinism(small):
    ref, fresh, tab, d, _ = small
    sched = S.DDPMScheduler()
    kw = dict(steps=3, batch=4, anp_eps=0.4, anp_steps=2, lr=0.2, momentum=0.9, layers="conv", seed=3)
    runs = [anp.learn_neuron_mask(fresh(), sched, d["clean"], **kw) for _ in range(2)]
    a, b = runs
    conv = anp.neuron_table(fresh(), "conv")
    assert list(a.masks) == list(conv.slices) and a.n_neurons == conv.n_neurons and a.settings()["anp_steps"] == 2
    m = a.flat()
    assert 0.0 <= float(m.min()) and float(m.max()) <= 1.0 and float(m.min()) < 1.0
    assert len(a.natural) == len(a.robust) == 3 and all(math.isfinite(v) and v > 0 for v in a.natural + a.robust)
    assert torch.equal(bits(m), bits(b.flat())) and a.natural == b.natural and a.robust == b.robust     # Philox noise, fixed summation orders
    c = anp.learn_neuron_mask(fresh(), sched, d["clean"], **(kw | dict(seed=4)))
    assert c.natural != a.natural
    # a tensor and a callable give the same run
    t1 = anp.learn_neuron_mask(fresh(), sched, d["clean"], timesteps=d["timesteps"], noise=d["noise"], perturbation=d["pert"], **(kw | dict(layers="all")))
    t2 = anp.learn_neuron_mask(fresh(), sched, d["clean"], timesteps=lambda i: d["timesteps"][i], noise=lambda i: d["noise"][i],
                               perturbation=lambda i: d["pert"][i], **(kw | dict(layers="all")))
    assert torch.equal(bits(t1.flat()), bits(t2.flat())) and t1.robust == t2.robust


# ------------------------------------------------------------------------------------------------------------ 3. the model is left alone
def test_learning_a_mask_leaves_the_model_alone(small):
    ref, fresh, tab, d, _ = small
    sched = S.DDPMScheduler()
    net = fresh()
    next(net.parameters()).requires_grad_(False)                               # a mix of frozen and trainable parameters comes back as it was
    flags = [p.requires_grad for p in net.parameters()]
    x, t = d["noise"][0].to(DEV), d["timesteps"][0].to(DEV)
    with torch.no_grad():
        out_before = net(x, t)[0].clone()
    before = net.flat_param.clone()
    kw = dict(steps=3, batch=4, anp_eps=0.4, layers="all")
    res = anp.learn_neuron_mask(net, sched, d["clean"], **kw)
    assert float(res.flat().min()) < 1.0                                       # the loop did run on scaled weights
    assert torch.equal(bits(net.flat_param), bits(before)) and [p.requires_grad for p in net.parameters()] == flags and not flags[0]
    with torch.no_grad():
        assert torch.equal(bits(net(x, t)[0]), bits(out_before))               # caches were invalidated and rebuilt from the restored weights

    def boom(i):
        if i == 1:
            raise RuntimeError("boom")                                         # the second step: the weights are scaled at that moment
        return d["noise"][i]
    with pytest.raises(RuntimeError, match="boom"):
        anp.learn_neuron_mask(net, sched, d["clean"], noise=boom, **kw)
    assert torch.equal(bits(net.flat_param), bits(before)) and [p.requires_grad for p in net.parameters()] == flags
    with torch.no_grad():
        assert torch.equal(bits(net(x, t)[0]), bits(out_before))
    assert float(net.flat_grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 4. the tool
def test_tool_anp_defense_in_a_child_process(tmp_path):
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=1)
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "pruned")
    P.DDIMPipeline(net, S.DDIMScheduler()).save_pretrained(ckpt)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "anp_defense.py"), "--ckpt", ckpt, "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "16",
                          "--steps", "2", "--batch", "4", "--fraction", "0.05", "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    pruned = P.DiffusionPipeline.from_pretrained(out).unet
    tab = anp.neuron_table(net, "conv")
    k = int(math.floor(0.05 * tab.n_neurons))
    masks = torch.load(os.path.join(out, "anp_mask.pt"))
    assert list(masks) == list(tab.slices)
    twin = UNet2DModel(**SMALL, device="cpu")
    twin.flat_param.data.copy_(net.flat_param.cpu())
    counts = anp.prune_neurons(twin, masks, fraction=0.05)                     # the selection the masks imply, applied to the input checkpoint
    assert sum(counts.values()) == k
    assert torch.equal(bits(pruned.flat_param), bits(twin.flat_param))         # the pruned rows are zero, every other parameter has its bits
    zero_rows = 0
    for name in tab.slices:
        zero_rows += int((pruned.P[name].reshape(pruned.P[name].shape[0], -1).abs().amax(1) == 0).sum())
    assert zero_rows == k
    info = json.load(open(os.path.join(out, "anp.json")))
    assert len(info["natural"]) == len(info["robust"]) == 2 and all(math.isfinite(v) for v in info["natural"] + info["robust"])
    assert sum(info["pruned"].values()) == info["pruned_total"] == k == line["pruned_total"] and info["pruned"] == counts
    assert (info["steps"], info["batch"], info["layers"], info["fraction"], info["n_clean"], info["n_neurons"]) == (2, 4, "conv", 0.05, 16, tab.n_neurons)
