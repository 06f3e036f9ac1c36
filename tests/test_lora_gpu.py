"""LoRA fine-tuning (villandiffusion_amd.lora) on the GPU: the two kernels on synthetic tables (exact on integers, inside derived bounds on
reals), the adapter gradient through the small UNet and a small NCSN++ against autograd on the oracle, six optimiser steps of
`Trainer(lora=...)` against torch Adam on (A, B), "the model is left alone", the training state, and the driver in child processes."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_families_ref as fam  # noqa: E402
import lora_ref  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import lora, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.lora import LoRAAdapter, LoRAConfig  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.pipelines import DDPMPipeline  # noqa: E402
from villandiffusion_amd.trainer import EMAConfig, FusedAdam, Trainer  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_anp_gpu.py's
PP1 = dict(fam.SMALL_PP, layers_per_block=1)
NAN = float("nan")


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. the kernels on synthetic tables
# The issue's shapes, then the edges of the kernels' own partitions: 4 rows a workgroup (3 / 4 / 5 rows), 256 columns a tile and 64 items a
# wave pass (255 / 256 / 257 floats a row), two tiles and a one-float third (513), 9 rows = two full row workgroups and one row.
SHAPES = ((3, 27), (1, 1), (7, 129), (32, 288), (5, 4608), (5, 16128), (897, 20), (4, 255), (5, 256), (3, 257), (9, 513))
RANKS = (1, 4, 7, 32)


def synthetic_table(r, s):
    """One job per shape.  Weight offsets alternate between multiples of four floats and 1 / 2 / 3 past one, so rows start aligned and unaligned
    whatever the row length; five to eight unused floats lie between the weights and 64 after the last.  The pieces of the adapter buffer start
    at multiples of four floats with 0, 4 or 8 unused floats between them beyond the padding, and 8 after the last."""
    jobs, slices, cursor, acur, rb, cb = [], {}, 3, 0, 0, 0
    for k, (M, L) in enumerate(SHAPES):
        off = (cursor + 3) // 4 * 4 + (k % 4 if k % 2 else 0)
        cursor = off + M * L + 5
        aoff = acur + 4 * (k % 3)
        boff = aoff + (r * L + 3) // 4 * 4 + 4 * ((k + 1) % 2)
        acur = boff + (M * r + 3) // 4 * 4
        jobs.append((off, M, L, aoff, boff, rb, cb))
        slices[f"job{k}"] = (slice(aoff, aoff + r * L), slice(boff, boff + M * r))
        rb += (M + 3) // 4
        cb += (L + 255) // 256
    tab = lora.AdapterTable(jobs, slices, acur + 8, r, s)
    assert tab.extent == cursor - 5 and any(j[0] % 4 for j in jobs) and any(j[0] % 4 == 0 for j in jobs)
    assert (tab.row_blocks, tab.col_blocks) == (rb, cb)
    return tab, cursor + 64


def on_device(host, shift):
    """A device copy of `host` whose base pointer is `shift` floats past 16-byte alignment."""
    buf = torch.empty(host.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + host.numel()]
    v.copy_(host)
    return v


def pieces(tab, k):
    off, M, L, aoff, boff, _, _ = tab.jobs[k]
    return (slice(off, off + M * L), slice(aoff, aoff + tab.r * L), slice(boff, boff + M * tab.r), M, L)


def fill_adapter(tab, draw):
    """[numel] host buffer: draw(n) in every piece, NaN in the padding and the gaps (never read, never written)."""
    ab = torch.full((tab.numel,), NAN)
    for k in range(tab.n_jobs):
        _, a, b, _, _ = pieces(tab, k)
        ab[a] = draw(a.stop - a.start)
        ab[b] = draw(b.stop - b.start)
    return ab


@pytest.mark.parametrize("shifts", [(0, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1)], ids=["aligned", "all+4B", "w+4B", "ab+4B"])
@pytest.mark.parametrize("r", RANKS)
def test_kernels_are_exact_on_small_integers(r, shifts):
    """|values| <= 8, s = 1/2: every product, every partial sum (at most 16128 * 64 < 2^24) and the product with s are exact in f32 in any order,
    so merge, dB and dA equal the integer results, and the NaN sentinel survives outside the jobs and in the padding."""
    s = 0.5
    tab, numel = synthetic_table(r, s)
    gen = g(10 + r)
    ints = lambda n: torch.randint(-8, 9, (n,), generator=gen).float()
    w0, gv, ab = ints(numel), ints(numel), fill_adapter(tab, ints)
    w_d = on_device(torch.full((numel,), NAN), shifts[1])
    ab_d = on_device(ab, shifts[2])
    gab_d = on_device(torch.full((tab.numel,), NAN), shifts[2])
    ops.lora_merge(on_device(w0, shifts[0]), w_d, tab, ab_d)
    ops.lora_grad(on_device(gv, shifts[0]), tab, ab_d, gab_d)
    torch.cuda.synchronize()
    w, gab = w_d.cpu(), gab_d.cpu()
    want_w, want_g = torch.full((numel,), NAN), torch.full((tab.numel,), NAN)
    for k in range(tab.n_jobs):
        ws, a, b, M, L = pieces(tab, k)
        A, B = ab[a].view(r, L).long(), ab[b].view(M, r).long()
        want_w[ws] = (w0[ws].view(M, L) + s * (B @ A).float()).reshape(-1)
        G = gv[ws].view(M, L).long()
        want_g[a] = (s * (B.t() @ G).float()).reshape(-1)
        want_g[b] = (s * (G @ A.t()).float()).reshape(-1)
    assert torch.equal(bits(w), bits(want_w))                     # the sentinel between the jobs and behind them included
    assert torch.equal(bits(gab), bits(want_g))                   # ... and in the padding and the gaps of the gradient buffer
    assert int(torch.isnan(want_w).sum()) == numel - tab.weight_floats and int(torch.isnan(want_g).sum()) == tab.numel - tab.adapter_floats
    assert torch.equal(bits(ab_d), bits(ab))


@pytest.mark.parametrize("r", RANKS)
def test_kernels_stay_inside_the_derived_bounds_accumulate_and_repeat(r):
    """Random reals against the float64 closed forms, element by element: merge within 2 (r + 2) u (|w0| + |s| sum |B||A|), the gradients within
    2 (n + 2) u |s| sum |terms| (n addends; any order).  accumulate adds in f32 to what is there; a second run gives the same bits."""
    s = 1.7
    tab, numel = synthetic_table(r, s)
    gen = g(20 + r)
    w0, gv = torch.randn(numel, generator=gen), torch.randn(numel, generator=gen)
    ab = fill_adapter(tab, lambda n: torch.randn(n, generator=gen))
    w0_d, g_d, ab_d = on_device(w0, 0), on_device(gv, 0), on_device(ab, 0)
    w_d = on_device(torch.full((numel,), NAN), 0)
    gab_d = on_device(torch.full((tab.numel,), NAN), 0)
    ops.lora_merge(w0_d, w_d, tab, ab_d)
    ops.lora_grad(g_d, tab, ab_d, gab_d)
    torch.cuda.synchronize()
    w, gab = w_d.cpu(), gab_d.cpu()
    worst = {"merge": 0.0, "dA": 0.0, "dB": 0.0}
    for k in range(tab.n_jobs):
        ws, a, b, M, L = pieces(tab, k)
        A, B, W0, G = ab[a].view(r, L), ab[b].view(M, r), w0[ws].view(M, L), gv[ws].view(M, L)
        err = (w[ws].view(M, L).double() - lora_ref.merged(W0, A, B, s)).abs()
        bound = lora_ref.merge_bound(W0, A, B, s)
        assert bool((err <= bound).all()), (k, "merge")
        worst["merge"] = max(worst["merge"], float((err / bound).max()))
        dA, dB = lora_ref.grads(G, A, B, s)
        bA, bB = lora_ref.grad_bounds(G, A, B, s)
        eA, eB = (gab[a].view(r, L).double() - dA).abs(), (gab[b].view(M, r).double() - dB).abs()
        assert bool((eA <= bA).all()) and bool((eB <= bB).all()), (k, "grad")
        worst["dA"], worst["dB"] = max(worst["dA"], float((eA / bA).max())), max(worst["dB"], float((eB / bB).max()))
    print(f"[lora] r={r}: worst error / bound: merge {worst['merge']:.3f}, dA {worst['dA']:.3f}, dB {worst['dB']:.3f}")
    pad = tab.padding_mask()
    assert bool(torch.isnan(gab[pad]).all()) and not bool(torch.isnan(gab[~pad]).any())
    # accumulate: f32 addition to what is there, the padding still untouched
    c = torch.randn(tab.numel, generator=gen)
    c[pad] = NAN
    acc_d = on_device(c, 0)
    ops.lora_grad(g_d, tab, ab_d, acc_d, accumulate=True)
    again_d = on_device(torch.full((tab.numel,), NAN), 0)
    ops.lora_grad(g_d, tab, ab_d, again_d)
    w2_d = on_device(torch.full((numel,), NAN), 0)
    ops.lora_merge(w0_d, w2_d, tab, ab_d)
    torch.cuda.synchronize()
    assert torch.equal(bits(acc_d.cpu()[~pad]), bits((c + gab)[~pad])) and bool(torch.isnan(acc_d.cpu()[pad]).all())
    assert torch.equal(bits(again_d), bits(gab)) and torch.equal(bits(w2_d), bits(w))          # a repeat: the same bits


def test_rank_outside_1_to_32_is_refused_on_both_sides():
    tab, numel = synthetic_table(4, 1.0)
    with pytest.raises(ValueError, match="rank"):
        lora.AdapterTable(tab.jobs, tab.slices, tab.numel, 33)
    w0, w, ab = torch.zeros(numel, device=DEV), torch.zeros(numel, device=DEV), torch.zeros(tab.numel, device=DEV)
    table = tab.device_table(w.device)
    lib = ops.L.load()
    for r in (0, 33):
        assert lib.vd_lora_merge(w0.data_ptr(), w.data_ptr(), table.data_ptr(), tab.n_jobs, tab.row_blocks, ab.data_ptr(), r, 1.0, None) != 0
        assert "rank" in ops.L.last_error()
        assert lib.vd_lora_grad(w0.data_ptr(), table.data_ptr(), tab.n_jobs, tab.row_blocks + tab.col_blocks, ab.data_ptr(), w.data_ptr(), r, 1.0, 0,
                                None) != 0
    torch.cuda.synchronize()
    assert float(w.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 2. gradients through the network
def _random_adapters(ref, tab, r, seed):
    ad = lora_ref.init_adapters(ref, list(tab.slices), r, seed)
    gen = g(seed + 1)
    return {n: (A, 0.05 * torch.randn(B.shape, generator=gen)) for n, (A, B) in ad.items()}


@pytest.fixture(scope="module")
def through_the_network():
    """Per family: the oracle, the table, random adapters with B != 0, one batch of 4, and -- computed once, shared read-only -- autograd's
    dA, dB and the oracle's weight gradients at the merged weights."""
    cfg = LoRAConfig(r=4, alpha=8.0, target="all")
    out = {}
    torch.manual_seed(0)
    vp = UNet2DModelRef(**SMALL)
    fam.perturb_norms(vp)
    for name, ref, cls, kw, t in (("vp", vp, UNet2DModel, SMALL, torch.tensor([3, 250, 600, 870])),
                                  ("ve", fam.small_ncsnpp(1), NCSNppModel, PP1, torch.tensor([0.05, 1.7, 30.0, 120.0]))):
        size = int(kw["sample_size"])
        make = lambda device=None, cls=cls, kw=kw: cls(**kw, device=device)
        tab = lora.adapter_table(make("cpu"), cfg)
        ad = _random_adapters(ref, tab, cfg.r, 5)
        x = torch.randn(4, 3, size, size, generator=g(2))
        w = torch.randn(4, 3, size, size, generator=g(3))
        gab, gw, y = lora_ref.autograd_grads(ref, ad, cfg.s, x, t, w)
        out[name] = dict(ref=ref, make=make, tab=tab, ad=ad, x=x, t=t, w=w, gab=gab, gw=gw, y=y, cfg=cfg)
    return out


@pytest.mark.parametrize("math_mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("family", ["vp", "ve"])
def test_adapter_gradient_through_the_network(through_the_network, family, math_mode):
    d = through_the_network[family]
    cfg, tab, ad = d["cfg"], d["tab"], d["ad"]
    net = d["make"]()
    net.load_state_dict(d["ref"].state_dict())
    net.conv_math = math_mode
    adapter = LoRAAdapter(net, cfg)
    assert adapter.table.jobs == tab.jobs
    adapter.param.copy_(lora_ref.flat_of(ad, tab.slices, tab.numel))
    adapter.merge_()
    net.zero_grad()
    y = net(d["x"].cuda(), d["t"].cuda())[0]
    (y * d["w"].cuda()).sum().backward()
    adapter.backward_()
    torch.cuda.synchronize()
    e_y = float((y.detach().cpu().double() - d["y"].double()).abs().max() / d["y"].double().abs().max())
    got = lora_ref.adapters_of(adapter.grad.cpu(), tab.slices, tab.shapes, cfg.r)
    worst = (0.0, "")
    for name in tab.slices:
        for k, which in enumerate(("dA", "dB")):
            want = d["gab"][name][k].double()
            e = float((got[name][k].double() - want).abs().max() / want.abs().max())
            if e > worst[0]:
                worst = (e, f"{name} {which}")
    print(f"[parity] LoRA gradient through the {family} network ({math_mode}): forward {e_y:.2e}; worst layer max|diff|/max|ref| {worst[0]:.3e} "
          f"at {worst[1]}")
    assert e_y < 1e-4
    assert worst[0] < 1e-3, worst                            # test_unet_gpu.py's per-parameter gradient gate, both arithmetics
    assert float(adapter.grad[tab.padding_mask().cuda()].abs().sum()) == 0.0
    adapter.unmerge_()
    assert torch.equal(bits(net.flat_param), bits(adapter.base))


@pytest.mark.parametrize("family", ["vp", "ve"])
def test_kernel_alone_on_the_oracles_weight_gradient(through_the_network, family):
    """vd_lora_grad fed the ORACLE's weight gradient: the network's arithmetic is out of the picture and the kernel bounds of test 1 apply."""
    d = through_the_network[family]
    cfg, tab, ad = d["cfg"], d["tab"], d["ad"]
    net = d["make"]("cpu")
    flat_g = torch.zeros(net.flat_numel)
    for name in tab.slices:
        off, n, _ = net._offs[name]
        flat_g[off:off + n] = d["gw"][name].reshape(-1)
    gab = torch.full((tab.numel,), NAN, device=DEV)
    ops.lora_grad(flat_g.to(DEV), tab, lora_ref.flat_of(ad, tab.slices, tab.numel).to(DEV), gab)
    torch.cuda.synchronize()
    got = lora_ref.adapters_of(gab.cpu(), tab.slices, tab.shapes, cfg.r)
    worst = 0.0
    for name, (A, B) in ad.items():
        G = d["gw"][name]
        dA, dB = lora_ref.grads(G, A, B, cfg.s)
        bA, bB = lora_ref.grad_bounds(G, A, B, cfg.s)
        eA, eB = (got[name][0].double() - dA).abs(), (got[name][1].double() - dB).abs()
        assert bool((eA <= bA).all()) and bool((eB <= bB).all()), name
        tiny = 1e-300
        worst = max(worst, float((eA / (bA + tiny)).max()), float((eB / (bB + tiny)).max()))
    print(f"[lora] kernel alone on the {family} oracle's weight gradient: worst error / bound {worst:.3f}")
    assert bool(torch.isnan(gab.cpu()[tab.padding_mask()]).all())


# ------------------------------------------------------------------------------------------------------------ 3. the trajectory
def batch_of(i, B=4):
    """tests/test_ema_gpu.py's batches."""
    gen = g(100 + i)
    x0 = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    R = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    R[::2] = 0
    eps = torch.randn(B, 3, 32, 32, generator=gen)
    t = torch.randint(0, 1000, (B,), generator=gen)
    return x0, R, t, eps


def make_trainer(lora_cfg, seed=3, ema=None, **kw):
    """tests/test_ema_gpu.py's make_trainer, with the lora argument."""
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=seed)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    if lora_cfg is None:
        return Trainer(net, lf, lr=1e-3, total_steps=20, warmup_steps=0, ema=ema, **kw)
    return Trainer(net, lf, lr=1e-3, total_steps=20, warmup_steps=0, ema=ema, lora=lora_cfg, **kw)


def run_steps(tr, first, last):
    for i in range(first, last):
        x0, R, t, eps = batch_of(i)
        tr.train_step({"target": x0.cuda(), "pixel_values": R.cuda()}, t.cuda(), noise=eps.cuda())
    torch.cuda.synchronize()


CFG = LoRAConfig(r=4, alpha=8.0, target="all", seed=7)


def _rel_l2(got, want, start):
    return float(((got.double() - want.double()) ** 2).sum() / ((want.double() - start.double()) ** 2).sum()) ** 0.5


@pytest.mark.parametrize("start", ["default", "random_B"])
def test_six_optimiser_steps_follow_adam_on_the_adapters_of_the_oracle(start):
    tr = make_trainer(CFG)
    net, ad, tab = tr.model, tr.adapter, tr.adapter.table
    assert tr.opt.ema is None and ad.table.skipped == ["conv_out.weight"]
    if start == "random_B":
        with torch.no_grad():
            for _, b in tab.slices.values():
                ad.param[b] = (0.05 * torch.randn(b.stop - b.start, generator=g(b.start))).cuda()
        ad.merge_()
    base, p0, w_start = ad.base.cpu().clone(), ad.param.cpu().clone(), net.flat_param.cpu().clone()
    ref = UNet2DModelRef(**SMALL)
    ref.load_state_dict({k: base[off:off + n].view(shape).clone() for k, (off, n, shape) in net._offs.items()})
    oracle = lora_ref.AdamOnAdapters(ref, lora_ref.adapters_of(p0, tab.slices, tab.shapes, CFG.r), CFG.s, lr=1e-3, total_steps=20)
    inside = torch.zeros(net.flat_numel, dtype=torch.bool)
    for off, M, L, *_ in tab.jobs:
        inside[off:off + M * L] = True
    pad = tab.padding_mask()
    if start == "default":
        assert torch.equal(net.flat_param.cpu(), base)                          # B = 0: the adapted network starts as the base
    for i in range(6):
        x0, R, t, eps = batch_of(i)
        loss = tr.train_step({"target": x0.cuda(), "pixel_values": R.cuda()}, t.cuda(), noise=eps.cuda())
        l_ref = oracle.step(x0, R, t, eps)
        assert abs(float(loss) - l_ref) <= 1e-4 * abs(l_ref), (i, float(loss), l_ref)
        assert abs(tr.lr - oracle.opt.param_groups[0]["lr"]) < 1e-15
        now = net.flat_param.cpu()
        assert torch.equal(bits(now[~inside]), bits(base[~inside])), i          # every frozen float keeps the base's bits
        assert not torch.equal(now[inside], base[inside])
        assert float(ad.param.cpu()[pad].abs().sum()) == 0.0 and int(tr.opt.skipped) == 0, i
    assert tr.opt.step_count == tr.sched_step == 6
    want_p = lora_ref.flat_of(oracle.adapters, tab.slices, tab.numel)
    upd_ad = _rel_l2(ad.param.cpu(), want_p, p0)
    msd = oracle.merged_state()
    want_w = base.clone()
    for name in tab.slices:
        off, n, _ = net._offs[name]
        want_w[off:off + n] = msd[name].reshape(-1)
    upd_w = _rel_l2(net.flat_param.cpu(), want_w, w_start)                     # relative to the update of the merged weights over the six steps
    print(f"[parity] 6 LoRA optimiser steps from {start}: update L2 error, adapter {upd_ad:.3e}, merged weights {upd_w:.3e}")
    # measured on MI355X: default 1.27e-4 (adapter) / 1.05e-4 (merged weights); random_B 7.84e-4 / 7.21e-4
    assert upd_ad <= 1e-3, upd_ad
    assert upd_w <= 1e-3, upd_w


# ------------------------------------------------------------------------------------------------------------ 4. leaves the model alone
def test_zero_B_is_the_base_network_and_unmerge_restores_it():
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=3)
    x, t = torch.randn(2, 3, 32, 32, generator=g(4)).cuda(), torch.tensor([10.0, 900.0], device=DEV)
    before = bits(net.flat_param)
    with torch.no_grad():
        y0 = net(x, t, return_dict=False)[0].clone()
        ad = LoRAAdapter(net, LoRAConfig(r=4, target="all"))
        ad.merge_()
        assert torch.equal(net.flat_param, ad.base)                             # w0 + s * 0
        assert torch.equal(net(x, t, return_dict=False)[0], y0)
        ad.param.copy_(torch.where(ad.table.padding_mask(), torch.zeros(()), 0.05 * torch.randn(ad.table.numel, generator=g(5))).cuda())
        with ad:                                                                # merged inside, restored on exit
            assert not torch.equal(net.flat_param, ad.base)
            y1 = net(x, t, return_dict=False)[0].clone()
            assert not torch.equal(y1, y0)
        assert torch.equal(bits(net.flat_param), before) and torch.equal(net(x, t, return_dict=False)[0], y0)
        with pytest.raises(ZeroDivisionError):
            with ad:
                1 / 0
        assert torch.equal(bits(net.flat_param), before)
        ad.merge_()
        ad.unmerge_()
        assert torch.equal(bits(net.flat_param), before) and torch.equal(net(x, t, return_dict=False)[0], y0)


def test_a_trainer_without_lora_takes_the_path_it_always_took():
    """Trainer(lora=None) against the step written out by hand from the pieces that existed before LoRA (loss, backward, FusedAdam.step with
    the schedule's rate): the same bits after three steps; and a trainer built without the argument at all is the same object graph."""
    twin = make_trainer(None)
    assert twin.adapter is None and type(twin.opt) is FusedAdam
    run_steps(twin, 0, 3)
    net = UNet2DModel(**SMALL)
    net.reset_parameters(seed=3)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    opt = FusedAdam(net, 1e-3, max_grad_norm=1.0)
    lam = S.get_cosine_schedule_with_warmup_lambda(0, 20)
    net.zero_grad()
    lf.grad_scale = 1.0
    for i in range(3):
        x0, R, t, eps = batch_of(i)
        loss = lf.p_loss_by_keys({"target": x0.cuda(), "pixel_values": R.cuda()}, net, target_latent_key="target", poison_latent_key="pixel_values",
                                 timesteps=t.cuda(), noise=eps.cuda())
        loss.backward()
        opt.step(lr=1e-3 * lam(i), grad_inv_scale=1.0, need_norm=False)
        net.zero_grad()
    torch.cuda.synchronize()
    assert torch.equal(bits(twin.model.flat_param), bits(net.flat_param))
    assert "lora" not in twin.state_dict()


# ------------------------------------------------------------------------------------------------------------ 5. state
def clone_state(sd):
    return {k: clone_state(v) if isinstance(v, dict) else (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in sd.items()}


def test_resume_is_bit_exact_and_the_two_kinds_of_state_do_not_mix(tmp_path):
    tr = make_trainer(CFG)
    base = tr.adapter.base.clone()
    run_steps(tr, 0, 3)
    st = clone_state(tr.state_dict())
    assert set(st["lora"]) == {"param", "base", "config"} and st["lora"]["config"]["r"] == 4 and "ema" not in st["optimizer"]
    run_steps(tr, 3, 6)
    other = make_trainer(CFG, seed=99)                                           # other weights, other base: everything comes from the state
    assert not torch.equal(other.model.flat_param, tr.model.flat_param)
    other.load_state_dict(st)
    assert other.opt.step_count == 3 and torch.equal(bits(other.adapter.base), bits(base))
    run_steps(other, 3, 6)
    assert torch.equal(bits(other.adapter.param), bits(tr.adapter.param)) and torch.equal(bits(other.model.flat_param), bits(tr.model.flat_param))
    plain = make_trainer(None)
    run_steps(plain, 0, 1)
    sd_plain = clone_state(plain.state_dict())
    before = bits(plain.model.flat_param)
    with pytest.raises(ValueError, match="LoRA"):
        plain.load_state_dict(st)
    assert torch.equal(bits(plain.model.flat_param), before)
    with pytest.raises(ValueError, match="LoRA"):
        other.load_state_dict(sd_plain)
    with pytest.raises(ValueError, match="adapter is"):
        make_trainer(LoRAConfig(r=2, target="all")).load_state_dict(st)
    with pytest.raises(ValueError, match="ema"):
        make_trainer(CFG, ema=EMAConfig())
    # save_pretrained(lora=...): unet/ holds the merged weights; the adapter on a fresh copy of the base reproduces them bit for bit
    out = str(tmp_path / "ckpt")
    DDPMPipeline(tr.model, S.DDPMScheduler()).save_pretrained(out, lora=tr.adapter)
    assert sorted(os.listdir(os.path.join(out, "unet_lora"))) == ["adapter_config.json", "adapter_model.safetensors"]
    loaded = DDPMPipeline.from_pretrained(out).unet
    assert torch.equal(bits(loaded.flat_param), bits(tr.model.flat_param))
    fresh = UNet2DModel(**SMALL)
    with torch.no_grad():
        fresh.flat_param.copy_(base)
    ad = LoRAAdapter.load(fresh, os.path.join(out, "unet_lora"))
    assert ad.cfg.r == 4 and ad.cfg.s == 2.0 and ad.cfg.target == "all"
    ad.merge_()
    torch.cuda.synchronize()
    assert torch.equal(bits(fresh.flat_param), bits(tr.model.flat_param)) and torch.equal(bits(ad.param), bits(tr.adapter.param))


# ------------------------------------------------------------------------------------------------------------ 6. the driver
def test_cli_lora_train_resume_sample_and_merge(tmp_path):
    from safetensors.torch import load_file
    base_net = UNet2DModel(**SMALL)
    base_net.reset_parameters(seed=1)
    root = tmp_path / "ckpts"
    DDPMPipeline(base_net, S.DDPMScheduler()).save_pretrained(str(root / "SMALL-BASE"))
    env = dict(os.environ, PYTHONPATH=ROOT, VILLAN_CKPT_ROOT=str(root), VILLAN_CFG_OVERRIDES=json.dumps({"batch_32": 8, "eval_sample_n": 2, "lr_warmup_steps": 0}))
    code = ("import sys; sys.argv=['VillanDiffusion.py']+%r; import villandiffusion_amd.dataset as D;"
            "D.synthetic_images=(lambda f: (lambda n=60000, **k: f(n=32, **k)))(D.synthetic_images);"
            "import VillanDiffusion as V; V.main()")

    def drive(argv):
        out = subprocess.run([sys.executable, "-c", code % (argv,)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]

    res = str(tmp_path / "res")
    drive(["--mode", "train", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "8", "--epoch", "1", "--poison_rate", "0.1", "--trigger", "BOX_14",
           "--target", "HAT", "--ckpt", "SMALL-BASE", "--fclip", "o", "-o", "--result", res, "--sched", "DDIM-SCHED", "--infer_steps", "2",
           "--save_image_epochs", "1", "--save_model_epochs", "1", "--lora_r", "4", "--lora_target", "attn"])
    run = os.path.join(res, os.listdir(res)[0])
    for f in ("unet/diffusion_pytorch_model.safetensors", "unet_lora/adapter_config.json", "unet_lora/adapter_model.safetensors", "samples/final.png"):
        assert os.path.exists(os.path.join(run, f)), f
    args = json.load(open(os.path.join(run, "args.json")))
    assert args["lora_r"] == 4 and "lora_alpha" not in args and "ema_decay" not in args
    assert args.get("lora_target", "attn") == "attn"                             # (at its default a flag stays out of the side files)
    assert json.load(open(os.path.join(run, "config.json")))["lora_r"] == 4
    st = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    steps = st["optimizer"]["step"]
    assert steps >= 1 and st["lora"]["config"] == {"r": 4, "alpha": None, "target": "attn", "seed": 0}
    assert torch.equal(st["lora"]["base"], base_net.flat_param.cpu())
    first = load_file(os.path.join(run, "unet", "diffusion_pytorch_model.safetensors"))
    drive(["--mode", "resume", "--ckpt", run])
    st2 = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    assert st2["optimizer"]["step"] > steps and torch.equal(st2["lora"]["base"], st["lora"]["base"])
    assert not torch.equal(st2["lora"]["param"], st["lora"]["param"])
    os.remove(os.path.join(run, "samples", "final.png"))
    drive(["--mode", "sampling", "--ckpt", run, "--sched", "DDIM-SCHED", "--infer_steps", "2"])
    assert os.path.exists(os.path.join(run, "samples", "final.png")) and json.load(open(os.path.join(run, "sampling.json")))["lora_r"] == 4
    # base + adapter = the run's own unet/, bit for bit; only the attention projections moved
    merged = str(tmp_path / "merged")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lora_adapter.py"), "merge", "--base", str(root / "SMALL-BASE"), "--adapter",
                          os.path.join(run, "unet_lora"), "--out", merged], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    a = load_file(os.path.join(merged, "unet", "diffusion_pytorch_model.safetensors"))
    b = load_file(os.path.join(run, "unet", "diffusion_pytorch_model.safetensors"))
    assert set(a) == set(b) and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
    base_sd = {k: v.cpu() for k, v in base_net.state_dict().items()}
    moved = {k for k in b if not torch.equal(b[k], base_sd[k])}
    assert moved and all(".attentions." in k and k.endswith(".weight") for k in moved) and len(moved) == 16
    assert any(not torch.equal(first[k], b[k]) for k in moved)                   # the resumed steps went on training the adapter
    info = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lora_adapter.py"), "info", os.path.join(run, "unet_lora"), "--base",
                           str(root / "SMALL-BASE")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert info.returncode == 0, info.stderr[-2000:]
    rec = json.loads(info.stdout)
    assert rec["r"] == 4 and rec["n_layers"] == 16 and all(0 < v["update_over_base_fro"] < 1 for v in rec["layers"].values())
