"""LoRA's adapted backward on the GPU: vd_lora_act_grad alone (exact on small integers, inside derived bounds on reals, its argument checks),
the adapter gradient through the small UNet against autograd on the oracle, what is NOT computed, the optimiser trajectory, gradient
accumulation with and without the graphed micro-step, determinism and state, "full" untouched, and the driver in child processes."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_families_ref as fam  # noqa: E402
import lora_act_ref  # noqa: E402
import lora_ref  # noqa: E402
import test_lora_gpu as base  # noqa: E402  (its SMALL network, batches, trainer factory and helpers)
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import lora, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.lora import LoRAAdapter, LoRAConfig  # noqa: E402
from villandiffusion_amd.pipelines import DDPMPipeline  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"
ROOT = base.ROOT
SMALL = base.SMALL
NAN = float("nan")
bits, g = base.bits, base.g
RANKS = (1, 4, 7, 32)
# (M, L, N, B): one pixel; the 4x4 level; pixel tails and unaligned rows around two tiles; unaligned channel counts; several tiles per workgroup
# and several workgroups per job.  8 max(L, M) B N < 2^24 for each, so sums of products of values in [-2, 2] are exact in any association.
PLAIN = ((5, 3, 1, 1), (32, 32, 16, 3), (64, 64, 64, 2), (64, 64, 63, 2), (64, 64, 65, 2), (33, 129, 256, 3), (32, 64, 1024, 4))
QKV = (32, 32, 100, 2)          # three jobs sharing one x; dy the channel slices of a [B, 96, N] tensor
SHORT = (24, 40, 81, 2)         # x is [:, :L] of a [B, L + 8, N] buffer
LEFT_OUT = (8, 8, 9, 1)         # has slots in the adapter buffer but no job in the table


class Case:
    """The jobs above on the device: operands (`draw(shape)` on the host, shifted one float off 16-byte alignment for every other tensor), the
    adapter buffer (NaN in padding and gaps) and, per job, the host views the reference reads."""

    def __init__(self, r, draw):
        self.r, self.jobs, self.host, self.keep, self.snap = r, [], [], [], []
        cursor = 0
        self.slots = []

        def slot(M, L, k):
            nonlocal cursor
            aoff = cursor + 4 * (k % 2)
            boff = aoff + (r * L + 3) // 4 * 4 + 4 * ((k + 1) % 3)
            cursor = boff + (M * r + 3) // 4 * 4
            self.slots.append((slice(aoff, aoff + r * L), slice(boff, boff + M * r), M, L))
            return aoff, boff

        def dev(t, k):
            buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
            v = buf[k % 2:k % 2 + t.numel()].view(t.shape)
            v.copy_(t)
            self.keep.append(v)
            self.snap.append((v, t))
            return v

        def add(dy_v, x_v, dy_h, x_h, k):
            Bn, M, N = dy_h.shape
            L = x_h.shape[1]
            aoff, boff = slot(M, L, k)
            self.jobs.append((dy_v.data_ptr(), dy_v.stride(0), x_v.data_ptr(), x_v.stride(0), Bn, M, L, N, aoff, boff))
            self.host.append((dy_h, x_h))

        k = 0
        for M, L, N, Bn in PLAIN:
            dy, x = draw((Bn, M, N)), draw((Bn, L, N))
            add(dev(dy, k), dev(x, k + 1), dy, x, k)
            k += 1
        M, L, N, Bn = QKV
        dqkv, x = draw((Bn, 3 * M, N)), draw((Bn, L, N))
        dq_d, x_d = dev(dqkv, k), dev(x, k)
        for i in range(3):
            add(dq_d[:, i * M:(i + 1) * M], x_d, dqkv[:, i * M:(i + 1) * M], x, k)
            k += 1
        M, L, N, Bn = SHORT
        dy, wide = draw((Bn, M, N)), draw((Bn, L + 8, N))
        add(dev(dy, k), dev(wide, k)[:, :L], dy, wide[:, :L], k)
        self.left_out = slot(LEFT_OUT[0], LEFT_OUT[1], k + 1)
        self.numel = cursor + 8
        self.pad = torch.ones(self.numel, dtype=torch.bool)
        self.ab = torch.full((self.numel,), NAN)
        for a, b, _, _ in self.slots:
            self.pad[a] = self.pad[b] = False
            self.ab[a], self.ab[b] = draw((a.stop - a.start,)), draw((b.stop - b.start,))
        self.in_table = self.pad.clone()
        for a, b, _, _ in self.slots[:-1]:
            self.in_table[a] = self.in_table[b] = True
        self.in_table ^= self.pad                                                 # slots of the jobs that ARE in the table
        self.ab_d = self.ab.to(DEV)

    def want(self, s, integers=False):
        """(float64 result, bound) laid out like the adapter buffer; NaN outside the table's jobs.  integers: the sums in int64 (an integer zero is
        +0, where a float64 sum of products can be -0), then the product with s."""
        out, bound = torch.full((self.numel,), NAN, dtype=torch.float64), torch.full((self.numel,), NAN, dtype=torch.float64)
        for (a, b, M, L), (dy, x) in zip(self.slots, self.host):
            A, Bm = self.ab[a].view(self.r, L), self.ab[b].view(M, self.r)
            dA, dB = lora_act_ref.grads(dy, x, A, Bm, s)
            if integers:
                iy, ix, iA, iB = dy.long(), x.long(), A.long(), Bm.long()
                nA = torch.einsum("bqp,blp->ql", torch.einsum("mq,bmp->bqp", iB, iy), ix)
                nB = torch.einsum("bmp,bqp->mq", iy, torch.einsum("ql,blp->bqp", iA, ix))
                assert torch.equal(dA, s * nA.double()) and torch.equal(dB, s * nB.double())      # (equal as numbers: the helper agrees)
                dA, dB = s * nA.double(), s * nB.double()
            bA, bB = lora_act_ref.bounds(dy, x, A, Bm, s)
            out[a], out[b], bound[a], bound[b] = dA.reshape(-1), dB.reshape(-1), bA.reshape(-1), bB.reshape(-1)
        return out, bound

    def run(self, s, workgroups, gab, accumulate=False):
        plan = ops.lora_act_plan(self.jobs, self.r, workgroups=workgroups)
        ws = torch.full((plan.ws_floats + 16,), NAN, device=DEV)
        ops.lora_act_grad(plan, self.ab_d, gab, s, ws, accumulate=accumulate)
        torch.cuda.synchronize()
        return plan

    def inputs_unchanged(self):
        return all(torch.equal(bits(v), bits(t)) for v, t in self.snap) and torch.equal(bits(self.ab_d), bits(self.ab))


@pytest.mark.parametrize("workgroups", [48, 512], ids=["tiles-per-wg", "wg-per-tile"])
@pytest.mark.parametrize("r", RANKS)
def test_act_grad_is_exact_on_small_integers(r, workgroups):
    s = 0.5
    gen = g(30 + r)
    case = Case(r, lambda shape: torch.randint(-2, 3, shape, generator=gen).float())
    assert all(8 * max(M, L) * dy.shape[0] * dy.shape[2] < 2 ** 24 for (_, _, M, L), (dy, _) in zip(case.slots, case.host))
    gab = torch.full((case.numel,), NAN, device=DEV)
    plan = case.run(s, workgroups, gab)
    h = plan.host
    big = h[h[:, 7] == 1024][0]
    tiles = int(big[4]) * 32
    assert (1 < int(big[11]) < tiles) if workgroups == 48 else int(big[11]) == tiles      # several tiles per workgroup / one tile each
    want, _ = case.want(s, integers=True)
    differ = bits(gab) != bits(want.float())
    print(f"[lora_act] r={r}, {workgroups} workgroups: {int(differ.sum())} of {case.numel} floats differ from the integer result"
          + (f"; first at {int(differ.nonzero()[0])}: {float(gab[int(differ.nonzero()[0])])!r} vs {float(want[int(differ.nonzero()[0])])!r}"
             if bool(differ.any()) else ""))
    assert torch.equal(bits(gab), bits(want.float()))              # bit for bit; the NaN of the padding and of the job left out included
    assert int(torch.isnan(want).sum()) == int((~case.in_table).sum()) and bool(torch.isnan(gab.cpu()[case.left_out[0]:case.left_out[0] + 4]).all())
    assert case.inputs_unchanged()


@pytest.mark.parametrize("r", RANKS)
def test_act_grad_stays_inside_the_derived_bounds_accumulates_and_repeats(r):
    s = 1.7
    gen = g(40 + r)
    case = Case(r, lambda shape: torch.randn(shape, generator=gen))
    gab = torch.full((case.numel,), NAN, device=DEV)
    case.run(s, 512, gab)
    want, bound = case.want(s)
    m = case.in_table
    got = gab.cpu()
    err = (got.double()[m] - want[m]).abs()
    worst = float((err / bound[m]).max())
    print(f"[lora_act] r={r}: worst error / bound {worst:.4f}")
    assert bool((err <= bound[m]).all()), worst
    assert bool(torch.isnan(got[~m]).all()) and bool(torch.isfinite(got[m]).all())
    c = torch.randn(case.numel, generator=gen)
    c[~m] = NAN
    acc = c.to(DEV)
    case.run(s, 512, acc, accumulate=True)
    again = torch.full((case.numel,), NAN, device=DEV)
    case.run(s, 512, again)
    assert torch.equal(bits(acc.cpu()[m]), bits((c + got)[m])) and bool(torch.isnan(acc.cpu()[~m]).all())      # accumulate adds in f32
    assert torch.equal(bits(again), bits(gab))                                                               # a repeat: the same bits
    assert case.inputs_unchanged()


def test_act_grad_refuses_bad_arguments_before_any_launch():
    gen = g(50)
    case = Case(4, lambda shape: torch.randn(shape, generator=gen))
    plan = ops.lora_act_plan(case.jobs, 4)
    table = plan.table(torch.device(DEV))
    gab = torch.zeros(case.numel, device=DEV)
    ws = torch.zeros(plan.ws_floats, device=DEV)
    lib = ops.L.load()
    call = lambda r, wsf: lib.vd_lora_act_grad(plan.host.data_ptr(), table.data_ptr(), plan.n_rows, case.ab_d.data_ptr(), gab.data_ptr(), r, 1.0, 0,
                                               ws.data_ptr(), wsf, None)
    for r in (0, 33):
        assert call(r, ws.numel()) != 0 and "rank" in ops.L.last_error()
        assert lib.vd_lora_act_grad_ws_floats(plan.host.data_ptr(), plan.n_rows, r) == -1
    assert call(4, plan.ws_floats - 1) != 0 and "workspace" in ops.L.last_error()
    assert lib.vd_lora_act_grad_ws_floats(plan.host.data_ptr(), plan.n_rows, 4) == plan.ws_floats
    torch.cuda.synchronize()
    assert float(gab.abs().sum()) == 0.0 and float(ws.abs().sum()) == 0.0
    assert call(4, plan.ws_floats) == 0
    torch.cuda.synchronize()
    assert float(gab.abs().sum()) > 0.0


# ------------------------------------------------------------------------------------------------------------ through the network
@functools.lru_cache(maxsize=None)
def oracle_case(target, head_dim):
    """The oracle, the table, random adapters with B != 0, one batch of 4 and autograd's dA, dB: computed once per case, shared read-only."""
    kw = dict(SMALL, attention_head_dim=head_dim) if head_dim else SMALL
    cfg = LoRAConfig(r=4, alpha=8.0, target=target)
    torch.manual_seed(0)
    ref = UNet2DModelRef(**kw)
    fam.perturb_norms(ref)
    tab = lora.adapter_table(UNet2DModel(**kw, device="cpu"), cfg)
    ad = base._random_adapters(ref, tab, cfg.r, 5)
    x, w = torch.randn(4, 3, 32, 32, generator=g(2)), torch.randn(4, 3, 32, 32, generator=g(3))
    t = torch.tensor([3, 250, 600, 870])
    gab, _, y = lora_ref.autograd_grads(ref, ad, cfg.s, x, t, w)
    return dict(kw=kw, cfg=cfg, ref=ref, tab=tab, ad=ad, x=x, w=w, t=t, gab=gab, y=y)


def adapted_network(d, math_mode="f32"):
    net = UNet2DModel(**d["kw"])
    net.load_state_dict(d["ref"].state_dict())
    net.conv_math = math_mode
    adapter = LoRAAdapter(net, d["cfg"], backward="adapted")
    adapter.param.copy_(lora_ref.flat_of(d["ad"], d["tab"].slices, d["tab"].numel))
    adapter.merge_()
    return net, adapter


@pytest.mark.parametrize("target,math_mode,head_dim", [(t, m, None) for t in ("attn", "conv", "all") for m in ("f32", "bf16x3")] + [("attn", "f32", 16)])
def test_adapter_gradient_through_the_network(target, math_mode, head_dim):
    d = oracle_case(target, head_dim)
    tab, cfg = d["tab"], d["cfg"]
    net, adapter = adapted_network(d, math_mode)
    assert adapter.table.jobs == tab.jobs and net.lora_route is adapter.route
    net.zero_grad()
    adapter.zero_grad()
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
    print(f"[parity] adapted LoRA gradient, target {target}, {math_mode}, head_dim {head_dim}: forward {e_y:.2e}; worst layer "
          f"max|diff|/max|ref| {worst[0]:.3e} at {worst[1]}")
    assert e_y < 1e-4
    assert worst[0] < 1e-3, worst
    assert float(adapter.grad[tab.padding_mask().cuda()].abs().sum()) == 0.0
    adapter.detach()


def test_attn_target_never_touches_flat_grad():
    d = oracle_case("attn", None)
    net, adapter = adapted_network(d)
    assert adapter.route.full_table is None
    net.flat_grad.fill_(NAN)
    before = bits(net.flat_grad).clone()
    adapter.zero_grad()
    y = net(d["x"].cuda(), d["t"].cuda())[0]
    (y * d["w"].cuda()).sum().backward()
    adapter.backward_()
    torch.cuda.synchronize()
    assert torch.equal(bits(net.flat_grad), before)
    assert bool(torch.isfinite(adapter.grad).all()) and float(adapter.grad.abs().sum()) > 0.0


def test_conv_target_writes_only_the_adapted_3x3_gradients():
    d = oracle_case("conv", None)
    net, adapter = adapted_network(d)
    slots = torch.zeros(net.flat_numel, dtype=torch.bool)
    for name in adapter.route.full_names:
        off, n, shape = net._offs[name]
        assert tuple(shape[2:]) == (3, 3)
        slots[off:off + n] = True
    fill = torch.where(slots, torch.zeros(()), torch.full((), NAN))
    net.flat_grad.copy_(fill)
    adapter.zero_grad()
    y = net(d["x"].cuda(), d["t"].cuda())[0]
    (y * d["w"].cuda()).sum().backward()
    adapter.backward_()
    torch.cuda.synchronize()
    got = net.flat_grad.cpu()
    assert torch.equal(bits(got[~slots]), bits(fill[~slots]))                   # shortcuts, biases, GroupNorm, attention, the time MLP: untouched
    assert bool(torch.isfinite(got[slots]).all()) and float(got[slots].abs().sum()) > 0.0
    assert bool(torch.isfinite(adapter.grad).all())


# ------------------------------------------------------------------------------------------------------------ the trajectory
def _random_B(tr):
    tab, ad = tr.adapter.table, tr.adapter
    with torch.no_grad():
        for _, b in tab.slices.values():
            ad.param[b] = (0.05 * torch.randn(b.stop - b.start, generator=g(b.start))).cuda()
    ad.merge_()


@pytest.mark.parametrize("target", ["attn", "all"])
def test_six_adapted_steps_follow_adam_on_the_adapters_of_the_oracle(target):
    cfg = LoRAConfig(r=4, alpha=8.0, target=target, seed=7)
    tr = base.make_trainer(cfg, lora_backward="adapted")
    net, ad, tab = tr.model, tr.adapter, tr.adapter.table
    assert ad.backward == "adapted" and net.lora_route is ad.route
    _random_B(tr)
    start_base, p0, w_start = ad.base.cpu().clone(), ad.param.cpu().clone(), net.flat_param.cpu().clone()
    ref = UNet2DModelRef(**SMALL)
    ref.load_state_dict({k: start_base[off:off + n].view(shape).clone() for k, (off, n, shape) in net._offs.items()})
    oracle = lora_ref.AdamOnAdapters(ref, lora_ref.adapters_of(p0, tab.slices, tab.shapes, cfg.r), cfg.s, lr=1e-3, total_steps=20)
    inside = torch.zeros(net.flat_numel, dtype=torch.bool)
    for off, M, L, *_ in tab.jobs:
        inside[off:off + M * L] = True
    pad = tab.padding_mask()
    for i in range(6):
        x0, R, t, eps = base.batch_of(i)
        loss = tr.train_step({"target": x0.cuda(), "pixel_values": R.cuda()}, t.cuda(), noise=eps.cuda())
        l_ref = oracle.step(x0, R, t, eps)
        assert abs(float(loss) - l_ref) <= 1e-4 * abs(l_ref), (i, float(loss), l_ref)
        now = net.flat_param.cpu()
        assert torch.equal(bits(now[~inside]), bits(start_base[~inside])), i    # every frozen float keeps the base's bits
        assert float(ad.param.cpu()[pad].abs().sum()) == 0.0 and int(tr.opt.skipped) == 0, i
    want_p = lora_ref.flat_of(oracle.adapters, tab.slices, tab.numel)
    upd_ad = base._rel_l2(ad.param.cpu(), want_p, p0)
    msd = oracle.merged_state()
    want_w = start_base.clone()
    for name in tab.slices:
        off, n, _ = net._offs[name]
        want_w[off:off + n] = msd[name].reshape(-1)
    upd_w = base._rel_l2(net.flat_param.cpu(), want_w, w_start)
    print(f"[parity] 6 adapted LoRA steps, target {target}: update L2 error, adapter {upd_ad:.3e}, merged weights {upd_w:.3e}")
    assert upd_ad <= 1e-3, upd_ad
    assert upd_w <= 1e-3, upd_w


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_gradient_accumulation_agrees_with_the_full_backward(graph):
    cfg = LoRAConfig(r=4, alpha=8.0, target="all", seed=7)
    runs = {}
    for mode in ("full", "adapted"):
        tr = base.make_trainer(cfg, lora_backward=mode, grad_accum=2, graph_micro_step=graph)
        _random_B(tr)
        p0 = tr.adapter.param.cpu().clone()
        base.run_steps(tr, 0, 6)                                                # three optimiser steps of two micro-steps
        assert tr.opt.step_count == 3 and bool(tr._graphs) is graph
        runs[mode] = tr.adapter.param.cpu().clone()
    diff = base._rel_l2(runs["adapted"], runs["full"], p0)
    print(f"[parity] grad_accum=2, graph_micro_step={graph}: adapted vs full update L2 {diff:.3e}")
    assert diff <= 2e-3, diff                                                   # each meets 1e-3 against the oracle


# ------------------------------------------------------------------------------------------------------------ determinism, state, "full"
CFG = LoRAConfig(r=4, alpha=8.0, target="all", seed=7)


def test_adapted_runs_repeat_and_resume_bit_exactly_and_states_cross_modes():
    a, b = base.make_trainer(CFG, lora_backward="adapted"), base.make_trainer(CFG, lora_backward="adapted")
    base.run_steps(a, 0, 3)
    base.run_steps(b, 0, 3)
    assert torch.equal(bits(a.adapter.param), bits(b.adapter.param))
    st = base.clone_state(a.state_dict())
    assert set(st["lora"]) == {"param", "base", "config"} and st["lora"]["config"] == CFG.to_dict()
    base.run_steps(a, 3, 6)
    other = base.make_trainer(CFG, seed=99, lora_backward="adapted")
    other.load_state_dict(st)
    base.run_steps(other, 3, 6)
    assert torch.equal(bits(other.adapter.param), bits(a.adapter.param)) and torch.equal(bits(other.model.flat_param), bits(a.model.flat_param))
    full = base.make_trainer(CFG)
    base.run_steps(full, 0, 3)
    st_full = base.clone_state(full.state_dict())
    assert set(st_full) == set(st) and st_full["lora"]["config"] == st["lora"]["config"]
    cross = base.make_trainer(CFG, seed=99, lora_backward="adapted")
    cross.load_state_dict(st_full)                                              # a state saved in "full" loads into "adapted" ...
    assert torch.equal(bits(cross.adapter.param), bits(full.adapter.param)) and torch.equal(bits(cross.model.flat_param), bits(full.model.flat_param))
    base.run_steps(cross, 3, 4)
    back = base.make_trainer(CFG, seed=99)
    back.load_state_dict(st)                                                    # ... and the other way round
    base.run_steps(back, 3, 4)
    assert bool(torch.isfinite(cross.adapter.param).all()) and bool(torch.isfinite(back.adapter.param).all())


def test_full_is_untouched():
    a, b = base.make_trainer(CFG), base.make_trainer(CFG, lora_backward="full")
    assert a.model.lora_route is None and b.model.lora_route is None and b.adapter.backward == "full"
    base.run_steps(a, 0, 3)
    base.run_steps(b, 0, 3)
    assert torch.equal(bits(a.model.flat_param), bits(b.model.flat_param)) and torch.equal(bits(a.adapter.param), bits(b.adapter.param))


# ------------------------------------------------------------------------------------------------------------ the driver
def test_cli_adapted_train_and_resume(tmp_path):
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
           "--save_image_epochs", "1", "--save_model_epochs", "1", "--lora_r", "4", "--lora_backward", "adapted"])
    run = os.path.join(res, os.listdir(res)[0])
    for f in ("unet/diffusion_pytorch_model.safetensors", "unet_lora/adapter_config.json", "unet_lora/adapter_model.safetensors"):
        assert os.path.exists(os.path.join(run, f)), f
    args = json.load(open(os.path.join(run, "args.json")))
    assert args["lora_r"] == 4 and args["lora_backward"] == "adapted"
    assert "backward" not in json.load(open(os.path.join(run, "unet_lora", "adapter_config.json")))
    st = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    assert st["optimizer"]["step"] >= 1 and st["lora"]["config"] == {"r": 4, "alpha": None, "target": "attn", "seed": 0}
    assert float(st["lora"]["param"].abs().sum()) > 0 and bool(torch.isfinite(st["lora"]["param"]).all())
    drive(["--mode", "resume", "--ckpt", run])                                  # takes --lora_backward from args.json
    st2 = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    assert st2["optimizer"]["step"] > st["optimizer"]["step"] and not torch.equal(st2["lora"]["param"], st["lora"]["param"])
    import VillanDiffusion as V
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", run])).lora_backward == "adapted"
