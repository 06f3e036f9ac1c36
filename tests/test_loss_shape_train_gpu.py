"""The shaped loss through the networks: LossFn(snr_gamma / poison_weight / track_split) on the small UNet and a small NCSN++ against autograd
through the oracle with the weighted loss of loss_shape_ref.py (the gates of test_unet_gpu.py: loss 1e-5, gradient norm 1e-4, every parameter
gradient 1e-3 of its scale), the identities with the unshaped loss, the graphed micro-step, loss_profile and the driver in child processes."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import anp_families_ref as fam  # noqa: E402
import loss_shape_ref as R  # noqa: E402
from oracle.loss_ref import SDE_VE, SDE_VP, LossFnRef  # noqa: E402
from oracle.schedulers_ref import DDPMSchedulerRef, ScoreSdeVeSchedulerRef  # noqa: E402
from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.loss_profile import loss_profile  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.pipelines import DDPMPipeline  # noqa: E402
from villandiffusion_amd.trainer import Trainer  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_lora_gpu.py's
PP1 = dict(fam.SMALL_PP, layers_per_block=1)


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def vp_batch(B=8, seed=5, size=32):
    gen = g(seed)
    x0 = torch.rand(B, 3, size, size, generator=gen) * 2 - 1
    Rr = torch.rand(B, 3, size, size, generator=gen) * 2 - 1
    poison = torch.arange(B) % 3 == 1                               # both classes
    Rr[~poison] = 0
    eps = torch.randn(B, 3, size, size, generator=gen)
    t = torch.tensor([0, 1, 64, 129, 130, 400, 998, 999][:B])       # below and above the 130 timesteps min-SNR (gamma 5) weighs down
    return x0, Rr, eps, t, poison


@pytest.fixture(scope="module")
def small_ref():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**SMALL)
    fam.perturb_norms(ref)
    return ref


def gates(what, net, loss, ref_model, loss_ref):
    gref = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in ref_model.named_parameters()}      # (a parameter the oracle never uses)
    gmax = max(float(v.abs().max()) for v in gref.values())
    gn_ref = float(torch.sqrt(sum((v.double() ** 2).sum() for v in gref.values())))
    e_loss = abs(float(loss.detach()) - float(loss_ref.detach())) / abs(float(loss_ref.detach()))
    e_gn = abs(float(torch.sqrt((net.flat_grad.double() ** 2).sum())) - gn_ref) / gn_ref
    worst = (0.0, "")
    for n, p in net.named_parameters():
        a, b = p.grad.detach().double().cpu(), gref[n].double()
        e = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))
        worst = max(worst, (e, n))
    print(f"[parity] {what}: loss {e_loss:.2e}, grad-norm {e_gn:.2e}, worst param-grad {worst[0]:.2e} at {worst[1]}")
    assert e_loss <= 1e-5 and e_gn <= 1e-4 and worst[0] <= 1e-3, (what, e_loss, e_gn, worst)


def small_net(ref):
    net = UNet2DModel(**SMALL)
    net.load_state_dict(ref.state_dict())
    net.zero_grad()
    return net


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def test_vp_min_snr_and_poison_weight_against_the_oracle(small_ref):
    x0, Rr, eps, t, poison = vp_batch()
    lref = LossFnRef(DDPMSchedulerRef(), SDE_VP, psi=1)
    w = R.oracle_weights(lref, t, poison, snr_gamma=5.0, pw=2.0)
    assert float(w.min()) < 1e-3 and float(w.max()) == 2.0 and len(set(w.tolist())) >= 5
    small_ref.zero_grad()
    loss_ref, l_ref = R.oracle_shaped_loss(lref, small_ref, x0, Rr, t, eps, w)
    loss_ref.backward()
    net = small_net(small_ref)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, snr_gamma=5.0, poison_weight=2.0, track_split=True)
    loss = lf.p_loss_by_keys({"target": x0.cuda(), "pixel_values": Rr.cuda(), "is_clean": ~poison}, net, "target", "pixel_values", t.cuda(),
                             noise=eps.cuda())
    loss.backward()
    torch.cuda.synchronize()
    gates("VP gamma 5, poison weight 2", net, loss, small_ref, loss_ref)
    sl, ld = lf.last_sample_loss.double().cpu(), l_ref.detach().double()
    assert float(((sl - ld).abs() / ld).max()) <= 1e-5, "the per-sample losses are the oracle's"
    st = lf.last_split.double().cpu()
    assert st[[1, 3]].tolist() == [float((~poison).sum()), float(poison.sum())]
    assert abs(float(st[0]) - float(ld[~poison].sum())) <= 1e-5 * float(ld[~poison].sum()) and abs(float(st[2]) - float(ld[poison].sum())) <= 1e-5 * float(ld[poison].sum())
    # an explicit weight per sample multiplies in
    sw = torch.tensor([1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 3.0])
    small_ref.zero_grad()
    loss_ref2, _ = R.oracle_shaped_loss(lref, small_ref, x0, Rr, t, eps, w * sw.double())
    loss_ref2.backward()
    net.zero_grad()
    loss2 = lf.p_loss(net, x0.cuda(), Rr.cuda(), t.cuda(), noise=eps.cuda(), is_poison=poison, sample_weight=sw)
    loss2.backward()
    gates("VP gamma 5, poison weight 2, sample weights", net, loss2, small_ref, loss_ref2)


def test_ve_poison_weight_against_the_oracle():
    ref = fam.small_ncsnpp(1)
    B = 8
    gen = g(9)
    x0 = torch.rand(B, 3, 16, 16, generator=gen)
    Rr = torch.rand(B, 3, 16, 16, generator=gen)
    poison = torch.arange(B) % 3 == 1
    Rr[~poison] = 0
    eps = torch.randn(B, 3, 16, 16, generator=gen)
    t = torch.tensor([0, 5, 300, 700, 1000, 1400, 1900, 1999])
    lref = LossFnRef(ScoreSdeVeSchedulerRef(**fam.VE_SCHED), SDE_VE, psi=0)
    w = R.oracle_weights(lref, t, poison, pw=2.0)
    ref.zero_grad()
    loss_ref, _ = R.oracle_shaped_loss(lref, ref, x0, Rr, t, eps, w)
    loss_ref.backward()
    net = NCSNppModel(**PP1)
    net.load_state_dict(ref.state_dict())
    net.zero_grad()
    with pytest.raises(NotImplementedError, match="snr_gamma"):
        LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0, snr_gamma=5.0)
    lf = LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0, poison_weight=2.0)
    loss = lf.p_loss_by_keys({"target": x0.cuda(), "pixel_values": Rr.cuda(), "is_clean": ~poison}, net, "target", "pixel_values", t.cuda(),
                             noise=eps.cuda())
    loss.backward()
    torch.cuda.synchronize()
    gates("VE poison weight 2", net, loss, ref, loss_ref)
    assert lf.last_split.cpu()[[1, 3]].tolist() == [float((~poison).sum()), float(poison.sum())]


# ---------------------------------------------------------------------------------------------------------- identities through the network
def test_neutral_shaping_is_the_unshaped_gradient_and_an_unshaped_trainer_never_calls_the_kernel(small_ref, monkeypatch):
    calls = {"shaped": 0, "plain": 0}
    real_s, real_p = ops.loss_sample_fwd_bwd, ops.mse_fwd_bwd
    monkeypatch.setattr(ops, "loss_sample_fwd_bwd", lambda *a, **k: (calls.__setitem__("shaped", calls["shaped"] + 1), real_s(*a, **k))[1])
    monkeypatch.setattr(ops, "mse_fwd_bwd", lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), real_p(*a, **k))[1])
    x0, Rr, eps, t, poison = vp_batch()
    batch = {"target": x0.cuda(), "pixel_values": Rr.cuda(), "is_clean": ~poison}
    grads, losses = {}, {}
    for name, kw in (("plain", {}), ("neutral", dict(snr_gamma=1e6, poison_weight=1.0, track_split=True))):
        net = small_net(small_ref)
        lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, **kw)
        loss = lf.p_loss_by_keys(batch, net, "target", "pixel_values", t.cuda(), noise=eps.cuda())
        loss.backward()
        torch.cuda.synchronize()
        grads[name], losses[name] = net.flat_grad.clone(), float(loss.detach())
    assert calls == {"shaped": 1, "plain": 1}
    assert torch.equal(grads["plain"], grads["neutral"]) and float(grads["plain"].abs().max()) > 0
    assert abs(losses["plain"] - losses["neutral"]) <= 1e-6 * losses["plain"]
    for graphed in (False, True):                              # an unshaped Trainer, eager and graphed: the kernels it always ran
        calls.update(shaped=0, plain=0)
        tr = Trainer(small_net(small_ref), LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), lr=1e-3, total_steps=20, warmup_steps=0, grad_accum=2,
                     graph_micro_step=graphed)
        for _ in range(2):
            tr.train_step(batch, t.cuda(), noise=eps.cuda())
        torch.cuda.synchronize()
        assert calls["shaped"] == 0 and calls["plain"] >= 2 and tr.loss_fn.last_split is None, (graphed, calls)


# ----------------------------------------------------------------------------------------------------------------------------- graph
def test_graphed_shaped_micro_step_is_the_eager_one(small_ref):
    """test_graphed_micro_step_is_the_eager_micro_step with shaping on: 3 G micro-steps, G = 4, bit for bit -- losses, the mid-window gradient,
    the split, the parameters -- with poison_weight changed between the second and the third window, which rebuilds the graph."""
    G, B = 4, 4
    out = {}
    for graphed in (False, True):
        net = small_net(small_ref)
        lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, snr_gamma=5.0, poison_weight=2.0, track_split=True)
        lf.noise_seed = 77
        tr = Trainer(net, lf, lr=1e-3, total_steps=100, warmup_steps=0, grad_accum=G, graph_micro_step=graphed)
        losses, snaps, splits, built = [], [], [], []
        for k in range(3 * G):
            x0, Rr, eps, _, _ = vp_batch(B, seed=200 + k)
            gen = g(300 + k)
            t = torch.randint(0, 1000, (B,), generator=gen)
            t[0] = k                                              # some below 130
            poison = torch.rand(B, generator=gen) < 0.5
            if k == 2 * G:
                lf.poison_weight = 3.0
            noise = eps.cuda() if k % 2 == 0 else None
            losses.append(float(tr.train_step({"target": x0.cuda(), "pixel_values": Rr.cuda(), "is_clean": ~poison}, t.cuda(), noise=noise)))
            splits.append(lf.last_split.cpu().clone())
            built.append(next(iter(tr._graphs.values())).key[-1] if tr._graphs else None)      # the shaping the replayed graph was captured with
            if k == G - 2:
                snaps.append(net.flat_grad.clone())
        torch.cuda.synchronize()
        assert tr.opt.step_count == 3 and (len(tr._graphs) == 1) == graphed
        if graphed:
            assert set(built[:2 * G]) == {(5.0, 2.0, True)} and set(built[2 * G:]) == {(5.0, 3.0, True)}, "the new poison weight rebuilt the graph"
        out[graphed] = (losses, snaps, net.flat_param.clone(), torch.stack(splits))
    assert out[False][0] == out[True][0]
    assert torch.equal(out[False][1][0], out[True][1][0]) and float(out[True][1][0].abs().max()) > 0
    assert torch.equal(bits(out[False][3]), bits(out[True][3]))
    assert torch.equal(out[False][2], out[True][2])
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, poison_weight=2.0)
    tr = Trainer(small_net(small_ref), lf, lr=1e-3, total_steps=100, warmup_steps=0, grad_accum=G, graph_micro_step=True)
    x0, Rr, eps, t, _ = vp_batch(B)
    with pytest.raises(ValueError, match="flags"):
        tr.train_step({"target": x0.cuda(), "pixel_values": Rr.cuda()}, t[:B].cuda(), noise=eps.cuda())


# --------------------------------------------------------------------------------------------------------------------------- profile
def test_loss_profile_against_the_oracle(small_ref):
    x0, Rr, _, _, poison = vp_batch(8, seed=11)
    ts = [0, 129, 500, 999]
    net = small_net(small_ref)
    before = bits(net.flat_param)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, snr_gamma=5.0)
    res = loss_profile(net, lf, {"target": x0, "pixel_values": Rr, "is_clean": ~poison}, ts, noise_seed=3)
    noise = torch.empty(8, 3, 32, 32, device="cuda")
    ops.randn(noise, 3, 0)
    lref = LossFnRef(DDPMSchedulerRef(), SDE_VP, psi=1)
    assert res["timesteps"] == ts and (res["n_clean"], res["n_poison"]) == (int((~poison).sum()), int(poison.sum()))
    with torch.no_grad():
        for k, t in enumerate(ts):
            _, l = R.oracle_shaped_loss(lref, small_ref, x0, Rr, torch.full((8,), t), noise.cpu())
            for key, sel in (("loss_clean", ~poison), ("loss_poison", poison)):
                want = float(l[sel].double().mean())
                print(f"[parity] loss_profile t={t} {key}: {res[key][k]:.6e} vs {want:.6e}")
                assert abs(res[key][k] - want) <= 1e-5 * want, (t, key, res[key][k], want)
    assert res["snr_weight"] == [float(lf.snr_table()[t]) for t in ts] and res["snr_weight"][0] < 1e-3 and res["snr_weight"][-1] == 1.0
    assert torch.equal(bits(net.flat_param), before) and float(net.flat_grad.abs().max()) == 0.0, "the model is left alone"
    allc = loss_profile(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), {"target": x0, "pixel_values": Rr, "is_clean": torch.ones(8, dtype=torch.bool)}, [10])
    assert allc["loss_poison"] == [None] and allc["n_poison"] == 0 and "snr_weight" not in allc
    with pytest.raises(NotImplementedError, match="SDE-LDM"):
        loss_profile(net, LossFn(S.DDPMScheduler(), "SDE-LDM"), {"target": x0, "pixel_values": Rr, "is_clean": ~poison}, [10])
    with pytest.raises(NotImplementedError, match="UNet2DModel"):
        loss_profile(net, LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0), {"target": x0, "pixel_values": Rr, "is_clean": ~poison}, [10])
    with pytest.raises(ValueError, match="timesteps"):
        loss_profile(net, lf, {"target": x0, "pixel_values": Rr, "is_clean": ~poison}, [1000])


def test_loss_profile_ve_runs_on_ncsnpp():
    ref = fam.small_ncsnpp(1)
    net = NCSNppModel(**PP1)
    net.load_state_dict(ref.state_dict())
    gen = g(4)
    x0, Rr = torch.rand(8, 3, 16, 16, generator=gen), torch.rand(8, 3, 16, 16, generator=gen)
    poison = torch.arange(8) % 2 == 1
    Rr[~poison] = 0
    ts = [0, 700, 1999]
    res = loss_profile(net, LossFn(S.ScoreSdeVeScheduler(**fam.VE_SCHED), "SDE-VE", psi=0), {"target": x0, "pixel_values": Rr, "is_clean": ~poison}, ts, noise_seed=1)
    noise = torch.empty(8, 3, 16, 16, device="cuda")
    ops.randn(noise, 1, 0)
    lref = LossFnRef(ScoreSdeVeSchedulerRef(**fam.VE_SCHED), SDE_VE, psi=0)
    with torch.no_grad():
        for k, t in enumerate(ts):
            _, l = R.oracle_shaped_loss(lref, ref, x0, Rr, torch.full((8,), t), noise.cpu())
            for key, sel in (("loss_clean", ~poison), ("loss_poison", poison)):
                want = float(l[sel].double().mean())
                assert abs(res[key][k] - want) <= 1e-5 * want, (t, key, res[key][k], want)


# ---------------------------------------------------------------------------------------------------------------------------- driver
def test_cli_shaped_train_resume_and_profile(tmp_path):
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
        return out.stdout

    res = str(tmp_path / "res")
    log = drive(["--mode", "train", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "8", "--epoch", "1", "--poison_rate", "0.5", "--trigger", "BOX_14",
                 "--target", "HAT", "--ckpt", "SMALL-BASE", "--fclip", "o", "-o", "--result", res, "--sched", "DDIM-SCHED", "--infer_steps", "2",
                 "--save_image_epochs", "1", "--save_model_epochs", "1", "--snr_gamma", "5", "--poison_loss_weight", "2", "--log_loss_split"])
    run = os.path.join(res, os.listdir(res)[0])
    for side in ("args.json", "config.json"):
        d = json.load(open(os.path.join(run, side)))
        assert (d["snr_gamma"], d["poison_loss_weight"], d["log_loss_split"]) == (5.0, 2.0, True), side
    lines = [ln for ln in log.splitlines() if ln.startswith("epoch ") and " loss_clean " in ln]
    assert lines, log[-2000:]
    f = lines[-1].split()
    clean, pois = f[f.index("loss_clean") + 1], f[f.index("loss_poison") + 1]
    assert float(clean) > 0 and float(pois) > 0, lines[-1]                      # poison rate 0.5: both classes had samples
    st = torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")
    log2 = drive(["--mode", "resume", "--ckpt", run])                           # resume takes the flags from args.json
    assert any(" loss_clean " in ln and " loss_poison " in ln for ln in log2.splitlines()), log2[-2000:]
    assert torch.load(os.path.join(run, "ckpt", "trainer.pt"), map_location="cpu")["optimizer"]["step"] > st["optimizer"]["step"]
    out = str(tmp_path / "profile")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loss_profile.py"), "--ckpt", run, "--dataset", "SYNTHETIC-CIFAR10", "--trigger", "BOX_14",
                        "--target", "HAT", "--n", "16", "--t-grid", "3", "--snr-gamma", "5", "--out", out], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.load(open(os.path.join(out, "loss_profile.json")))
    assert rec["timesteps"] == [0, 500, 999] and rec["n_clean"] + rec["n_poison"] == 16 and rec["n_clean"] > 0 and rec["n_poison"] > 0
    assert all(v > 0 for v in rec["loss_clean"] + rec["loss_poison"]) and len(rec["snr_weight"]) == 3
