"""Trigger inversion (villandiffusion_amd.defense): the fused objective kernel against float64 torch, inversion_objective against the CPU oracle,
the Adam update of the trigger against torch.optim.Adam, and invert_trigger end to end."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import defense, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def pair():
    torch.manual_seed(0)
    ref = UNet2DModelRef()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    net = UNet2DModel()
    net.load_state_dict(ref.state_dict())
    return ref, net


def _objective(e, tau, lam):
    B = e.shape[0]
    loss = torch.empty(1, device=DEV)
    dout = torch.full_like(e, float("nan"))
    dtau = torch.full_like(tau, float("nan"))
    partial = torch.empty(1024, device=DEV)
    ops.trigger_inv_objective(e, tau, lam, loss, dout, dtau, partial)
    torch.cuda.synchronize()
    return loss, dout, dtau


# ------------------------------------------------------------------------------------------------------------ 7. the objective kernel
@pytest.mark.parametrize("B", [1, 4, 100])
@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 64, 64), (5, 7, 9)])
def test_objective_kernel_against_float64(B, shape):
    lam = 0.5
    e = torch.randn((B,) + shape, generator=g(B))
    tau = torch.rand(shape, generator=g(B + 1))
    e64 = e.double().requires_grad_(True)
    t64 = tau.double().requires_grad_(True)
    r = e64.mean(0) - lam * t64
    L = r.norm()
    L.backward()
    dtau_direct = -lam * r.detach() / L.detach()                 # (t64.grad is the same thing: e64 does not depend on tau here)
    assert torch.allclose(t64.grad, dtau_direct)
    loss, dout, dtau = _objective(e.to(DEV), tau.to(DEV), lam)
    e_loss = abs(float(loss) - L.item()) / L.item()
    e_dout = float((dout.double().cpu() - e64.grad).abs().max() / e64.grad.abs().max())
    e_dtau = float((dtau.double().cpu() - dtau_direct).abs().max() / dtau_direct.abs().max())
    print(f"[parity] trigger-inversion objective B={B} {shape}: loss {e_loss:.2e}, dout {e_dout:.2e}, dtau_direct {e_dtau:.2e}")
    assert e_loss <= 1e-6 and e_dout <= 1e-6 and e_dtau <= 1e-6
    again = _objective(e.to(DEV), tau.to(DEV), lam)
    assert torch.equal(again[0], loss) and torch.equal(again[1], dout) and torch.equal(again[2], dtau)     # fixed summation order


def test_objective_kernel_zero_residual_and_strided_input():
    lam = 0.5
    tau = torch.rand(3, 32, 32, generator=g(3)) * 2          # lam * tau is exact, and so is the mean of 4 equal images
    e = (lam * tau).expand(4, 3, 32, 32).contiguous()
    loss, dout, dtau = _objective(e.to(DEV), tau.to(DEV), lam)
    assert float(loss) == 0.0 and float(dout.abs().max()) == 0.0 and float(dtau.abs().max()) == 0.0       # no NaN
    # e as a channel slice of a wider buffer (batch stride > C*H*W)
    buf = torch.randn(4, 8, 32, 32, generator=g(4)).to(DEV)
    a = _objective(buf[:, 2:5], tau.to(DEV), lam)
    b = _objective(buf[:, 2:5].contiguous(), tau.to(DEV), lam)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and float(a[0]) > 0


# ------------------------------------------------------------------------------------------------------------ 8. against the oracle
def _oracle_objective(ref, tau, eps, t, lam):
    tr = tau.clone().requires_grad_(True)
    e = ref(eps + tr, t)[0]
    L = (e.mean(0) - lam * tr).norm()
    L.backward()
    ref.zero_grad()
    return L.item(), tr.grad


def test_inversion_objective_matches_oracle(pair):
    ref, net = pair
    B, lam = 4, 0.5
    eps = torch.randn(B, 3, 32, 32, generator=g(5))
    tau = torch.rand(3, 32, 32, generator=g(6))
    t = torch.full((B,), 999)
    L_ref, dtau_ref = _oracle_objective(ref, tau, eps, t, lam)
    flags = [p.requires_grad for p in net.parameters()]
    loss, dtau = defense.inversion_objective(net, tau.to(DEV), eps.to(DEV), t.to(DEV), lam)
    assert [p.requires_grad for p in net.parameters()] == flags and all(flags)
    e_loss = abs(float(loss) - L_ref) / L_ref
    e_g = float((dtau.double().cpu() - dtau_ref.double()).abs().max() / dtau_ref.double().abs().max())
    print(f"[parity] inversion_objective: L={float(loss):.4f} (oracle {L_ref:.4f}, rel {e_loss:.2e}); dtau rel_err {e_g:.2e} "
          f"(max|dtau_ref| {float(dtau_ref.abs().max()):.3e})")
    assert e_loss <= 1e-5 and e_g <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 9. one Adam iteration
def test_one_adam_iteration_matches_torch(pair):
    ref, net = pair
    B, lam = 4, 0.5
    eps = torch.randn(B, 3, 32, 32, generator=g(5))
    tau0 = torch.rand(3, 32, 32, generator=g(6))
    _, dtau_ref = _oracle_objective(ref, tau0, eps, torch.full((B,), 999), lam)      # the oracle's gradient: rounding-level sign flips are not the subject
    p = tau0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.1)
    p.grad = dtau_ref.clone()
    opt.step()
    tau = tau0.to(DEV)
    m, v = torch.zeros_like(tau), torch.zeros_like(tau)
    epoch = ops.WEIGHTS_EPOCH
    defense.adam_update(tau, dtau_ref.to(DEV), m, v, 1, 0.1)
    assert ops.WEIGHTS_EPOCH == epoch                            # the trigger is no network weight: packed operands stay valid
    err = float((tau.cpu() - p.detach()).abs().max())
    print(f"[parity] Adam step on the trigger vs torch.optim.Adam: max abs err {err:.2e}")
    assert err <= 1e-6 and float((tau.cpu() - tau0).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------------------ 10. end to end
def test_invert_trigger_end_to_end(pair):
    ref, net = pair
    steps, batch = 8, 4
    noise = torch.randn(steps, batch, 3, 32, 32, generator=g(7))
    sched = S.DDPMScheduler()
    sentinel = (torch.arange(net.flat_grad.numel(), device=DEV, dtype=torch.float32) % 127.0) - 63.0
    net.flat_grad.copy_(sentinel)
    flags = [p.requires_grad for p in net.parameters()]
    try:
        res = defense.invert_trigger(net, sched, steps=steps, batch=batch, seed=3, noise=noise)
        assert [p.requires_grad for p in net.parameters()] == flags and all(flags)
        assert torch.equal(net.flat_grad, sentinel)
        assert len(res.losses) == steps and all(math.isfinite(x) for x in res.losses)
        print(f"[inversion] losses {['%.4f' % x for x in res.losses]}, ||tau|| {res.trigger_norm:.3f}")
        assert res.losses[-1] < res.losses[0]
        assert res.timestep == 999 and tuple(res.trigger.shape) == (3, 32, 32)
        res2 = defense.invert_trigger(net, sched, steps=steps, batch=batch, seed=3, noise=lambda i: noise[i])
        assert res2.losses == res.losses and torch.equal(res2.trigger, res.trigger)
        # device noise (Philox): reproducible for the same seed, different for another
        a = defense.invert_trigger(net, sched, steps=2, batch=batch, seed=11)
        b = defense.invert_trigger(net, sched, steps=2, batch=batch, seed=11)
        c = defense.invert_trigger(net, sched, steps=2, batch=batch, seed=12)
        assert a.losses == b.losses and torch.equal(a.trigger, b.trigger) and a.losses != c.losses
        # flags come back after an exception inside the loop too
        with pytest.raises(ValueError):
            defense.invert_trigger(net, sched, steps=2, batch=batch, noise=lambda i: noise[i][:1])
        assert [p.requires_grad for p in net.parameters()] == flags
    finally:
        net.zero_grad()


def test_invert_trigger_refuses_what_it_is_not_built_for(pair):
    from villandiffusion_amd.ncsnpp import NCSNppModel
    ref, net = pair
    small = dict(sample_size=16, block_out_channels=(32, 64, 64),
                 down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                 up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        defense.invert_trigger(NCSNppModel(**small), S.DDPMScheduler(), steps=1, batch=1)
    with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
        defense.invert_trigger(net, S.ScoreSdeVeScheduler(), steps=1, batch=1)


def test_tool_writes_the_trigger_and_its_record(tmp_path):
    """tools/invert_trigger.py on a (small) diffusers-format checkpoint written by the project's own save_pretrained, in a child process."""
    import json
    import os
    import subprocess
    import sys
    from villandiffusion_amd.pipelines import DDPMPipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net = UNet2DModel(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                      down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
    net.reset_parameters(seed=1)
    ckpt, out = str(tmp_path / "ckpt"), str(tmp_path / "out")
    DDPMPipeline(net, S.DDPMScheduler()).save_pretrained(ckpt)
    run = subprocess.run([sys.executable, os.path.join(root, "tools", "invert_trigger.py"), "--ckpt", ckpt, "--steps", "3", "--batch", "4",
                          "--seed", "2", "--out", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    info = json.load(open(os.path.join(out, "trigger_inv.json")))
    tau = torch.load(os.path.join(out, "trigger_inv.pt"))
    assert info["steps"] == 3 and info["batch"] == 4 and info["seed"] == 2 and info["timestep"] == 999 and len(info["losses"]) == 3
    assert all(math.isfinite(x) for x in info["losses"]) and tuple(tau.shape) == (3, 32, 32)
    assert abs(info["trigger_l2"] - float(tau.double().norm())) <= 1e-6 * info["trigger_l2"]
