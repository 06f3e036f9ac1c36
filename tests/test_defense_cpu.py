"""villandiffusion_amd.defense without a GPU: import, argument validation before the device is touched, no fallback, the tool's --help and the
header's declaration of the objective's entry point."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from villandiffusion_amd.unet import UNet2DModel
    return UNet2DModel(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                       down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), device="cpu")


def test_defense_imports_and_validates_before_touching_the_device(monkeypatch):
    from villandiffusion_amd import defense, lib
    from villandiffusion_amd import schedulers as S
    assert set(defense.__all__) == {"TriggerInversion", "inversion_objective", "invert_trigger"}
    monkeypatch.setattr(lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device touched before validation")))
    net, sched = _model(), S.DDPMScheduler()
    for bad in (dict(steps=0, batch=4), dict(steps=-1, batch=4), dict(steps=2.5, batch=4), dict(steps=2, batch=0), dict(steps=2, batch="4"),
                dict(steps=2, batch=4, lam=float("nan")), dict(steps=2, batch=4, lam=float("inf")), dict(steps=2, batch=4, lr=0.0),
                dict(steps=2, batch=4, noise=torch.zeros(2, 4, 3, 16, 16)), dict(steps=2, batch=4, noise=torch.zeros(3, 4, 3, 32, 32)),
                dict(steps=2, batch=4, init=torch.zeros(3, 16, 16)), dict(steps=2, batch=4, timestep=1000)):
        with pytest.raises(ValueError):
            defense.invert_trigger(net, sched, **bad)
    with pytest.raises(TypeError):
        defense.invert_trigger(net, sched, steps=2, batch=4, noise=3)
    with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
        defense.invert_trigger(net, S.ScoreSdeVeScheduler(), steps=2, batch=4)
    from villandiffusion_amd.ncsnpp import NCSNppModel
    pp = NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1, device="cpu",
                     down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                     up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        defense.invert_trigger(pp, sched, steps=2, batch=4)
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        defense.inversion_objective(pp, torch.zeros(3, 16, 16), torch.zeros(2, 3, 16, 16), 0)


def test_frozen_flags_are_restored_after_an_exception():
    from villandiffusion_amd import defense
    net = _model()
    first = next(net.parameters())
    first.requires_grad_(False)                       # a mix of frozen and trainable parameters comes back as it was
    flags = [p.requires_grad for p in net.parameters()]
    with pytest.raises(RuntimeError, match="boom"):
        with defense._frozen(net):
            assert not any(p.requires_grad for p in net.parameters())
            raise RuntimeError("boom")
    assert [p.requires_grad for p in net.parameters()] == flags and not flags[0] and all(flags[1:])


def test_trainable_is_the_mirror_of_frozen_and_restores_after_an_exception():
    from villandiffusion_amd import defense
    net = _model()
    params = list(net.parameters())
    params[0].requires_grad_(False)                   # frozen by the caller: trainable inside, frozen again afterwards
    params[2].requires_grad_(False)                   # in `skip`: never switched on
    flags = [p.requires_grad for p in params]
    with defense._trainable(net, skip=(params[2],)):
        assert [p.requires_grad for p in params] == [i != 2 for i in range(len(params))]
    assert [p.requires_grad for p in params] == flags
    with pytest.raises(RuntimeError, match="boom"):
        with defense._trainable(net, skip=(params[2],)):
            assert all(p.requires_grad for i, p in enumerate(params) if i != 2) and not params[2].requires_grad
            raise RuntimeError("boom")
    assert [p.requires_grad for p in params] == flags and not flags[0] and not flags[2] and all(flags[3:]) and flags[1]


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_gpu():
    from villandiffusion_amd import defense, lib
    from villandiffusion_amd import schedulers as S
    with pytest.raises(lib.VillanHipError):
        defense.invert_trigger(_model(), S.DDPMScheduler(), steps=1, batch=1)
    with pytest.raises(lib.VillanHipError):
        defense.inversion_objective(_model(), torch.zeros(3, 32, 32), torch.zeros(1, 3, 32, 32), 999)


def test_tool_help_exits_zero():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "invert_trigger.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--ckpt", "--steps", "--batch", "--lam", "--lr", "--seed", "--out"):
        assert flag in out.stdout, flag


def test_header_declares_the_objective_and_the_wrapper_exists():
    from villandiffusion_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "int vd_trigger_inv_objective(" in hdr
    assert "vd_trigger_inv_objective" in lib.PROTOTYPES and len(lib.PROTOTYPES["vd_trigger_inv_objective"][1]) == 11
    assert callable(ops.trigger_inv_objective)


def test_input_gradient_switch_is_on_for_the_unet_and_off_for_ncsnpp():
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.unet import UNet2DModel
    assert UNet2DModel._input_grad is True and NCSNppModel._input_grad is False
    net = _model()
    assert "conv_in" in net._wt_offs and net._wt_total == sum(
        p.numel() for n, p in net.named_parameters() if n.endswith(".weight") and p.dim() == 4 and p.shape[2] == 3)
