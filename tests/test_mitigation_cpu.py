"""villandiffusion_amd.mitigation without a GPU: import, argument validation before the device is touched, no fallback, the two tools' --help and
the header's declarations of the two entry points."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from villandiffusion_amd.unet import UNet2DModel
    return UNet2DModel(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                       down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), device="cpu")


def _ncsnpp():
    from villandiffusion_amd.ncsnpp import NCSNppModel
    return NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1, device="cpu",
                       down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                       up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))


def _no_device(monkeypatch):
    from villandiffusion_amd import lib
    monkeypatch.setattr(lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device touched before validation")))


def test_public_names():
    from villandiffusion_amd import mitigation
    assert mitigation.__all__ == ["ImageSetStats", "image_set_stats", "BackdoorFeatures", "backdoor_features", "removal_objective",
                                  "BackdoorRemoval", "remove_backdoor"]
    from villandiffusion_amd import defense
    assert mitigation._check_model is defense._check_model and mitigation._frozen is defense._frozen      # imported, not copied
    assert "mitigation" in defense.__doc__


def test_shared_pieces_are_imported_and_a_vp_record_has_no_sigma():
    from villandiffusion_amd import defense, mitigation
    assert mitigation._noise_of is defense._noise_of and mitigation._trainable is defense._trainable
    assert mitigation._check_loop_args is defense._check_loop_args and mitigation._shape is defense._shape
    stats = mitigation.ImageSetStats(n=2, uniformity=1.0, tv=2.0, mean_image=torch.zeros(3, 4, 4))
    f = mitigation.BackdoorFeatures(clean=stats, shifted=stats, uniformity_ratio=1.0, tv_ratio=1.0, n=2, batch=2, num_inference_steps=1, seed=0)
    r = mitigation.BackdoorRemoval(total=[1.0], clean=[0.5], shift=[0.5], frozen=None, lr=1e-4, steps=1, batch=2, w_clean=1.0, w_shift=1.0,
                                   max_grad_norm=1.0, timestep=999, seed=0)
    assert f.sigma is None and r.sigma is None and "sigma" not in f.as_dict()
    assert mitigation.BackdoorFeatures(clean=stats, shifted=stats, uniformity_ratio=1.0, tv_ratio=1.0, n=2, batch=2, num_inference_steps=1, seed=0,
                                       sigma=380.0).sigma == 380.0


def test_remove_backdoor_validates_before_touching_the_device(monkeypatch):
    from villandiffusion_amd import mitigation
    from villandiffusion_amd import schedulers as S
    _no_device(monkeypatch)
    net, sched, tau = _model(), S.DDPMScheduler(), torch.zeros(3, 32, 32)
    ok = dict(steps=2, batch=4, lr=1e-4)
    for bad in (dict(ok, steps=0), dict(ok, steps=-1), dict(ok, steps=2.5), dict(ok, steps=True), dict(ok, batch=0), dict(ok, batch="4"),
                dict(ok, lr=0.0), dict(ok, lr=float("inf")), dict(ok, lr=float("nan")), dict(ok, w_clean=-1.0), dict(ok, w_shift=float("nan")),
                dict(ok, w_shift=float("inf")), dict(ok, max_grad_norm=0.0), dict(ok, timestep=1000), dict(ok, timestep=-1),
                dict(ok, noise=torch.zeros(2, 4, 3, 16, 16)), dict(ok, noise=torch.zeros(3, 4, 3, 32, 32))):
        with pytest.raises(ValueError):
            mitigation.remove_backdoor(net, sched, tau, **bad)
    with pytest.raises(ValueError, match="trigger"):
        mitigation.remove_backdoor(net, sched, torch.zeros(3, 16, 16), **ok)
    with pytest.raises(TypeError):
        mitigation.remove_backdoor(net, sched, tau, noise=3, **ok)
    with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
        mitigation.remove_backdoor(net, S.ScoreSdeVeScheduler(), tau, **ok)
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        mitigation.remove_backdoor(_ncsnpp(), sched, torch.zeros(3, 16, 16), **ok)
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        mitigation.removal_objective(_ncsnpp(), _ncsnpp(), torch.zeros(3, 16, 16), torch.zeros(2, 3, 16, 16), 0)
    with pytest.raises(ValueError):
        mitigation.removal_objective(net, net, torch.zeros(3, 16, 16), torch.zeros(2, 3, 32, 32), 999)
    net.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16"):
        mitigation.remove_backdoor(net, sched, tau, **ok)
    with pytest.raises(NotImplementedError, match="f16"):
        mitigation.removal_objective(net, net, tau, torch.zeros(2, 3, 32, 32), 999)


def test_features_validate_before_touching_the_device(monkeypatch):
    from villandiffusion_amd import mitigation
    from villandiffusion_amd import pipelines as P
    from villandiffusion_amd import schedulers as S
    _no_device(monkeypatch)
    pipe, tau = P.DDIMPipeline(_model(), S.DDIMScheduler()), torch.zeros(3, 32, 32)
    for bad in (dict(n=0, batch=4), dict(n=1, batch=4), dict(n=8.0, batch=4), dict(n=8, batch=0), dict(n=8, batch=True),
                dict(n=8, batch=4, num_inference_steps=0)):
        with pytest.raises(ValueError):
            mitigation.backdoor_features(pipe, tau, **bad)
    with pytest.raises(ValueError, match="trigger"):
        mitigation.backdoor_features(pipe, torch.zeros(3, 16, 16), n=8, batch=4)
    with pytest.raises(NotImplementedError, match="LDMPipeline"):
        mitigation.backdoor_features(P.LDMPipeline(vqvae=object(), unet=_model(), scheduler=S.DDIMScheduler()), tau, n=8, batch=4)
    with pytest.raises(NotImplementedError, match="ScoreSdeVePipeline"):
        mitigation.backdoor_features(P.ScoreSdeVePipeline(_ncsnpp(), S.ScoreSdeVeScheduler()), torch.zeros(3, 16, 16), n=8, batch=4)
    with pytest.raises(TypeError):
        mitigation.backdoor_features(object(), tau, n=8, batch=4)
    for bad in (torch.zeros(1, 3, 8, 8), torch.zeros(0, 3, 8, 8), torch.zeros(3, 8, 8)):
        with pytest.raises(ValueError):
            mitigation.image_set_stats(bad)
    with pytest.raises(TypeError):                             # the threshold is the caller's: there is no default
        mitigation.BackdoorFeatures.verdict(object())


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_gpu():
    from villandiffusion_amd import lib, mitigation
    from villandiffusion_amd import pipelines as P
    from villandiffusion_amd import schedulers as S
    tau = torch.zeros(3, 32, 32)
    with pytest.raises(lib.VillanHipError):
        mitigation.remove_backdoor(_model(), S.DDPMScheduler(), tau, steps=1, batch=1, lr=1e-4)
    with pytest.raises(lib.VillanHipError):
        mitigation.removal_objective(_model(), _model(), tau, torch.zeros(1, 3, 32, 32), 999)
    with pytest.raises(lib.VillanHipError):
        mitigation.image_set_stats(torch.zeros(2, 3, 32, 32))
    with pytest.raises(lib.VillanHipError):
        mitigation.backdoor_features(P.DDIMPipeline(_model(), S.DDIMScheduler()), tau, n=4, batch=2, num_inference_steps=2)


@pytest.mark.parametrize("tool,flags", [
    ("detect_backdoor.py", ("--ckpt", "--trigger", "--n", "--batch", "--steps", "--seed", "--threshold", "--out")),
    ("remove_backdoor.py", ("--ckpt", "--trigger", "--steps", "--batch", "--lr", "--w-clean", "--w-shift", "--seed", "--out"))])
def test_tool_help_exits_zero(tool, flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in flags:
        assert flag in out.stdout, flag


def test_header_declares_both_entry_points_and_the_wrappers_exist():
    from villandiffusion_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    for name, n_args in (("vd_removal_loss", 12), ("vd_image_set_stats", 14)):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args
        assert name in lib.PROTOTYPES and len(lib.PROTOTYPES[name][1]) == n_args
    assert callable(ops.removal_loss) and callable(ops.image_set_stats)
    assert re.search(r"#define VD_ABI_VERSION 12\b", hdr)
    mk = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_defense.hip" in mk and re.search(r"vd_defense\.o:.*\n\t.*-ffp-contract=off", mk)


def test_abi_version_is_12():
    from villandiffusion_amd import lib
    assert lib.load().vd_abi_version() == 12
