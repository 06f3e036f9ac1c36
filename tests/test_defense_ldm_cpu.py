"""villandiffusion_amd.defense_ldm without a GPU: the module surface, the new entry point in the header and the ctypes table, every refusal and
argument check before the device is touched and the tools' argument parsing.  (The VQModel's input-gradient switch and its answers as a frozen
network: tests/test_flat_layout_cpu.py.)"""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VQ = dict(block_out_channels=(32, 64), down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2,
          layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3, sample_size=16)


def _unet():
    from villandiffusion_amd.unet import UNet2DModel
    return UNet2DModel(sample_size=8, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                       down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), device="cpu")


def _vq():
    from villandiffusion_amd.vqmodel import VQModel
    return VQModel(**VQ, device="cpu")


def _pipe(sched=None):
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.pipelines import LDMPipeline
    return LDMPipeline(vqvae=_vq(), unet=_unet(), scheduler=sched if sched is not None else S.DDIMScheduler())


def test_module_surface():
    from villandiffusion_amd import defense, defense_ldm, mitigation
    assert defense_ldm.__all__ == ["ImageSetAccumulator", "LDMBackdoorFeatures", "trigger_space", "encode_trigger", "render_trigger",
                                   "inversion_objective", "invert_trigger", "backdoor_features", "remove_backdoor"]
    assert all(callable(getattr(defense_ldm, n)) for n in defense_ldm.__all__)
    # reused, not copied
    assert defense_ldm.TriggerInversion is defense.TriggerInversion and defense_ldm._objective_into is defense._objective_into
    assert defense_ldm.adam_update is defense.adam_update and defense_ldm._feature_inits is mitigation._feature_inits
    assert defense_ldm.BackdoorRemoval is mitigation.BackdoorRemoval and defense_ldm.ImageSetStats is mitigation.ImageSetStats
    assert issubclass(defense_ldm.LDMBackdoorFeatures, mitigation.BackdoorFeatures)
    st = mitigation.ImageSetStats(n=2, uniformity=1.0, tv=2.0, mean_image=torch.zeros(1))
    f = defense_ldm.LDMBackdoorFeatures(clean=st, shifted=st, uniformity_ratio=1.0, tv_ratio=1.0, n=2, batch=2, num_inference_steps=1, seed=0,
                                        latent_clean=st, latent_shifted=st, latent_uniformity_ratio=1.0, space="pixel")
    parent = mitigation.BackdoorFeatures(clean=st, shifted=st, uniformity_ratio=1.0, tv_ratio=1.0, n=2, batch=2, num_inference_steps=1, seed=0)
    d = f.as_dict()
    assert set(d) == set(parent.as_dict()) | {"latent", "space"} and d["space"] == "pixel"
    assert d["latent"] == {"clean": st.as_dict(), "shifted": st.as_dict(), "uniformity_ratio": 1.0} and f.verdict(2.0) is True


def test_merge_entry_point_in_header_and_ctypes_table():
    from villandiffusion_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    m = re.search(r"int vd_image_set_merge\(([^)]*)\);", hdr)
    assert m, "vd_image_set_merge is not declared in include/villan_hip.h"
    assert "vd_image_set_merge" in lib.PROTOTYPES and len(lib.PROTOTYPES["vd_image_set_merge"][1]) == len(m.group(1).split(",")) == 9
    assert hasattr(lib.load(), "vd_image_set_merge") and callable(ops.image_set_merge)
    assert re.search(r"#define VD_ABI_VERSION 12\b", hdr) and lib.load().vd_abi_version() == 12


def test_refusals_fire_before_the_device_is_touched(monkeypatch):
    from villandiffusion_amd import defense_ldm, lib
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DDIMPipeline, LDMPipeline, ScoreSdeVePipeline

    def no_device():
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(lib, "require_device", no_device)
    z, p = torch.zeros(3, 8, 8), torch.zeros(3, 16, 16)
    pp = NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1,
                     down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                     up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), device="cpu")
    calls = {
        "invert_trigger": lambda pipe: defense_ldm.invert_trigger(pipe, steps=1, batch=1),
        "invert_trigger(pixel)": lambda pipe: defense_ldm.invert_trigger(pipe, space="pixel", steps=1, batch=1),
        "inversion_objective": lambda pipe: defense_ldm.inversion_objective(pipe, p, torch.zeros(1, 3, 8, 8), 999),
        "backdoor_features": lambda pipe: defense_ldm.backdoor_features(pipe, z, n=4, batch=2),
        "remove_backdoor": lambda pipe: defense_ldm.remove_backdoor(pipe, z, steps=1, batch=1, lr=1e-4),
        "encode_trigger": lambda pipe: defense_ldm.encode_trigger(pipe, p),
        "render_trigger": lambda pipe: defense_ldm.render_trigger(pipe, z),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=r"DDIMPipeline.*villandiffusion_amd\.defense / villandiffusion_amd\.mitigation"):
            call(DDIMPipeline(_unet(), S.DDIMScheduler()))
        with pytest.raises(NotImplementedError, match=r"NCSNppModel.*villandiffusion_amd\.defense_ve"):
            call(ScoreSdeVePipeline(pp, S.ScoreSdeVeScheduler()))
        with pytest.raises(NotImplementedError, match=r"NCSNppModel.*villandiffusion_amd\.defense_ve"):
            call(LDMPipeline(vqvae=_vq(), unet=pp, scheduler=S.DDIMScheduler()))
        with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
            call(_pipe(S.ScoreSdeVeScheduler()))
        with pytest.raises(NotImplementedError, match="object"):
            call(LDMPipeline(vqvae=object(), unet=_unet(), scheduler=S.DDIMScheduler()))
        with pytest.raises(TypeError):
            call(object())
    pipe = _pipe()
    bad = torch.zeros(3, 12, 12)                           # neither the latent nor the pixel shape
    for call in (lambda: defense_ldm.backdoor_features(pipe, bad, n=4, batch=2), lambda: defense_ldm.remove_backdoor(pipe, bad, steps=1, batch=1, lr=1e-4),
                 lambda: defense_ldm.trigger_space(pipe, bad), lambda: defense_ldm.encode_trigger(pipe, z), lambda: defense_ldm.render_trigger(pipe, p),
                 lambda: defense_ldm.inversion_objective(pipe, z, torch.zeros(1, 3, 8, 8), 999)):
        with pytest.raises(ValueError, match=r"\(3, 8, 8\)|\(3, 16, 16\)"):
            call()
    assert defense_ldm.trigger_space(pipe, z) == "latent" and defense_ldm.trigger_space(pipe, p) == "pixel"
    # the argument checks of the loops
    for kw in (dict(space="voxel", steps=1, batch=1), dict(space="pixel", steps=0, batch=1), dict(space="pixel", steps=1, batch=1, init=z),
               dict(space="pixel", steps=1, batch=1, clamp=(1.0, -1.0)), dict(space="pixel", steps=1, batch=1, noise=torch.zeros(1, 1, 3, 16, 16)),
               dict(space="pixel", steps=1, batch=1, timestep=1000), dict(space="pixel", steps=1, batch=1, lr=0.0)):
        with pytest.raises(ValueError):
            defense_ldm.invert_trigger(pipe, **kw)
    for kw in (dict(n=1, batch=2), dict(n=4, batch=0), dict(n=4, batch=2, num_inference_steps=0)):
        with pytest.raises(ValueError):
            defense_ldm.backdoor_features(pipe, z, **kw)
    for kw in (dict(steps=1, batch=1, lr=-1.0), dict(steps=1, batch=1, lr=1e-4, w_shift=-1.0), dict(steps=1, batch=1, lr=1e-4, timestep=-1)):
        with pytest.raises(ValueError):
            defense_ldm.remove_backdoor(pipe, p, **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_device():
    from villandiffusion_amd import defense_ldm, lib
    with pytest.raises(lib.VillanHipError):
        defense_ldm.invert_trigger(_pipe(), space="pixel", steps=1, batch=1)
    with pytest.raises(lib.VillanHipError):
        defense_ldm.ImageSetAccumulator((3, 8, 8), "cpu")


def test_tools_parse_space_and_describe_the_ldm_path():
    for tool, words in (("invert_trigger.py", ("--space", "{latent,pixel}", "trigger_inv.png", "defense_ldm")),
                        ("detect_backdoor.py", ("defense_ldm", '"latent"', '"space"')), ("remove_backdoor.py", ("defense_ldm", '"space"'))):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-1000:]
        for w in words:
            assert w in run.stdout, (tool, w)
    assert "out of scope" not in open(os.path.join(ROOT, "tools", "detect_backdoor.py")).read()
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "invert_trigger.py"), "--ckpt", ROOT, "--space", "voxel"], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "invalid choice" in bad.stderr
    # --space pixel needs a vqvae/ folder: refused by the parser, before anything is loaded
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "invert_trigger.py"), "--ckpt", ROOT, "--space", "pixel"], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "vqvae" in bad.stderr
