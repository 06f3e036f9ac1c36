"""villandiffusion_amd.defense_ve without a GPU: the public names, the two new entry points in the header and the ctypes table, every refusal
and argument check before the device is touched, no fallback and the tools' --help.  (The per-instance input-gradient switch: tests/test_flat_layout_cpu.py.)"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1,
             down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
             up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))


def _pp():
    from villandiffusion_amd.ncsnpp import NCSNppModel
    return NCSNppModel(**SMALL, device="cpu")


def _unet():
    from villandiffusion_amd.unet import UNet2DModel
    return UNet2DModel(sample_size=16, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                       down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"), device="cpu")


def test_public_names_and_entry_points():
    from villandiffusion_amd import defense, defense_ve, lib, mitigation, ops
    assert defense_ve.__all__ == ["inversion_objective", "invert_trigger", "backdoor_features", "removal_objective", "remove_backdoor"]
    # reused, not copied
    assert defense_ve.TriggerInversion is defense.TriggerInversion and defense_ve._frozen is defense._frozen
    assert defense_ve.adam_update is defense.adam_update and defense_ve._removal_into is mitigation._removal_into
    assert defense_ve._frozen_copy is mitigation._frozen_copy and defense_ve.image_set_stats is mitigation.image_set_stats
    assert defense_ve.BackdoorFeatures is mitigation.BackdoorFeatures and defense_ve.BackdoorRemoval is mitigation.BackdoorRemoval
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    for name, n_args in (("vd_score_inv_objective", 12), ("vd_pyramid_dgrad", 12)):
        assert f"int {name}(" in hdr
        assert name in lib.PROTOTYPES and len(lib.PROTOTYPES[name][1]) == n_args
        assert hasattr(lib.load(), name)
    assert "#define VD_ABI_VERSION 12" in hdr and lib.load().vd_abi_version() == 12
    assert callable(ops.score_inv_objective) and callable(ops.pyramid_dgrad)


def test_shared_loops_and_checks_are_reused_not_copied():
    from villandiffusion_amd import defense, defense_ve, mitigation
    for name in ("_noise_of", "_check_loop_args", "_shape", "_trainable", "_objective_into", "_run_inversion"):
        assert getattr(defense_ve, name) is getattr(defense, name), name
    for name in ("_removal_step", "_run_removal", "_check_removal_args", "_check_feature_args"):
        assert getattr(defense_ve, name) is getattr(mitigation, name), name
    assert mitigation._noise_of is defense._noise_of


def test_sigma_comes_from_the_training_table_not_from_an_inference_table():
    from villandiffusion_amd import defense_ve
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.loss import LossFn
    for smax in (50.0, 380.0, 1348.0):
        sched = S.ScoreSdeVeScheduler(sigma_max=smax)
        captured = LossFn(sched, "SDE-VE", psi=0)._sigmas_asc                  # what training reads
        sched.set_timesteps(7)
        sched.set_sigmas(7)                                                   # what a pipeline call leaves behind
        tab = defense_ve._training_sigmas(sched)
        assert torch.equal(tab, captured) and len(sched.sigmas) == 7
        T, sigma = defense_ve._sigma_at(sched, None, "x")
        assert T == 1999 and sigma == float(captured.max()) and abs(sigma - smax) <= 1e-4 * smax
        assert defense_ve._sigma_at(sched, 0, "x")[1] == float(captured[0])
        with pytest.raises(ValueError):
            defense_ve._sigma_at(sched, 2000, "x")


def test_everything_is_validated_before_the_device_is_touched(monkeypatch):
    from villandiffusion_amd import defense_ve as D
    from villandiffusion_amd import lib
    from villandiffusion_amd import pipelines as P
    from villandiffusion_amd import schedulers as S
    monkeypatch.setattr(lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device touched before validation")))
    pp, sched = _pp(), S.ScoreSdeVeScheduler()
    tau, eps = torch.zeros(3, 16, 16), torch.zeros(2, 3, 16, 16)
    flags = [p.requires_grad for p in pp.parameters()]
    # ---- invert_trigger
    for bad in (dict(steps=0, batch=4), dict(steps=2.5, batch=4), dict(steps=True, batch=4), dict(steps=2, batch=0), dict(steps=2, batch="4"),
                dict(steps=2, batch=4, lam=float("nan")), dict(steps=2, batch=4, lam=float("inf")), dict(steps=2, batch=4, lr=0.0),
                dict(steps=2, batch=4, noise=torch.zeros(2, 4, 3, 8, 8)), dict(steps=2, batch=4, noise=torch.zeros(3, 4, 3, 16, 16)),
                dict(steps=2, batch=4, init=torch.zeros(3, 8, 8)), dict(steps=2, batch=4, timestep=2000), dict(steps=2, batch=4, timestep=-1)):
        with pytest.raises(ValueError):
            D.invert_trigger(pp, sched, **bad)
    with pytest.raises(TypeError):
        D.invert_trigger(pp, sched, steps=2, batch=4, noise=3)
    with pytest.raises(TypeError):
        D.invert_trigger(torch.nn.Linear(2, 2), sched, steps=2, batch=4)
    with pytest.raises(NotImplementedError, match="defense"):
        D.invert_trigger(_unet(), S.DDPMScheduler(), steps=2, batch=4)
    with pytest.raises(NotImplementedError, match="KarrasVeScheduler"):
        D.invert_trigger(pp, S.KarrasVeScheduler(), steps=2, batch=4)
    with pytest.raises(NotImplementedError, match="DDPMScheduler"):
        D.invert_trigger(pp, S.DDPMScheduler(), steps=2, batch=4)
    for mode in ("f16", "bf16"):
        pp.conv_math = mode
        try:
            for call in (lambda: D.invert_trigger(pp, sched, steps=2, batch=4), lambda: D.inversion_objective(pp, tau, eps, 380.0),
                         lambda: D.remove_backdoor(pp, sched, tau, steps=1, batch=1, lr=1e-4), lambda: D.removal_objective(pp, pp, tau, eps, 380.0),
                         lambda: D.backdoor_features(P.ScoreSdeVePipeline(pp, sched), tau, n=4, batch=2)):
                with pytest.raises(NotImplementedError, match=mode):
                    call()
        finally:
            pp.conv_math = "bf16x3"
    # ---- inversion_objective / removal_objective
    for fn in (lambda **k: D.inversion_objective(pp, **k), lambda **k: D.removal_objective(pp, pp, **k)):
        with pytest.raises(ValueError):
            fn(tau=torch.zeros(3, 8, 8), eps=eps, sigma=380.0)
        with pytest.raises(ValueError):
            fn(tau=tau, eps=eps[0], sigma=380.0)
        for bad in (0.0, -1.0, float("nan"), float("inf"), torch.tensor([1.0, 2.0])):
            with pytest.raises(ValueError):
                fn(tau=tau, eps=eps, sigma=bad)
    with pytest.raises(NotImplementedError, match="mitigation"):
        D.inversion_objective(_unet(), tau, eps, 380.0)
    with pytest.raises(NotImplementedError, match="mitigation"):
        D.removal_objective(pp, _unet(), tau, eps, 380.0)
    # ---- remove_backdoor
    for bad in (dict(steps=0, batch=4, lr=1e-4), dict(steps=2, batch=0, lr=1e-4), dict(steps=2, batch=4, lr=0.0), dict(steps=2, batch=4, lr=float("inf")),
                dict(steps=2, batch=4, lr=1e-4, w_clean=-1.0), dict(steps=2, batch=4, lr=1e-4, w_shift=float("inf")),
                dict(steps=2, batch=4, lr=1e-4, max_grad_norm=0.0), dict(steps=2, batch=4, lr=1e-4, timestep=2000),
                dict(steps=2, batch=4, lr=1e-4, noise=torch.zeros(2, 4, 3, 8, 8))):
        with pytest.raises(ValueError):
            D.remove_backdoor(pp, sched, tau, **bad)
    with pytest.raises(ValueError):
        D.remove_backdoor(pp, sched, torch.zeros(3, 8, 8), steps=2, batch=4, lr=1e-4)
    with pytest.raises(TypeError):
        D.remove_backdoor(pp, sched, tau, steps=2, batch=4, lr=1e-4, noise=3)
    with pytest.raises(NotImplementedError, match="mitigation"):
        D.remove_backdoor(_unet(), S.DDPMScheduler(), tau, steps=2, batch=4, lr=1e-4)
    with pytest.raises(NotImplementedError, match="KarrasVeScheduler"):
        D.remove_backdoor(pp, S.KarrasVeScheduler(), tau, steps=2, batch=4, lr=1e-4)
    # ---- backdoor_features
    pipe = P.ScoreSdeVePipeline(pp, sched)
    for bad in (dict(n=1, batch=2), dict(n=4, batch=0), dict(n=4.0, batch=2), dict(n=4, batch=2, num_inference_steps=0)):
        with pytest.raises(ValueError):
            D.backdoor_features(pipe, tau, **bad)
    with pytest.raises(ValueError):
        D.backdoor_features(pipe, torch.zeros(3, 8, 8), n=4, batch=2)
    with pytest.raises(TypeError):
        D.backdoor_features(object(), tau, n=4, batch=2)
    with pytest.raises(NotImplementedError, match="DDIMPipeline"):
        D.backdoor_features(P.DDIMPipeline(_unet(), S.DDIMScheduler()), tau, n=4, batch=2)
    with pytest.raises(NotImplementedError, match="KarrasVePipeline"):
        D.backdoor_features(P.KarrasVePipeline(pp, S.KarrasVeScheduler()), tau, n=4, batch=2)
    with pytest.raises(NotImplementedError, match="mitigation"):
        D.backdoor_features(P.ScoreSdeVePipeline(_unet(), sched), tau, n=4, batch=2)
    assert [p.requires_grad for p in pp.parameters()] == flags and pp._input_grad is False and not pp.time_proj.weight.requires_grad


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_gpu():
    from villandiffusion_amd import defense_ve as D
    from villandiffusion_amd import lib
    from villandiffusion_amd import pipelines as P
    from villandiffusion_amd import schedulers as S
    pp, sched = _pp(), S.ScoreSdeVeScheduler()
    tau, eps = torch.zeros(3, 16, 16), torch.zeros(1, 3, 16, 16)
    flags = [p.requires_grad for p in pp.parameters()]
    for call in (lambda: D.invert_trigger(pp, sched, steps=1, batch=1), lambda: D.inversion_objective(pp, tau, eps, 380.0),
                 lambda: D.remove_backdoor(pp, sched, tau, steps=1, batch=1, lr=1e-4), lambda: D.removal_objective(pp, pp, tau, eps, 380.0),
                 lambda: D.backdoor_features(P.ScoreSdeVePipeline(pp, sched), tau, n=2, batch=2)):
        with pytest.raises(lib.VillanHipError):
            call()
    assert [p.requires_grad for p in pp.parameters()] == flags and pp._input_grad is False


@pytest.mark.parametrize("tool,flags", [("invert_trigger.py", ("--ckpt", "--steps", "--batch", "--lam", "--lr", "--seed", "--timestep", "--out")),
                                        ("detect_backdoor.py", ("--ckpt", "--trigger", "--n", "--batch", "--steps", "--seed", "--threshold", "--out")),
                                        ("remove_backdoor.py", ("--ckpt", "--trigger", "--steps", "--batch", "--lr", "--w-clean", "--w-shift", "--out")),
                                        ("ve_defense_ab.py", ("--alternations", "--batch", "--out"))])
def test_tool_help_exits_zero_and_names_the_ve_path(tool, flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in flags:
        assert flag in out.stdout, flag
    assert "defense_ve" in out.stdout
