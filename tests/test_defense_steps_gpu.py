"""The per-iteration calls the A/B tools time (tools/ve_defense_ab.py, tools/removal_step_ab.py) are the library's own: driving
`defense._objective_into` + `adam_update` and `mitigation._removal_step` by hand for two iterations gives, bit for bit, what `invert_trigger` and
`remove_backdoor` give for steps=2 -- for VP (`defense` / `mitigation`, a small UNet2DModel) and for SDE-VE (`defense_ve`, a small NCSN++)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from villandiffusion_amd import defense, defense_ve, mitigation  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402
from villandiffusion_amd.pipelines import sampler_forward  # noqa: E402
from villandiffusion_amd.trainer import FusedAdam  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"
STEPS, B, SEED, LAM, LR_INV, LR_FIX = 2, 4, 2, 0.5, 0.1, 1e-4
UNET = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))      # test_mitigation_gpu.py::SMALL
NCSNPP = dict(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1,
              down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
              up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))                                 # test_defense_ve_cpu.py::SMALL


def _family(name):
    """(a factory of identical fresh networks, the scheduler, the module pair, the noise level as `t`, sigma or None)"""
    if name == "vp":
        cls, cfg, sched, sigma = UNet2DModel, UNET, S.DDPMScheduler(), None
    else:
        cls, cfg, sched = NCSNppModel, NCSNPP, S.ScoreSdeVeScheduler(num_train_timesteps=2000, sigma_min=0.01, sigma_max=380.0, snr=0.075)
        sigma = defense_ve._sigma_at(sched, None, "test")[1]

    def fresh():
        net = cls(**cfg)
        net.reset_parameters(seed=1)
        return net
    return fresh, sched, sigma


@pytest.mark.parametrize("family", ["vp", "ve"])
def test_hand_driven_inversion_iterations_are_invert_triggers(family):
    fresh, sched, sigma = _family(family)
    net = fresh()
    shape = (3,) + (net.sample_size,) * 2
    noise = torch.randn((STEPS, B) + shape, generator=torch.Generator().manual_seed(7))
    lib_run = (defense if sigma is None else defense_ve).invert_trigger(net, sched, steps=STEPS, batch=B, lam=LAM, lr=LR_INV, seed=SEED, noise=noise)

    tau = torch.rand(shape, generator=torch.Generator().manual_seed(SEED)).to(DEV)                  # the default start: U[0, 1) from `seed`
    m, v, dtau = torch.zeros_like(tau), torch.zeros_like(tau), torch.empty_like(tau)
    losses, partial = torch.zeros(STEPS, device=DEV), torch.empty(1024, device=DEV)
    t = torch.full((B,), 999, device=DEV) if sigma is None else torch.full((B,), sigma, device=DEV)
    with defense._frozen(net), net.input_gradients():
        for it in range(STEPS):
            defense._objective_into(net, tau, noise[it].to(DEV), t, LAM, losses[it:it + 1], dtau, partial, sigma)
            defense.adam_update(tau, dtau, m, v, it + 1, LR_INV)
    print(f"[steps] {family} inversion losses {lib_run.losses}")
    assert all(math.isfinite(x) for x in lib_run.losses) and lib_run.losses[0] != lib_run.losses[1]
    assert torch.equal(tau, lib_run.trigger) and torch.equal(losses.cpu(), torch.tensor(lib_run.losses))


@pytest.mark.parametrize("family", ["vp", "ve"])
def test_hand_driven_removal_steps_are_remove_backdoors(family):
    fresh, sched, sigma = _family(family)
    net, twin = fresh(), fresh()
    shape = (3,) + (net.sample_size,) * 2
    gen = torch.Generator().manual_seed(7)
    noise = torch.randn((STEPS, B) + shape, generator=gen)
    trigger = torch.rand(shape, generator=gen)
    lib_run = (mitigation if sigma is None else defense_ve).remove_backdoor(net, sched, trigger, steps=STEPS, batch=B, lr=LR_FIX, seed=SEED,
                                                                            noise=noise)

    s2 = 1.0 if sigma is None else sigma * sigma
    prepare = (lambda x: x) if sigma is None else (lambda x: defense_ve._scaled(x, sigma))
    tau = prepare(trigger.to(DEV))
    frozen = mitigation._frozen_copy(twin)
    opt = FusedAdam(twin, LR_FIX, max_grad_norm=1.0)
    curves, partial = torch.zeros((STEPS, 3), device=DEV), torch.empty(2048, device=DEV)
    t2 = torch.full((2 * B,), 999.0 if sigma is None else sigma, device=DEV)
    with defense._trainable(twin, skip=() if sigma is None else (twin.time_proj.weight,)):
        teacher = sampler_forward(frozen, B) if sigma is None else defense_ve._teacher(frozen)
        twin.zero_grad()
        for it in range(STEPS):
            mitigation._removal_step(twin, teacher, opt, tau, prepare(noise[it].to(DEV)), t2, 1.0 * s2, 1.0 * s2, curves[it], partial)
    host = curves.cpu().tolist()
    want = ([r[0] for r in host], [r[1] * s2 for r in host], [r[2] * s2 for r in host]) if sigma is not None else tuple(zip(*host))
    print(f"[steps] {family} removal total {lib_run.total}, shift {lib_run.shift}")
    assert all(math.isfinite(x) for x in lib_run.total) and not torch.equal(net.flat_param, lib_run.frozen.flat_param)
    assert torch.equal(twin.flat_param, net.flat_param)
    for got, exp in zip((lib_run.total, lib_run.clean, lib_run.shift), want):
        assert torch.equal(torch.tensor(got, dtype=torch.float64), torch.tensor(list(exp), dtype=torch.float64))
    assert lib_run.sigma == sigma
