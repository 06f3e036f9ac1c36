"""EMA of the weights without a GPU: the decay schedule (diffusers ``EMAModel.get_decay``, restated in trainer.ema_decay_at) against known answers,
and the ``unet_ema/`` folder of the diffusers on-disk layout (written only when asked for, read by ``from_pretrained(..., use_ema=True)``)."""
import filecmp
import json
import os

import pytest
import torch

from villandiffusion_amd.pipelines import EMA_CONFIG_KEYS, DDPMPipeline
from villandiffusion_amd.schedulers import DDPMScheduler
from villandiffusion_amd.trainer import EMAConfig, ema_decay_at, ema_one_minus_decay
from villandiffusion_amd.unet import UNet2DModel

SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))


def test_ema_decay_known_answers():
    cfg = EMAConfig()
    assert (cfg.decay, cfg.min_decay, cfg.update_after_step, cfg.use_ema_warmup, cfg.inv_gamma, cfg.power) == (0.9999, 0.0, 0, False, 1.0, 2 / 3)
    assert ema_decay_at(1, cfg) == 0.0                                   # the first update copies the parameters
    assert ema_decay_at(2, cfg) == 2 / 11
    assert ema_decay_at(3, cfg) == 3 / 12
    assert ema_decay_at(10 ** 6, cfg) == 0.9999                          # (1 + n) / (10 + n) -> 1: capped
    assert ema_decay_at(1000, cfg) == 1000 / 1009 < 0.9999
    # min_decay: a floor under the ramp, but not under the n <= 0 rule
    floor = EMAConfig(decay=0.999, min_decay=0.5)
    assert ema_decay_at(1, floor) == 0.0 and ema_decay_at(2, floor) == 0.5 and ema_decay_at(10, floor) == 10 / 19 and ema_decay_at(10 ** 6, floor) == 0.999
    # update_after_step: n counts from there
    late = EMAConfig(update_after_step=5)
    assert [ema_decay_at(k, late) for k in range(0, 7)] == [0.0] * 7 and ema_decay_at(7, late) == 2 / 11 and ema_decay_at(8, late) == 3 / 12
    # warm-up form at inv_gamma = 1, power = 2/3: 1 - (1 + n) ** (-2/3)
    warm = EMAConfig(use_ema_warmup=True)
    assert ema_decay_at(1, warm) == 0.0
    assert ema_decay_at(2, warm) == 1 - 2 ** (-2 / 3) and abs(ema_decay_at(2, warm) - 0.3700394750525634) < 1e-15
    assert ema_decay_at(8, warm) == 1 - 8 ** (-2 / 3) and abs(ema_decay_at(8, warm) - 0.75) < 1e-15
    assert ema_decay_at(10 ** 9, warm) == 0.9999
    assert ema_decay_at(28, EMAConfig(use_ema_warmup=True, inv_gamma=3.0, power=1.0, decay=1.0)) == 1 - 1 / 10       # 1 - (1 + 27/3) ** -1
    # what the kernel receives: 1 - d, rounded once to a C float
    assert ema_one_minus_decay(1, cfg) == 1.0
    assert ema_one_minus_decay(2, cfg) == float(torch.tensor(9 / 11, dtype=torch.float64).to(torch.float32))
    assert ema_one_minus_decay(10 ** 6, cfg) == float(torch.tensor(1 - 0.9999, dtype=torch.float64).to(torch.float32))


def _files(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def test_unet_ema_folder_round_trip(tmp_path):
    net = UNet2DModel(**SMALL, device="cpu")
    net.reset_parameters(seed=2)
    pipe = DDPMPipeline(net, DDPMScheduler())
    gen = torch.Generator().manual_seed(9)
    shadow = net.flat_param.detach().clone() + 0.01 * torch.randn(net.flat_numel, generator=gen)
    cfg = EMAConfig(decay=0.999, min_decay=0.1, update_after_step=2, use_ema_warmup=True, inv_gamma=2.0, power=0.75)
    plain, with_ema = str(tmp_path / "plain"), str(tmp_path / "ema")
    pipe.save_pretrained(plain)
    pipe.save_pretrained(with_ema, ema=(shadow, cfg, 17))
    # unet_ema/ only when asked for; everything else byte for byte what a save without EMA writes
    assert not os.path.exists(os.path.join(plain, "unet_ema"))
    assert _files(with_ema) == sorted(_files(plain) + ["unet_ema/config.json", "unet_ema/diffusion_pytorch_model.safetensors"])
    for f in _files(plain):
        assert filecmp.cmp(os.path.join(plain, f), os.path.join(with_ema, f), shallow=False), f
    assert "unet_ema" not in json.load(open(os.path.join(with_ema, "model_index.json")))
    # its config: the network's own plus the seven EMA keys
    ucfg = json.load(open(os.path.join(with_ema, "unet", "config.json")))
    ecfg = json.load(open(os.path.join(with_ema, "unet_ema", "config.json")))
    assert set(ecfg) - set(ucfg) == set(EMA_CONFIG_KEYS) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup",
                                                             "inv_gamma", "power"}
    assert {k: ecfg[k] for k in ucfg} == ucfg
    assert {k: ecfg[k] for k in EMA_CONFIG_KEYS} == {"decay": 0.999, "min_decay": 0.1, "optimization_step": 17, "update_after_step": 2,
                                                     "use_ema_warmup": True, "inv_gamma": 2.0, "power": 0.75}
    # use_ema=True: the shadow's weights; default: the raw ones
    raw = DDPMPipeline.from_pretrained(with_ema).unet
    ema = DDPMPipeline.from_pretrained(with_ema, use_ema=True).unet
    assert set(ema._offs) == set(net._offs)
    for name, (off, n, shape) in net._offs.items():
        assert torch.equal(raw.P[name].cpu(), net.P[name]), name
        assert torch.equal(ema.P[name].cpu(), shadow[off:off + n].view(shape)), name
    assert not torch.equal(ema.flat_param.cpu(), raw.flat_param.cpu())
    # a folder without unet_ema/ cannot give EMA weights
    with pytest.raises(FileNotFoundError, match="unet_ema"):
        DDPMPipeline.from_pretrained(plain, use_ema=True)


def test_cli_flags_and_side_files(tmp_path):
    """--ema_decay / --use_ema parse, map onto TrainingConfig fields, and at their defaults stay out of the JSON side files."""
    import VillanDiffusion as V
    a = V.parse_args(["--mode", "train", "--ema_decay", "0.999"])
    assert a.ema_decay == 0.999 and a.use_ema is False
    assert V.parse_args(["--mode", "sampling", "--use_ema"]).use_ema is True and V.parse_args(["--mode", "train"]).ema_decay is None
    c = V.TrainingConfig()
    assert c.ema_decay is None and c.use_ema is False
    base = ["--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--ckpt", "DDPM-32-DEFAULT", "-o"]
    off = V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "off")] + base))
    on = V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "on"), "--ema_decay", "0.999"] + base))
    assert off.ema_decay is None and on.ema_decay == 0.999
    for f in ("args.json", "config.json"):
        d_off, d_on = json.load(open(os.path.join(off.output_dir, f))), json.load(open(os.path.join(on.output_dir, f)))
        assert "ema_decay" not in d_off and "use_ema" not in d_off and "use_ema" not in d_on and d_on["ema_decay"] == 0.999, f
    # resume takes the decay from args.json; sampling accepts --use_ema, training does not
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", on.output_dir])).ema_decay == 0.999
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", off.output_dir])).ema_decay is None
    assert V.setup(V.parse_args(["--mode", "sampling", "--ckpt", on.output_dir, "--use_ema"])).use_ema is True
    assert V.setup(V.parse_args(["--mode", "sampling", "--ckpt", on.output_dir])).use_ema is False
    with pytest.raises(NotImplementedError):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--use_ema"] + base))
    with pytest.raises(NotImplementedError):
        V.setup(V.parse_args(["--mode", "sampling", "--ckpt", on.output_dir, "--ema_decay", "0.5"]))
