"""LoRA fine-tuning (villandiffusion_amd.lora) without a GPU: the adapter table on the small and the full-size networks, the configuration checks,
tests/lora_ref.py against itself (autograd through W0 + s B A vs the closed forms in float64), the adapter's save / load round trip on the host,
the C ABI, and the command-line flags."""
import json
import os
import re

import pytest
import torch

import lora_ref
from oracle.unet_ref import UNet2DModelRef
from villandiffusion_amd import lib, lora, ops
from villandiffusion_amd.lora import LoRAAdapter, LoRAConfig, adapter_table
from villandiffusion_amd.model import LDM_CELEBA_UNET_ARCH, NCSNPP_32_ARCH
from villandiffusion_amd.ncsnpp import NCSNppModel
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_anp_gpu.py's
SMALL_PP = dict(sample_size=16, block_out_channels=(32, 64, 64), down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=1)            # anp_families_ref.py's
ATTN = re.compile(r"^(.*attentions\.\d+)\.(to_q|to_k|to_v|to_out\.0)\.weight$")


@pytest.fixture(scope="module")
def nets():
    return {"small": UNet2DModel(**SMALL, device="cpu"), "small_pp": NCSNppModel(**SMALL_PP, device="cpu"),
            "cifar10": UNet2DModel(device="cpu"), "ldm": UNet2DModel(**LDM_CELEBA_UNET_ARCH, device="cpu"),
            "ncsnpp": NCSNppModel(**NCSNPP_32_ARCH, sample_size=32, device="cpu")}


def _want(net, target, r):
    """The issue's selection rule on the network's own layout: (adapted names, skipped names)."""
    adapted, skipped = [], []
    for name, shape, _ in net._layout:
        if target == "attn":
            ok = len(shape) >= 2 and ATTN.match(name) is not None
        elif target == "conv":
            ok = len(shape) == 4 and name.endswith(".weight")
        else:
            ok = len(shape) >= 2
        if ok:
            M = shape[0]
            n = 1
            for d in shape:
                n *= d
            (skipped if min(M, n // M) <= r else adapted).append(name)
    return adapted, skipped


@pytest.mark.parametrize("which", ["small", "small_pp", "cifar10", "ldm", "ncsnpp"])
@pytest.mark.parametrize("target", ["attn", "conv", "all"])
def test_adapter_table(nets, which, target):
    net, r = nets[which], 4
    tab = adapter_table(net, LoRAConfig(r=r, target=target))
    adapted, skipped = _want(net, target, r)
    assert list(tab.slices) == adapted and tab.skipped == skipped and tab.n_jobs == len(adapted) > 0
    assert tab.r == r and tab.s == 1.0 and tab.target == target
    cursor = rb = cb = 0
    for (off, M, L, aoff, boff, b0, c0), name in zip(tab.jobs, adapted):
        woff, n, shape = net._offs[name]
        assert (off, M, M * L) == (woff, shape[0], n) and min(M, L) > r
        assert aoff % 4 == 0 and boff % 4 == 0 and aoff == cursor and boff == aoff + (r * L + 3) // 4 * 4       # A, then B, each at a multiple of 4
        a, b = tab.slices[name]
        assert (a.start, a.stop, b.start, b.stop) == (aoff, aoff + r * L, boff, boff + M * r)
        assert (b0, c0) == (rb, cb)
        cursor = boff + (M * r + 3) // 4 * 4
        rb += (M + 3) // 4
        cb += (L + 255) // 256
    assert tab.numel == cursor and (tab.row_blocks, tab.col_blocks) == (rb, cb)
    assert tab.adapter_floats == sum(r * (j[1] + j[2]) for j in tab.jobs) <= tab.numel < tab.adapter_floats + 8 * tab.n_jobs
    assert int(tab.padding_mask().sum()) == tab.numel - tab.adapter_floats
    assert tab.weight_floats == sum(net._offs[n][1] for n in adapted) and tab.extent <= net.flat_numel
    # 1-d parameters, biases and GroupNorm parameters are never layers
    assert all(len(net._offs[n][2]) >= 2 for n in adapted)
    if target == "attn":                                   # exactly the four projections of every attention block
        blocks = {}
        for name in adapted:
            m = ATTN.match(name)
            assert m, name
            blocks.setdefault(m.group(1), []).append(m.group(2))
        n_attn = len({n.rsplit(".", 2)[0] for n in net._offs if ".attentions." in n and n.endswith("to_q.weight")})
        assert len(blocks) == n_attn > 0 and all(sorted(v) == ["to_k", "to_out.0", "to_q", "to_v"] for v in blocks.values())
        assert skipped == []
    else:
        assert "conv_out.weight" in skipped and "conv_in.weight" in adapted          # 3 rows <= 4; 27 floats a row > 4
        if which in ("small_pp", "ncsnpp"):               # the image pyramid: 3-row heads going up, 3-float rows going down
            pyramid = [n for n in net._offs if n.endswith(".skip_conv.weight")]
            assert pyramid and all(n in skipped for n in pyramid if min(net._offs[n][2][0], net._offs[n][1] // net._offs[n][2][0]) <= r)
            assert any(n.startswith("up_blocks.") for n in skipped) and "time_proj.weight" not in adapted and "time_proj.weight" not in skipped
    if target == "all":
        assert set(adapter_table(net, LoRAConfig(r=r, target="conv")).slices) < set(adapted)
        assert set(adapter_table(net, LoRAConfig(r=r, target="attn")).slices) < set(adapted)


def test_known_counts_of_the_cifar10_unet(nets):
    """The CIFAR10 UNet has two attention blocks per level with attention (down 2, up 3) and one in the middle."""
    tab = adapter_table(nets["cifar10"], LoRAConfig(r=4, target="attn"))
    assert tab.n_jobs == 4 * 6 and tab.weight_floats == 24 * 256 * 256 and tab.adapter_floats == 24 * 4 * 512 == tab.numel
    # a higher rank skips more: at r = 32 nothing of a 27-float-row conv_in is left
    t32 = adapter_table(nets["cifar10"], LoRAConfig(r=32, target="conv"))
    assert "conv_in.weight" in t32.skipped and "conv_out.weight" in t32.skipped


def test_config_validation(nets):
    for bad in (0, 33, -1, 4.0, True, None):
        with pytest.raises(ValueError, match="r must be"):
            LoRAConfig(r=bad)
    with pytest.raises(ValueError, match="target"):
        LoRAConfig(r=4, target="linear")
    for bad in (0, -1.0, float("nan"), "8"):
        with pytest.raises(ValueError, match="alpha"):
            LoRAConfig(r=4, alpha=bad)
    assert LoRAConfig(r=4).s == 1.0 and LoRAConfig(r=4).lora_alpha == 4.0 and LoRAConfig(r=4, alpha=8).s == 2.0 and LoRAConfig(r=1).target == "attn"
    assert LoRAConfig(r=32).r == 32
    with pytest.raises(TypeError):
        adapter_table(nets["small"], dict(r=4))
    with pytest.raises(TypeError):
        adapter_table(torch.nn.Linear(3, 3), LoRAConfig(r=4))
    with pytest.raises(ValueError, match="no jobs|rank"):
        lora.AdapterTable([], {}, 0, 4)
    with pytest.raises(ValueError, match="job 0"):
        lora.AdapterTable([(0, 8, 8, 2, 32, 0, 0)], {}, 64, 4)            # A off a multiple of 4
    with pytest.raises(ValueError, match="overlap"):
        lora.AdapterTable([(0, 8, 8, 0, 16, 0, 0)], {}, 64, 4)            # B inside A


def test_reference_autograd_equals_its_closed_forms_in_float64():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**SMALL).double()
    tab = adapter_table(UNet2DModel(**SMALL, device="cpu"), LoRAConfig(r=4, alpha=8.0, target="all"))
    assert lora_ref.selected(ref, "all", 4)[1] == ["conv_out.weight"] and sorted(lora_ref.selected(ref, "all", 4)[0]) == sorted(tab.slices)
    gen = torch.Generator().manual_seed(1)
    params = dict(ref.named_parameters())
    ad = {}
    for name in tab.slices:
        M = params[name].shape[0]
        L = params[name].numel() // M
        ad[name] = (torch.randn(4, L, generator=gen, dtype=torch.float64) * L ** -0.5, torch.randn(M, 4, generator=gen, dtype=torch.float64) * 0.1)
    x = torch.randn(2, 3, 32, 32, generator=gen, dtype=torch.float64)
    w = torch.randn(2, 3, 32, 32, generator=gen, dtype=torch.float64)
    gab, gw, _ = lora_ref.autograd_grads(ref, ad, tab.s, x, torch.tensor([3, 870]), w)
    worst = 0.0
    for name, (A, B) in ad.items():
        dA, dB = lora_ref.grads(gw[name], A, B, tab.s)
        for got, want in ((gab[name][0], dA), (gab[name][1], dB)):
            assert float(want.abs().max()) > 0
            worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    print(f"[lora_ref] autograd vs closed forms, float64: worst {worst:.2e}")
    assert worst < 1e-12
    # the merged weight, and the flat layout and back
    name = next(iter(ad))
    w0 = params[name].detach().reshape(params[name].shape[0], -1)
    assert torch.equal(lora_ref.merged(w0, *ad[name], tab.s), w0 + tab.s * (ad[name][1] @ ad[name][0]))
    flat = lora_ref.flat_of(ad, tab.slices, tab.numel)
    back = lora_ref.adapters_of(flat, tab.slices, tab.shapes, 4)
    assert all(torch.equal(back[n][0], ad[n][0]) and torch.equal(back[n][1], ad[n][1]) for n in ad)
    assert float(flat[tab.padding_mask()].abs().sum()) == 0.0


def test_initialisation_and_host_round_trip(tmp_path, nets):
    from safetensors.torch import load_file
    net = UNet2DModel(**SMALL, device="cpu")
    net.reset_parameters(seed=5)
    cfg = LoRAConfig(r=4, alpha=8.0, target="all", seed=11)
    ad = LoRAAdapter(net, cfg)
    tab = ad.table
    assert torch.equal(ad.base, net.flat_param) and ad.base.data_ptr() != net.flat_param.data_ptr()
    assert ad.param.numel() == ad.grad.numel() == tab.numel and float(ad.grad.abs().sum()) == 0.0
    want = lora_ref.init_adapters(UNet2DModelRef(**SMALL), list(tab.slices), 4, 11)          # U(+-1/sqrt(L)) in table order, B = 0
    assert torch.equal(ad.param, lora_ref.flat_of(want, tab.slices, tab.numel))
    for name, (a, b) in tab.slices.items():
        L = tab.shapes[name] and net._offs[name][1] // tab.shapes[name][0]
        assert float(ad.param[a].abs().max()) <= L ** -0.5 and float(ad.param[a].abs().max()) > 0.5 * L ** -0.5 and float(ad.param[b].abs().max()) == 0.0
    with torch.no_grad():
        ad.param.copy_(torch.randn(tab.numel, generator=torch.Generator().manual_seed(2)))
        ad.param[tab.padding_mask()] = 0.0
    sd = ad.state_dict()
    assert len(sd) == 2 * tab.n_jobs
    assert tuple(sd["conv_in.lora_A.weight"].shape) == (4, 3, 3, 3) and tuple(sd["conv_in.lora_B.weight"].shape) == (32, 4, 1, 1)
    q = "mid_block.attentions.0.to_q"
    assert tuple(sd[q + ".lora_A.weight"].shape) == (4, 64) and tuple(sd[q + ".lora_B.weight"].shape) == (64, 4)
    ad.save(str(tmp_path / "ad"))
    assert sorted(os.listdir(tmp_path / "ad")) == ["adapter_config.json", "adapter_model.safetensors"]
    c = json.load(open(tmp_path / "ad" / "adapter_config.json"))
    assert (c["peft_type"], c["r"], c["lora_alpha"], c["bias"], c["target"]) == ("LORA", 4, 8.0, "none", "all")
    assert "to_q" in c["target_modules"] and "to_out.0" in c["target_modules"] and "conv1" in c["target_modules"]
    on_disk = load_file(str(tmp_path / "ad" / "adapter_model.safetensors"))
    assert set(on_disk) == set(sd) and all(torch.equal(on_disk[k], sd[k]) for k in sd)
    twin = UNet2DModel(**SMALL, device="cpu")
    twin.reset_parameters(seed=6)                                               # another base: the adapter is portable
    back = LoRAAdapter.load(twin, str(tmp_path / "ad"))
    assert torch.equal(back.param, ad.param) and back.cfg == cfg and torch.equal(back.base, twin.flat_param)
    assert float(back.param[tab.padding_mask()].abs().sum()) == 0.0
    # a network whose layers differ: ValueError naming the first mismatch
    other = UNet2DModel(**dict(SMALL, block_out_channels=(32, 96)), device="cpu")
    with pytest.raises(ValueError, match=r"lora_[AB]\.weight is \("):
        LoRAAdapter.load(other, str(tmp_path / "ad"))
    with pytest.raises(ValueError, match="holds no"):
        LoRAAdapter(net, LoRAConfig(r=4, target="all")).load_state_dict({k: v for k, v in sd.items() if "conv_in" not in k})
    with pytest.raises(ValueError, match="no adapted layer"):
        LoRAAdapter(net, LoRAConfig(r=4, target="attn")).load_state_dict(sd)
    with pytest.raises(FileNotFoundError):
        LoRAAdapter.load(twin, str(tmp_path / "nothing"))


def test_pipeline_writes_unet_lora_only_when_asked(tmp_path):
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.pipelines import DDPMPipeline
    net = UNet2DModel(**SMALL, device="cpu")
    ad = LoRAAdapter(net, LoRAConfig(r=2))
    pipe = DDPMPipeline(net, S.DDPMScheduler())
    pipe.save_pretrained(str(tmp_path / "plain"))
    pipe.save_pretrained(str(tmp_path / "lora"), lora=ad)
    assert not os.path.exists(tmp_path / "plain" / "unet_lora")
    assert sorted(os.listdir(tmp_path / "lora" / "unet_lora")) == ["adapter_config.json", "adapter_model.safetensors"]
    assert sorted(os.listdir(tmp_path / "lora" / "unet")) == sorted(os.listdir(tmp_path / "plain" / "unet"))
    with pytest.raises(ValueError, match="this pipeline"):
        pipe.save_pretrained(str(tmp_path / "bad"), lora=LoRAAdapter(UNet2DModel(**SMALL, device="cpu"), LoRAConfig(r=2)))


def test_trainer_refusals_come_before_any_launch():
    """lora with ema, a wrong config type: raised in the constructor, on a structure-only network (nothing could have been launched)."""
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import EMAConfig, Trainer
    net = UNet2DModel(**SMALL, device="cpu")
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    with pytest.raises(ValueError, match="ema"):
        Trainer(net, lf, lr=1e-3, total_steps=10, ema=EMAConfig(), lora=LoRAConfig(r=4))
    with pytest.raises(TypeError, match="LoRAConfig"):
        Trainer(net, lf, lr=1e-3, total_steps=10, lora={"r": 4})


def test_header_prototypes_and_abi():
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "#define VD_ABI_VERSION 12" in hdr
    for name, n_args in (("vd_lora_merge", 9), ("vd_lora_grad", 10)):
        assert f"int {name}(" in hdr and len(lib.PROTOTYPES[name][1]) == n_args and callable(getattr(ops, name[3:]))
    assert "ADAPTER TABLE" in hdr and "n_jobs x 7 int64" in hdr
    mk = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_lora.hip" in mk


# ------------------------------------------------------------------------------------------------------------------------------- command line
def test_cli_flags(tmp_path, monkeypatch):
    import VillanDiffusion as V
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = V.parse_args(["--mode", "train", "--lora_r", "4", "--lora_alpha", "8", "--lora_target", "all"])
    assert (a.lora_r, a.lora_alpha, a.lora_target) == (4, 8.0, "all")
    d = V.parse_args(["--mode", "train"])
    assert (d.lora_r, d.lora_alpha, d.lora_target) == (None, None, None)
    with pytest.raises(SystemExit):
        V.parse_args(["--mode", "train", "--lora_target", "linear"])
    c = V.TrainingConfig()
    assert (c.lora_r, c.lora_alpha, c.lora_target) == (None, None, "attn") and V.lora_config(c) is None
    base = ["--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--ckpt", "DDPM-32-DEFAULT", "-o"]
    off = V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "off")] + base))
    on = V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "on"), "--lora_r", "4", "--lora_target", "conv"] + base))
    assert off.lora_r is None and (on.lora_r, on.lora_alpha, on.lora_target) == (4, None, "conv")
    lc = V.lora_config(on)
    assert (lc.r, lc.s, lc.target, lc.seed) == (4, 1.0, "conv", on.seed)
    assert on.output_dir.split(os.sep)[-1] == off.output_dir.split(os.sep)[-1]           # naming_fn does not know the flags
    for f in ("args.json", "config.json"):
        d_off, d_on = json.load(open(os.path.join(off.output_dir, f))), json.load(open(os.path.join(on.output_dir, f)))
        assert not any(k.startswith("lora_") for k in d_off), f
        assert d_on["lora_r"] == 4 and d_on["lora_target"] == "conv" and "lora_alpha" not in d_on, f
    # resume takes them from args.json; sampling reads the run but rejects the flags themselves
    r = V.setup(V.parse_args(["--mode", "resume", "--ckpt", on.output_dir]))
    assert (r.lora_r, r.lora_target) == (4, "conv") and V.lora_config(r).r == 4
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", off.output_dir])).lora_r is None
    assert V.setup(V.parse_args(["--mode", "sampling", "--ckpt", on.output_dir])).lora_r == 4
    with pytest.raises(NotImplementedError, match="lora_r"):
        V.setup(V.parse_args(["--mode", "sampling", "--ckpt", on.output_dir, "--lora_r", "4"]))
    with pytest.raises(NotImplementedError, match="lora_target"):
        V.setup(V.parse_args(["--mode", "measure", "--ckpt", off.output_dir, "--lora_target", "all"]))
    with pytest.raises(ValueError, match="ema_decay"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_r", "4", "--ema_decay", "0.999"] + base))
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_r", "4", "--gpu", "0,1"] + base))
    with pytest.raises(ValueError, match="r must be"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_r", "33"] + base))
    with pytest.raises(ValueError, match="need --lora_r"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_alpha", "8"] + base))
    assert not os.path.exists(tmp_path / "bad")                                          # every refusal came before the run directory


def test_tool_help():
    import subprocess
    import sys
    for tool in ("lora_adapter.py", "lora_step_ab.py"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, PYTHONPATH=ROOT))
        assert out.returncode == 0 and "usage" in out.stdout.lower(), out.stderr[-500:]
