"""LoRA's adapted backward without a GPU: tests/lora_act_ref.py against lora_ref and autograd in float64, the routing table of the small, the
CIFAR10 and the latent-diffusion networks, the refusals, the command line, the header."""
import json
import os
import subprocess
import sys

import pytest
import torch

import lora_act_ref
import lora_ref
from villandiffusion_amd import lib, lora, ops
from villandiffusion_amd.lora import BackwardRoute, LoRAAdapter, LoRAConfig, adapter_table, backward_routes
from villandiffusion_amd.model import LDM_CELEBA_UNET_ARCH
from villandiffusion_amd.ncsnpp import NCSNppModel
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_lora_gpu.py's
NETS = {"small": SMALL, "cifar10": {}, "ldm": LDM_CELEBA_UNET_ARCH}


# ------------------------------------------------------------------------------------------------------------------------------ the closed forms
@pytest.mark.parametrize("shape", [(5, 3, 1, 1), (8, 6, 7, 3), (6, 9, 16, 2)])
def test_closed_forms_equal_the_weight_gradient_route_and_autograd(shape):
    M, L, N, Bn = shape
    r, s = 2, 1.7
    gen = torch.Generator().manual_seed(M + L)
    dy, x = torch.randn(Bn, M, N, generator=gen, dtype=torch.float64), torch.randn(Bn, L, N, generator=gen, dtype=torch.float64)
    A, Bm, W0 = (torch.randn(*sh, generator=gen, dtype=torch.float64) for sh in ((r, L), (M, r), (M, L)))
    dA, dB = lora_act_ref.grads(dy, x, A, Bm, s)
    wA, wB = lora_ref.grads(lora_act_ref.weight_grad(dy, x), A, Bm, s)
    assert torch.allclose(dA, wA, rtol=1e-12, atol=1e-12) and torch.allclose(dB, wB, rtol=1e-12, atol=1e-12)
    a, b = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x.view(Bn, L, N, 1), (W0 + s * b @ a)[:, :, None, None])
    (y * dy.view(Bn, M, N, 1)).sum().backward()
    assert torch.allclose(dA, a.grad, rtol=1e-12, atol=1e-12) and torch.allclose(dB, b.grad, rtol=1e-12, atol=1e-12)
    bA, bB = lora_act_ref.bounds(dy, x, A, Bm, s)
    assert bA.shape == dA.shape and bB.shape == dB.shape and bool((bA > 0).all()) and bool((bB > 0).all())


# ------------------------------------------------------------------------------------------------------------------------------ the routing table
@pytest.fixture(scope="module")
def nets():
    return {k: UNet2DModel(**kw, device="cpu") for k, kw in NETS.items()}


@pytest.mark.parametrize("net_name", list(NETS))
@pytest.mark.parametrize("target", ["attn", "conv", "all"])
def test_routing_table(nets, net_name, target):
    net = nets[net_name]
    tab = adapter_table(net, LoRAConfig(r=4, target=target))
    rt = backward_routes(net, tab)
    direct, full = rt["direct"], rt["full"]
    assert sorted(direct + full) == sorted(tab.slices) and not set(direct) & set(full)              # a partition of the adapter table's jobs
    if target == "attn":
        assert full == [] and len(direct) == len(tab.slices) and rt["temb"] is False
        assert all(".attentions." in n for n in direct)
    elif target == "conv":
        assert direct and all(n.endswith(".conv_shortcut.weight") for n in direct) and rt["temb"] is False
        assert full and all(net._offs[n][2][2:] == (3, 3) for n in full)                            # every 3x3 is full, conv_in included
        assert sorted(direct) == sorted(n for n in tab.slices if net._offs[n][2][2:] == (1, 1))
    else:
        assert rt["temb"] is True
        assert "time_embedding.linear_1.weight" in full and "time_embedding.linear_2.weight" in full
        assert all(n in full for n in tab.slices if ".time_emb_proj." in n) and "conv_in.weight" in full
        assert all(n in direct for n in tab.slices if ".attentions." in n or ".conv_shortcut." in n)
    route = BackwardRoute(net, tab, torch.zeros(tab.numel), torch.zeros(tab.numel))
    by_name = dict(zip(tab.slices, tab.jobs))
    assert sorted(route.direct) == sorted(by_name[n][0] for n in direct) and route.full_offs == {by_name[n][0] for n in full}
    if full:
        sub = route.full_table
        assert [j[:5] for j in sub.jobs] == [by_name[n][:5] for n in full] and sub.numel == tab.numel and (sub.r, sub.s) == (tab.r, tab.s)
    else:
        assert route.full_table is None
    # the funnel's look-up: a fused q, k, v gradient view holds three direct adapters, a bias view none
    if target != "conv":
        prefix, ch = net._qkv[0]
        gq = net.Gq[prefix + "::qkv_w"]
        assert route.wants(net, gq) and route.wants(net, net.G[prefix + ".to_out.0.weight"])
    assert route.wants(net, net.G["conv_out.weight"].view(net.out_channels, -1)) is False           # min(M, L) <= r: never adapted
    assert route.wants(net, net.G["down_blocks.0.resnets.0.conv1.weight"].view(net._offs["down_blocks.0.resnets.0.conv1.weight"][2][0], -1)) \
        is (target != "attn")


def test_plan_lays_out_chunks_workgroups_and_workspace():
    r = 4
    jobs = [(4096, 96 * 64, 8192, 32 * 64, 2, 32, 32, 64, 0, 128),            # one table row
            (4096, 0, 8192, 0, 3, 896, 896, 1000, 256, 4096)]                 # 1792 accumulator rows: 768 + 768 + 256
    plan = ops.lora_act_plan(jobs, r, workgroups=64)
    h = plan.host
    assert h.shape == (4, ops.ACT_COLS) and h[:, 12].tolist() == [0, 0, 768, 1536] and h[:, 13].tolist() == [64, 768, 768, 256]
    tiles = [2 * 2, 3 * 32, 3 * 32, 3 * 32]
    assert all(1 <= int(n) <= t for n, t in zip(h[:, 11], tiles))
    assert h[:, 10].tolist() == [0] + torch.cumsum(h[:, 11], 0)[:-1].tolist()
    assert h[:, 14].tolist() == [0] + torch.cumsum(h[:, 11] * h[:, 13] * r, 0)[:-1].tolist()
    assert plan.ws_floats == int((h[:, 11] * h[:, 13] * r).sum()) == lib.load().vd_lora_act_grad_ws_floats(h.data_ptr(), 4, r)
    assert plan.nbytes == 4.0 * (2 * 64 * 64 + 3 * 1000 * 1792)
    bad = h.clone()
    bad[1, 13] = 769                                                          # more rows than a workgroup's threads can hold
    assert lib.load().vd_lora_act_grad_ws_floats(bad.data_ptr(), 4, r) == -1
    assert lib.load().vd_lora_act_grad_ws_floats(h.data_ptr(), 4, 33) == -1


# ------------------------------------------------------------------------------------------------------------------------------ refusals, surface
def test_refusals_come_before_the_device_is_touched():
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import Trainer
    net = UNet2DModel(**SMALL, device="cpu")
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    with pytest.raises(ValueError, match="backward must be one of"):
        LoRAAdapter(net, LoRAConfig(r=4), backward="lazy")
    with pytest.raises(ValueError, match="backward must be one of"):
        Trainer(net, lf, lr=1e-3, total_steps=10, lora=LoRAConfig(r=4), lora_backward="lazy")
    for mode in ("full", "adapted"):
        with pytest.raises(ValueError, match="needs lora"):
            Trainer(net, lf, lr=1e-3, total_steps=10, lora_backward=mode)
    import anp_families_ref as fam
    pp = NCSNppModel(**dict(fam.SMALL_PP, layers_per_block=1), device="cpu")
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        LoRAAdapter(pp, LoRAConfig(r=4, target="all"), backward="adapted")
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        Trainer(pp, lf, lr=1e-3, total_steps=10, lora=LoRAConfig(r=4, target="all"), lora_backward="adapted")
    assert net.lora_route is None and pp.lora_route is None and UNet2DModel.lora_route is None


def test_the_mode_belongs_to_the_run_not_to_the_adapter(tmp_path):
    net = UNet2DModel(**SMALL, device="cpu")
    cfg = LoRAConfig(r=4, alpha=8.0, target="all", seed=11)
    full = LoRAAdapter(net, cfg)
    assert full.backward == "full" and full.route is None and net.lora_route is None
    ad = LoRAAdapter(net, cfg, backward="adapted")
    assert ad.backward == "adapted" and net.lora_route is ad.route and ad.route.gab is ad.grad and ad.route.ab is ad.param
    assert torch.equal(ad.param, full.param) and ad.table.jobs == full.table.jobs
    assert ad.train_state()["config"] == full.train_state()["config"] == cfg.to_dict()
    ad.save(str(tmp_path / "a"))
    full.save(str(tmp_path / "f"))
    for f in ("adapter_config.json",):
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "f" / f).read()
    assert "backward" not in json.load(open(tmp_path / "a" / "adapter_config.json"))
    ad.grad.fill_(3.0)
    ad.zero_grad()
    assert float(ad.grad.abs().sum()) == 0.0
    ad.detach()
    assert net.lora_route is None


def test_header_prototypes_and_abi():
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "#define VD_ABI_VERSION 12" in hdr and lib.load().vd_abi_version() == 12
    assert "int vd_lora_act_grad(" in hdr and "int64_t vd_lora_act_grad_ws_floats(" in hdr and "ACTIVATION JOB TABLE" in hdr
    proto = hdr[hdr.index("int vd_lora_act_grad("):]
    proto = proto[:proto.index(";")]
    assert proto.count(",") + 1 == len(lib.PROTOTYPES["vd_lora_act_grad"][1]) == 11
    assert len(lib.PROTOTYPES["vd_lora_act_grad_ws_floats"][1]) == 3 and lib.PROTOTYPES["vd_lora_act_grad_ws_floats"][0] is lib._i64
    assert callable(ops.lora_act_grad) and callable(ops.lora_act_plan)


# ------------------------------------------------------------------------------------------------------------------------------- command line
def test_cli_flag(tmp_path, monkeypatch):
    import VillanDiffusion as V
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert V.parse_args(["--mode", "train"]).lora_backward is None
    assert V.parse_args(["--mode", "train", "--lora_r", "4", "--lora_backward", "adapted"]).lora_backward == "adapted"
    with pytest.raises(SystemExit):
        V.parse_args(["--mode", "train", "--lora_backward", "lazy"])
    base = ["--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--ckpt", "DDPM-32-DEFAULT", "-o"]
    runs = {}
    for name, extra in (("off", []), ("lora", ["--lora_r", "4"]), ("adapted", ["--lora_r", "4", "--lora_backward", "adapted"]),
                        ("full", ["--lora_r", "4", "--lora_backward", "full"])):
        runs[name] = V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / name)] + extra + base))
    assert [runs[k].lora_backward for k in ("off", "lora", "adapted", "full")] == [None, None, "adapted", "full"]
    for f in ("args.json", "config.json"):
        side = {k: json.load(open(os.path.join(c.output_dir, f))) for k, c in runs.items()}
        assert not any(k.startswith("lora_") for k in side["off"]), f               # a run without LoRA still has no lora_* key
        assert "lora_backward" not in side["lora"] and side["lora"]["lora_r"] == 4, f
        assert side["adapted"]["lora_backward"] == "adapted" and side["full"]["lora_backward"] == "full", f
    # resume reads it back; the other modes reject the flag itself
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", runs["adapted"].output_dir])).lora_backward == "adapted"
    assert V.setup(V.parse_args(["--mode", "resume", "--ckpt", runs["lora"].output_dir])).lora_backward is None
    for mode in ("resume", "sampling", "measure"):
        with pytest.raises(NotImplementedError, match="lora_backward"):
            V.setup(V.parse_args(["--mode", mode, "--ckpt", runs["adapted"].output_dir, "--lora_backward", "adapted"]))
    with pytest.raises(ValueError, match="need --lora_r"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_backward", "adapted"] + base))
    with pytest.raises(NotImplementedError, match="SDE-VE"):
        V.setup(V.parse_args(["--mode", "train", "--result", str(tmp_path / "bad"), "--lora_r", "4", "--lora_target", "all", "--lora_backward",
                              "adapted", "--sde_type", "SDE-VE"] + base))
    assert not os.path.exists(tmp_path / "bad")


def test_tool_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lora_backward_ab.py"), "--help"], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0 and "usage" in out.stdout.lower(), out.stderr[-500:]
