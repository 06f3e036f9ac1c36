"""Sharpness-aware fine-tuning without a GPU: the reference step of tests/sam_ref.py (rho -> 0 is the plain step, <e, g> = rho ||g||, which
floats the neuron mode moves), the library's new symbols and its host-only launch plan, every refusal of `Trainer(sam=...)` and every flag
check of the drivers -- none of them may ask for a kernel."""
import copy
import ctypes as C
import json
import math
import os

import pytest
import torch

import sam_ref
from oracle.unet_ref import UNet2DModelRef
from villandiffusion_amd import anp, lib, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd import schedulers as S
from villandiffusion_amd.loss import LossFn
from villandiffusion_amd.trainer import EMAConfig, SAMConfig, Trainer, check_sam
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_sam_plan", "vd_sam_norm_sq", "vd_sam_perturb", "vd_sam_neuron_coef", "vd_neuron_axpy")
EINVAL = -22


@pytest.fixture(scope="module")
def small_ref():
    torch.manual_seed(0)
    return UNet2DModelRef(**sam_ref.SMALL)


def state(ref):
    return {k: v.detach().clone() for k, v in ref.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_with_rho_zero_is_the_plain_step(small_ref):
    rows = anp.neuron_table(UNet2DModel(**sam_ref.SMALL, device="cpu"), "conv").slices
    plain = sam_ref.SamOnOracle(copy.deepcopy(small_ref), None)
    for i in range(2):
        plain.step(*sam_ref.batch_of(i))
    want = state(plain.ref)
    for mode in ("sam", "asam", "neuron"):
        o = sam_ref.SamOnOracle(copy.deepcopy(small_ref), mode, rho=0.0, rows=rows)
        for i in range(2):
            l1, l2 = o.step(*sam_ref.batch_of(i))
            assert l1 == l2                                   # e = 0: the second pass is the first
        got = state(o.ref)
        assert all(torch.equal(got[k], want[k]) for k in want), mode
    # ... and a small rho is a small change of the step, a large one a large change
    near = sam_ref.SamOnOracle(copy.deepcopy(small_ref), "sam", rho=1e-6)
    far = sam_ref.SamOnOracle(copy.deepcopy(small_ref), "sam", rho=0.05)
    for i in range(2):
        near.step(*sam_ref.batch_of(i))
        far.step(*sam_ref.batch_of(i))
    start = state(small_ref)
    d_near, d_far = sam_ref.update_l2_error(state(near.ref), want, start), sam_ref.update_l2_error(state(far.ref), want, start)
    assert d_near < 1e-3 < 0.05 < d_far, (d_near, d_far)


def test_reference_perturbations(small_ref):
    ref = copy.deepcopy(small_ref)
    net = UNet2DModel(**sam_ref.SMALL, device="cpu")
    o = sam_ref.SamOnOracle(ref, "sam", rho=0.05)
    o._pass(*sam_ref.batch_of(0))
    params = {k: p.detach().double() for k, p in o.named.items()}
    grads = {k: p.grad.detach().double() for k, p in o.named.items()}
    gnorm = math.sqrt(sum(float((v ** 2).sum()) for v in grads.values()))
    # "sam": <e, g> = rho ||g||, and ||e|| = rho
    e = sam_ref.perturbation(params, grads, "sam", 0.05)
    dot = sum(float((e[k] * grads[k]).sum()) for k in e)
    assert abs(dot - 0.05 * gnorm) <= 1e-9 * 0.05 * gnorm
    assert abs(math.sqrt(sum(float((v ** 2).sum()) for v in e.values())) - 0.05) <= 1e-9
    # "asam": ||e / T|| = rho, and a float with a larger |w| moves further for the same gradient
    ea = sam_ref.perturbation(params, grads, "asam", 0.5, 0.01)
    T = {k: params[k].abs() + 0.01 for k in params}
    assert abs(math.sqrt(sum(float(((ea[k] / T[k]) ** 2).sum()) for k in ea)) - 0.5) <= 1e-9
    # "neuron": exactly the floats outside the table's weight rows have e = 0
    for layers in ("conv", "all"):
        tab = anp.neuron_table(net, layers)
        en = sam_ref.perturbation(params, grads, "neuron", 0.5, 0.01, rows=tab.slices)
        for k, v in en.items():
            if k in tab.slices:
                assert bool((v != 0).any()) and v.shape[0] == tab.slices[k].stop - tab.slices[k].start, k
            else:
                assert not bool((v != 0).any()), k
        moved = sum(int((v != 0).sum()) for v in en.values())
        assert 0.9 * tab.weight_floats < moved <= tab.weight_floats
        assert "conv_out.weight" not in tab.slices and not any(k.endswith(".bias") for k in tab.slices)
        # sum_j T_j^2 gsq_j normalises it: || e_row / T_row || = rho
        tot = 0.0
        for k in tab.slices:
            w = params[k].reshape(params[k].shape[0], -1)
            Tj = ((w ** 2).sum(1) / w.shape[1]).sqrt() + 0.01
            tot += float(((en[k].reshape(w.shape) / Tj[:, None]) ** 2).sum())
        assert abs(math.sqrt(tot) - 0.5) <= 1e-9


# ------------------------------------------------------------------------------------------------------------------------------- the library
def test_header_prototypes_makefile_and_abi():
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "#define VD_ABI_VERSION 12" in hdr and lib.load().vd_abi_version() == 12
    for name, n_args in zip(NEW, (4, 8, 9, 10, 7)):
        assert f"int {name}(" in hdr and len(lib.PROTOTYPES[name][1]) == n_args and hasattr(lib.load(), name), name
    for fn in ("sam_plan", "sam_norm_sq", "sam_perturb", "sam_neuron_coef", "neuron_axpy"):
        assert callable(getattr(ops, fn))
    assert "longest chain of additions is ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18" in hdr
    assert "chain of additions is sum over the jobs of ceil(rows / 256), plus 8" in hdr
    mk = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_sam.hip" in mk and "vd_sam.o: vd_sam.hip" in mk and mk.split("vd_sam.o: vd_sam.hip")[1].split("\n\n")[0].count("-ffp-contract=off") == 1


def test_sam_plan_is_host_only(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))
    assert ops.sam_plan(0) == (1, 256, 16) and ops.sam_plan(1) == (1, 256, 16)
    assert ops.sam_plan(4096) == (1, 256, 16) and ops.sam_plan(4097) == (2, 256, 16)
    cap = ops.sam_plan(1 << 40)[0]
    assert cap <= 1024                                         # `partial` holds 1024 floats
    assert ops.sam_plan(cap * 4096)[0] == cap and ops.sam_plan((cap - 1) * 4096)[0] == cap - 1 and ops.sam_plan(cap * 4096 + 1)[0] == cap
    g, b, f = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.load().vd_sam_plan(-1, C.byref(g), C.byref(b), C.byref(f)) == EINVAL
    assert lib.load().vd_sam_plan(8, None, C.byref(b), C.byref(f)) == EINVAL
    assert sam_ref.norm_chain(35_700_000, *ops.sam_plan(35_700_000)[:2]) == 35 + 4 + 18


# ------------------------------------------------------------------------------------------------------------------------------- refusals
def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


def test_config_refusals():
    for bad in (0, 0.0, -0.1, float("inf"), float("nan"), "0.05", None, True):
        with pytest.raises(ValueError, match="rho"):
            SAMConfig(rho=bad)
    for bad in (-1e-3, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="eta"):
            SAMConfig(rho=0.05, eta=bad)
    with pytest.raises(ValueError, match="mode"):
        SAMConfig(rho=0.05, mode="fisher")
    with pytest.raises(ValueError, match="layers"):
        SAMConfig(rho=0.05, mode="neuron", layers="attn")
    c = SAMConfig(rho=0.05)
    assert (c.mode, c.eta, c.layers) == ("sam", 0.01, "conv") and SAMConfig(rho=1, eta=0).eta == 0


def test_trainer_refusals_come_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    from villandiffusion_amd.lora import LoRAConfig
    net = UNet2DModel(**sam_ref.SMALL, device="cpu")
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    sam = SAMConfig(rho=0.05)
    kw = dict(lr=1e-3, total_steps=10)
    with pytest.raises(ValueError, match="grad_accum"):
        Trainer(net, lf, grad_accum=2, sam=sam, **kw)
    with pytest.raises(ValueError, match="lora"):
        Trainer(net, lf, lora=LoRAConfig(r=4), sam=sam, **kw)
    with pytest.raises(ValueError, match="graph_micro_step"):
        Trainer(net, lf, graph_micro_step=True, sam=sam, **kw)
    with pytest.raises(TypeError, match="SAMConfig"):
        Trainer(net, lf, sam={"rho": 0.05}, **kw)
    net.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16"):
        Trainer(net, lf, sam=sam, **kw)
    net.conv_math = "bf16x3"
    with pytest.raises(NotImplementedError, match="more than one rank"):
        check_sam(sam, world=2)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        Trainer(net, lf, sam=sam, **kw)
    monkeypatch.undo()
    _no_kernels(monkeypatch)
    # what is allowed passes: every mode, with EMA, an eager micro-step, bf16x3 / f32 / bf16 arithmetic; sam=None is always allowed
    for mode, layers in (("sam", "conv"), ("asam", "conv"), ("neuron", "conv"), ("neuron", "all")):
        for math_mode in (None, "bf16x3", "f32", "bf16"):
            assert check_sam(SAMConfig(rho=0.05, mode=mode, layers=layers), 1, None, False, 1, math_mode) is None
    assert check_sam(None, grad_accum=4, lora=object(), graph_micro_step=True, world=8, conv_math="f16") is None


# ------------------------------------------------------------------------------------------------------------------------------- the drivers
def test_cli_flags_and_their_errors(tmp_path, monkeypatch):
    import VillanDiffusion as V
    import rm_backdoor_VillanDiffusion as RM
    _no_kernels(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("VILLAN_MIXED_PRECISION", raising=False)
    assert RM.main is V.main
    base = ["--project", "p", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--result", str(tmp_path), "-o"]
    a = V.parse_args(["--mode", "train", "--sam_rho", "0.05", "--sam_mode", "neuron", "--sam_eta", "0.02", "--sam_layers", "all"] + base)
    assert (a.sam_rho, a.sam_mode, a.sam_eta, a.sam_layers) == (0.05, "neuron", 0.02, "all")
    d = V.parse_args(["--mode", "train"])
    assert (d.sam_rho, d.sam_mode, d.sam_eta, d.sam_layers) == (None, None, None, None)
    for bad in (["--sam_mode", "fisher"], ["--sam_layers", "attn"]):
        with pytest.raises(SystemExit):
            V.parse_args(["--mode", "train"] + bad)
    cfg = V.setup(a)
    sc = V.sam_config(cfg)
    assert sc == SAMConfig(rho=0.05, mode="neuron", eta=0.02, layers="all") and cfg.gradient_accumulation_steps == 1
    for side in ("args.json", "config.json"):
        with open(os.path.join(cfg.output_dir, side)) as f:
            j = json.load(f)
        assert (j["sam_rho"], j["sam_mode"], j["sam_eta"], j["sam_layers"]) == (0.05, "neuron", 0.02, "all"), side
    # --sam_rho alone: the defaults are SAMConfig's, and stay out of the side files
    only = V.setup(V.parse_args(["--mode", "train", "--sam_rho", "0.05", "--postfix", "only"] + base))
    assert V.sam_config(only) == SAMConfig(rho=0.05)
    with open(os.path.join(only.output_dir, "args.json")) as f:
        j = json.load(f)
    assert j["sam_rho"] == 0.05 and not {"sam_mode", "sam_eta", "sam_layers"} & set(j)
    # resume takes them from args.json, and refuses them on its own command line
    r = V.setup(V.parse_args(["--mode", "resume", "--ckpt", cfg.output_dir]))
    assert V.sam_config(r) == sc
    assert V.sam_config(V.setup(V.parse_args(["--mode", "sampling", "--ckpt", cfg.output_dir]))) == sc
    for extra in (["--sam_rho", "0.1"], ["--sam_mode", "asam"], ["--sam_eta", "0.1"], ["--sam_layers", "conv"]):
        for mode in ("resume", "sampling", "measure"):
            with pytest.raises(NotImplementedError, match="isn't supported in mode"):
                V.setup(V.parse_args(["--mode", mode, "--ckpt", cfg.output_dir] + extra))
    # without the flags the side files read as before the options existed
    plain = V.setup(V.parse_args(["--mode", "train", "--postfix", "plain"] + base))
    assert V.sam_config(plain) is None
    with open(os.path.join(plain.output_dir, "config.json")) as f:
        assert not any(k.startswith("sam_") for k in json.load(f))

    def refused(exc, match, extra, tag):
        with pytest.raises(exc, match=match):
            V.setup(V.parse_args(["--mode", "train", "--postfix", tag] + extra + base))
        name = V.naming_fn(V.TrainingConfig(**{**{k: v for k, v in vars(plain).items() if k in V.TrainingConfig.__dataclass_fields__}, "postfix": tag}))
        assert not os.path.isdir(os.path.join(str(tmp_path), name)), f"{tag}: an argument error creates no run directory"

    for i, extra in enumerate((["--sam_mode", "sam"], ["--sam_eta", "0.01"], ["--sam_layers", "conv"])):
        refused(ValueError, "need --sam_rho", extra, f"norho{i}")
    refused(ValueError, "rho", ["--sam_rho", "0"], "rho0")
    refused(ValueError, "rho", ["--sam_rho", "-1"], "rhoneg")
    refused(ValueError, "rho", ["--sam_rho", "inf"], "rhoinf")
    refused(ValueError, "eta", ["--sam_rho", "0.05", "--sam_eta", "-1"], "etaneg")
    refused(ValueError, "lora", ["--sam_rho", "0.05", "--lora_r", "4"], "lora")
    refused(NotImplementedError, "more than one", ["--sam_rho", "0.05", "--gpu", "0,1"], "gpus")
    # the effective gradient-accumulation count is the data set's batch size over --batch: it must be 1
    with pytest.raises(ValueError, match="gradient-accumulation count of 1, got 2"):
        V.setup(V.parse_args(["--mode", "train", "--sam_rho", "0.05", "--postfix", "accum", "--project", "p", "--dataset", "SYNTHETIC-CIFAR10",
                              "--batch", "64", "--epoch", "1", "--result", str(tmp_path), "-o"]))
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "fp16")
    refused(NotImplementedError, "f16", ["--sam_rho", "0.05"], "f16")
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "bf16")
    assert V.sam_config(V.setup(V.parse_args(["--mode", "train", "--sam_rho", "0.05", "--postfix", "bf16"] + base))) == SAMConfig(rho=0.05)
