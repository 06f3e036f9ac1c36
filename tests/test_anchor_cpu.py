"""Anchored fine-tuning without a GPU: the oracle of tests/anchor_ref.py (its autograd penalty gradient is the closed form, its anchored
trajectories lie far from its plain one for the lambda, F and w0 the GPU tests use), the library's new symbols, their host-only launch plan and
their refusals, AnchorConfig, every refusal of `check_anchor` / `Trainer(anchor=...)`, fisher.pt, and every flag check of the drivers -- none of
them may ask for a kernel."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

import anchor_ref
from villandiffusion_amd import anchor, lib, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd import schedulers as S
from villandiffusion_amd.anchor import AnchorConfig, check_anchor
from villandiffusion_amd.loss import LossFn
from villandiffusion_amd.ncsnpp import NCSNppModel
from villandiffusion_amd.trainer import Trainer
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_anchor_plan", "vd_fisher_accum", "vd_anchor_grad")
EINVAL = -22


def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


# ------------------------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("mode", anchor_ref.MODES)
def test_the_oracles_penalty_gradient_is_the_closed_form(mode):
    """autograd of lam / 2 * sum F d^2 against lam * F * d: a product and a sum of two equal halves per element, so float32 rounding only."""
    s = anchor_ref.setup()
    gen = anchor_ref.g(5)
    params = {k: (v + 0.01 * torch.randn(v.shape, generator=gen)).requires_grad_(True) for k, v in s["start"].items()}
    w0, F = anchor_ref.named(s["w0"], s["offs"]), (anchor_ref.named(s["F"], s["offs"]) if mode == "ewc" else None)
    anchor_ref.penalty(params, w0, F, anchor_ref.LAM).backward()
    want = anchor_ref.closed_form_grad(params, w0, F, anchor_ref.LAM)
    worst = 0.0
    for k, p in params.items():
        assert bool(((p.grad - want[k]).abs() <= 4 * 2.0 ** -24 * want[k].abs()).all()), k
        worst = max(worst, float(want[k].abs().max()))
    assert worst > 1e-4                                        # the penalty acts


@pytest.mark.parametrize("mode", anchor_ref.MODES)
def test_the_anchored_trajectory_lies_far_from_the_plain_one(mode):
    """||theta - theta_plain|| / ||theta_plain - theta_0|| >= 0.1 after the four steps of the GPU trajectory test: a trainer that dropped the
    penalty could not pass it.  The penalty starts positive (w0 is the start plus a perturbation) and the loss is not drowned by it."""
    s, plain, o = anchor_ref.setup(), anchor_ref.oracle_run(None), anchor_ref.oracle_run(mode)
    away = anchor_ref.update_l2_error(o["end"], plain["end"], s["start"])
    print(f"[anchor] oracle {mode}: distance from the plain trajectory {away:.3f}; penalties {o['penalties']}; losses {o['losses']}")
    assert away >= 0.1, away
    assert o["penalties"][0] > 0.1 * o["losses"][0] and o["penalties"][0] < 10 * o["losses"][0]
    assert plain["penalties"] == [None] * 4 and o["losses"][0] == plain["losses"][0]
    F = s["F"]
    assert float(F.max()) > 100 * float(F[F > 0].min()) and abs(float(F.mean()) - 1) < 0.1     # non-uniform, about mean 1


def test_the_oracle_applies_the_penalty_once_per_optimiser_step():
    """Two micro-batches per step: the mean loss plus ONE penalty; its first step differs from two steps of one micro-batch each."""
    o2 = anchor_ref.oracle_run("ewc", accum=2, steps=2)
    o1 = anchor_ref.oracle_run("ewc")
    assert o2["penalties"][0] == o1["penalties"][0] and o2["losses"][0] != o1["losses"][0]


# ------------------------------------------------------------------------------------------------------------------------------- the library
def test_header_prototypes_makefile_and_abi():
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "#define VD_ABI_VERSION 12" in hdr and lib.load().vd_abi_version() == 12
    for name, n_args in zip(NEW, (4, 5, 9)):
        assert f"int {name}(" in hdr and len(lib.PROTOTYPES[name][1]) == n_args and hasattr(lib.load(), name), name
    for fn in ("anchor_plan", "fisher_accum", "anchor_grad"):
        assert callable(getattr(ops, fn))
    sec = hdr.split("int vd_anchor_plan(")[0].split("Anchored fine-tuning")[1] + hdr.split("int vd_anchor_plan(")[1].split("int vd_anchor_grad(")[0]
    assert "q = g[i] * g[i];  F[i] = F[i] + s * q" in sec and "d = w[i] - w0[i];  t = F[i] * d (F NULL: t = d, L2-SP);  g[i] = g[i] + coef * t" in sec
    assert "longest chain of additions is ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18" in sec and "vd_sam_plan's rule" in sec
    assert "no FMA contraction" in sec
    mk = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_anchor.hip" in mk and mk.split("vd_anchor.o: vd_anchor.hip")[1].split("\n\n")[0].count("-ffp-contract=off") == 1


def test_anchor_plan_is_host_only_and_is_sam_plans_rule(monkeypatch):
    _no_kernels(monkeypatch)
    for n in (0, 1, 4096, 4097, 100003, 1 << 22, (1 << 22) + 1, 1 << 40):
        assert ops.anchor_plan(n) == ops.sam_plan(n), n
    assert ops.anchor_plan(1 << 40) == (1024, 256, 16)
    g, b, f = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.load().vd_anchor_plan(-1, C.byref(g), C.byref(b), C.byref(f)) == EINVAL
    assert lib.load().vd_anchor_plan(8, None, C.byref(b), C.byref(f)) == EINVAL
    assert anchor_ref.pen_chain(35_700_000, *ops.anchor_plan(35_700_000)[:2]) == 35 + 4 + 18


def test_refusals_through_ctypes_need_no_device(monkeypatch):
    """VD_EINVAL before any launch, on host buffers whose addresses are only compared: nothing is launched, so no device is needed."""
    _no_kernels(monkeypatch)
    h = lib.load()
    n = 64
    bufs = [torch.zeros(n + 4) for _ in range(4)]
    g, w, w0, F = (C.c_void_p(t.data_ptr()) for t in bufs)
    partial, pen = torch.zeros(1024), torch.zeros(1)
    P = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")
    ok = dict(F=F, g=g, n=n, s=0.5)
    for bad in (dict(n=-1), dict(F=None), dict(g=None), dict(g=F), dict(g=C.c_void_p(bufs[3].data_ptr() + 16)), dict(s=nan), dict(s=inf),
                dict(s=-inf), dict(s=-0.5), dict(F=C.c_void_p(bufs[3].data_ptr() + 2))):
        a = dict(ok, **bad)
        assert h.vd_fisher_accum(a["F"], a["g"], a["n"], a["s"], None) == EINVAL, bad
    assert "vd_fisher_accum" in lib.last_error()
    assert h.vd_fisher_accum(F, g, 0, 0.5, None) == 0                        # n = 0: nothing to do, nothing launched
    ok = dict(g=g, w=w, w0=w0, F=F, n=n, coef=0.5, partial=P(partial), pen=P(pen))
    for bad in (dict(n=-1), dict(g=None), dict(w=None), dict(w0=None), dict(partial=None), dict(coef=nan), dict(coef=inf), dict(coef=-inf),
                dict(w=g), dict(w0=g), dict(F=g), dict(w0=w), dict(F=w), dict(F=w0), dict(w0=C.c_void_p(bufs[1].data_ptr() + 16)),
                dict(pen=g), dict(partial=w), dict(pen=C.c_void_p(partial.data_ptr() + 8)), dict(g=C.c_void_p(bufs[0].data_ptr() + 1))):
        a = dict(ok, **bad)
        assert h.vd_anchor_grad(a["g"], a["w"], a["w0"], a["F"], a["n"], a["coef"], a["partial"], a["pen"], None) == EINVAL, bad
    assert "vd_anchor_grad" in lib.last_error()
    assert h.vd_anchor_grad(g, w, w0, None, 0, 0.5, None, None, None) == 0   # n = 0 without pen: nothing to do; F and partial may be NULL
    assert all(float(t.abs().sum()) == 0.0 for t in bufs)


# ------------------------------------------------------------------------------------------------------------------------------- configuration
def test_config_validation():
    for bad in (0, 0.0, -0.1, float("inf"), float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="lam"):
            AnchorConfig(lam=bad)
    with pytest.raises(ValueError, match="mode"):
        AnchorConfig(lam=0.1, mode="fisher")
    with pytest.raises(ValueError, match="needs a Fisher"):
        AnchorConfig(lam=0.1, mode="ewc")
    with pytest.raises(ValueError, match="takes no Fisher"):
        AnchorConfig(lam=0.1, fisher=torch.ones(4))
    for bad in (torch.ones(2, 2), torch.ones(4, dtype=torch.float64), [1.0]):
        with pytest.raises(ValueError, match="flat float32"):
            AnchorConfig(lam=0.1, mode="ewc", fisher=bad)
    c = AnchorConfig(lam=1)
    assert (c.mode, c.fisher) == ("l2sp", None) and AnchorConfig(lam=0.1, mode="ewc", fisher=torch.ones(4)).mode == "ewc"


def test_check_anchor_and_trainer_refusals_come_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    from villandiffusion_amd.lora import LoRAConfig
    net = UNet2DModel(**anchor_ref.SMALL, device="cpu")
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    a = AnchorConfig(lam=0.1)
    kw = dict(lr=1e-3, total_steps=10)
    with pytest.raises(ValueError, match="lora.*belongs on the adapter"):
        Trainer(net, lf, lora=LoRAConfig(r=4), anchor=a, **kw)
    with pytest.raises(TypeError, match="AnchorConfig"):
        Trainer(net, lf, anchor={"lam": 0.1}, **kw)
    with pytest.raises(ValueError, match="anchor_weights needs anchor"):
        Trainer(net, lf, anchor_weights=torch.zeros(net.flat_numel), **kw)
    net.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16.*scale"):
        Trainer(net, lf, anchor=a, **kw)
    net.conv_math = "bf16x3"
    with pytest.raises(NotImplementedError, match="more than one rank.*test"):
        check_anchor(a, world=2)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        Trainer(net, lf, anchor=a, **kw)
    monkeypatch.undo()
    _no_kernels(monkeypatch)
    for math_mode in (None, "bf16x3", "f32", "bf16"):
        assert check_anchor(a, None, 1, math_mode) is None
    assert check_anchor(None, lora=object(), world=8, conv_math="f16") is None
    # a Fisher or an anchor of another size is refused by name
    with pytest.raises(ValueError, match="fisher holds .*flat_param has"):
        Trainer(net, lf, anchor=AnchorConfig(lam=0.1, mode="ewc", fisher=torch.ones(8)), **kw)
    with pytest.raises(ValueError, match="anchor_weights holds .*flat_param has"):
        Trainer(net, lf, anchor=a, anchor_weights=torch.ones(8), **kw)


def test_removal_keywords_are_checked_before_the_device(monkeypatch):
    _no_kernels(monkeypatch)
    from villandiffusion_amd import mitigation
    net = UNet2DModel(**anchor_ref.SMALL, device="cpu")
    assert mitigation._anchor_args("x", net, None, None) is None
    with pytest.raises(ValueError, match="fisher needs anchor_lambda"):
        mitigation._anchor_args("x", net, None, torch.ones(net.flat_numel))
    with pytest.raises(ValueError, match="lam"):
        mitigation._anchor_args("x", net, -1.0, None)
    with pytest.raises(ValueError, match="Fisher holds 8 entries"):
        mitigation._anchor_args("x", net, 0.1, torch.ones(8))
    assert mitigation._anchor_args("x", net, 0.1, torch.ones(net.flat_numel)).mode == "ewc"
    import inspect
    from villandiffusion_amd import defense_ldm, defense_ve
    for fn in (mitigation.remove_backdoor, defense_ve.remove_backdoor, defense_ldm.remove_backdoor, mitigation._run_removal):
        p = inspect.signature(fn).parameters
        assert p["anchor_lambda"].default is None and p["fisher"].default is None, fn
    assert inspect.signature(mitigation._removal_step).parameters["anchor"].default is None


# ------------------------------------------------------------------------------------------------------------------------------- fisher.pt
def test_fisher_file_round_trip_and_mismatch_refusals(tmp_path, golden_dir):
    net = UNet2DModel(**anchor_ref.SMALL, device="cpu")
    with open(os.path.join(golden_dir, "flat_layouts.json")) as f:
        assert anchor.layout_digest(net) == json.load(f)["unet_small"]["rows_sha256"]       # the digest is the recorded one
    F = anchor_ref.fisher_of(net.flat_numel)
    path = anchor.save_fisher(str(tmp_path / "fisher.pt"), F, net, n_batches=3, batch=2, normalize="mean")
    got, meta = anchor.load_fisher(path, net, with_meta=True)
    assert torch.equal(got, F) and got.dtype == torch.float32
    assert meta == {"n_batches": 3, "batch": 2, "normalize": "mean", "family": "UNet2DModel", "numel": net.flat_numel,
                    "layout_sha256": anchor.layout_digest(net)}
    assert torch.equal(anchor.load_fisher(str(tmp_path), net), F)            # a directory that holds one
    assert torch.equal(anchor.load_fisher(path), F)                          # no model: no check
    other = UNet2DModel(**dict(anchor_ref.SMALL, block_out_channels=(32, 96)), device="cpu")
    with pytest.raises(ValueError, match=f"{net.flat_numel} floats; this UNet2DModel has {other.flat_numel}"):
        anchor.load_fisher(path, other)
    # the same number of floats under other names or offsets: the digest tells them apart, and the message names both
    d = torch.load(path)
    d["layout_sha256"] = hashlib.sha256(b"other").hexdigest()
    torch.save(d, str(tmp_path / "moved.pt"))
    with pytest.raises(ValueError, match=f"{d['layout_sha256'][:12]}.*{anchor.layout_digest(net)[:12]}"):
        anchor.load_fisher(str(tmp_path / "moved.pt"), net)
    with pytest.raises(ValueError, match="flat float32 tensor of"):
        anchor.save_fisher(str(tmp_path / "bad.pt"), F[:-4], net, 1, 1, "none")
    torch.save({"x": 1}, str(tmp_path / "junk.pt"))
    with pytest.raises(ValueError, match="is no fisher.pt"):
        anchor.load_fisher(str(tmp_path / "junk.pt"))
    pp = NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1,
                     down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                     up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), device="cpu")
    with pytest.raises(ValueError, match="UNet2DModel of .* this NCSNppModel has"):
        anchor.load_fisher(path, pp)


def test_normalisation_and_statistics():
    F = torch.tensor([0.0, 1e-20, 2.0, 6.0])
    assert anchor.normalize_fisher(F, "none") is F
    assert torch.equal(anchor.normalize_fisher(F, "mean"), (F.double() / 2.0).float()) and float(anchor.normalize_fisher(F, "max").max()) == 1.0
    st = anchor.fisher_stats(F)
    assert st == {"mean": 2.0, "max": 6.0, "share_below_1e-12_max": 0.5}
    with pytest.raises(ValueError, match="normalize"):
        anchor.normalize_fisher(F, "sum")
    with pytest.raises(FloatingPointError, match="mean is 0.0"):
        anchor.normalize_fisher(torch.zeros(4), "mean")
    t, eps = anchor.fisher_draws((2, 3, 4, 4), 1000, 7, 1)
    t2, eps2 = anchor.fisher_draws((2, 3, 4, 4), 1000, 7, 1)
    t3, _ = anchor.fisher_draws((2, 3, 4, 4), 1000, 7, 2)
    assert torch.equal(t, t2) and torch.equal(eps, eps2) and not torch.equal(t, t3) and int(t.max()) < 1000


# ------------------------------------------------------------------------------------------------------------------------------- the drivers
def test_cli_flags_args_json_and_the_resume_default(tmp_path, monkeypatch):
    import VillanDiffusion as V
    import rm_backdoor_VillanDiffusion as RM
    _no_kernels(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("VILLAN_MIXED_PRECISION", raising=False)
    assert RM.main is V.main and RM._V.parse_args is V.parse_args               # both drivers share the flags and setup()
    net = UNet2DModel(**anchor_ref.SMALL, device="cpu")
    fisher = anchor.save_fisher(str(tmp_path / "fisher.pt"), anchor_ref.fisher_of(net.flat_numel), net, 3, 2, "mean")
    base = ["--project", "p", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--result", str(tmp_path), "-o", "--ckpt", "BASE"]
    a = V.parse_args(["--mode", "train", "--anchor_lambda", "0.5", "--anchor_fisher", fisher] + base)
    assert (a.anchor_lambda, a.anchor_fisher, a.anchor_ckpt) == (0.5, fisher, None)
    d = V.parse_args(["--mode", "train"])
    assert (d.anchor_lambda, d.anchor_fisher, d.anchor_ckpt) == (None, None, None)
    cfg = V.setup(a)
    assert V.anchor_settings(cfg) == "ewc" and cfg.anchor_ckpt == "BASE"        # --anchor_ckpt defaults to the run's --ckpt ...
    for side in ("args.json", "config.json"):
        with open(os.path.join(cfg.output_dir, side)) as f:
            j = json.load(f)
        assert (j["anchor_lambda"], j["anchor_fisher"], j["anchor_ckpt"]) == (0.5, fisher, "BASE"), side      # ... and is recorded
    # resume reads them back: w0 comes from the ORIGINAL checkpoint, not from the run directory the resume loads its weights from
    r = V.setup(V.parse_args(["--mode", "resume", "--ckpt", cfg.output_dir]))
    assert (r.anchor_lambda, r.anchor_fisher, r.anchor_ckpt) == (0.5, fisher, "BASE") and r.ckpt == cfg.output_dir
    assert V.anchor_settings(r) == "ewc"
    for extra in (["--anchor_lambda", "0.1"], ["--anchor_fisher", fisher], ["--anchor_ckpt", "X"]):
        for mode in ("resume", "sampling", "measure"):
            with pytest.raises(NotImplementedError, match="isn't supported in mode"):
                V.setup(V.parse_args(["--mode", mode, "--ckpt", cfg.output_dir] + extra))
    # L2-SP with an explicit anchor
    l2 = V.setup(V.parse_args(["--mode", "train", "--anchor_lambda", "0.1", "--anchor_ckpt", "OTHER", "--postfix", "l2"] + base))
    assert V.anchor_settings(l2) == "l2sp" and l2.anchor_ckpt == "OTHER"
    with open(os.path.join(l2.output_dir, "args.json")) as f:
        j = json.load(f)
    assert j["anchor_ckpt"] == "OTHER" and "anchor_fisher" not in j
    # without the flags the side files read as before the options existed
    plain = V.setup(V.parse_args(["--mode", "train", "--postfix", "plain"] + base))
    assert V.anchor_settings(plain) is None
    for side in ("args.json", "config.json"):
        with open(os.path.join(plain.output_dir, side)) as f:
            assert not any(k.startswith("anchor_") for k in json.load(f))

    def refused(exc, match, extra, tag, base=base):
        with pytest.raises(exc, match=match):
            V.setup(V.parse_args(["--mode", "train", "--postfix", tag] + extra + base))
        name = V.naming_fn(V.TrainingConfig(**{**{k: v for k, v in vars(plain).items() if k in V.TrainingConfig.__dataclass_fields__}, "postfix": tag}))
        assert not os.path.isdir(os.path.join(str(tmp_path), name)), f"{tag}: an argument error creates no run directory"

    refused(ValueError, "need --anchor_lambda", ["--anchor_fisher", fisher], "nolam0")
    refused(ValueError, "need --anchor_lambda", ["--anchor_ckpt", "X"], "nolam1")
    for i, bad in enumerate(("0", "-1", "inf", "nan")):
        refused(ValueError, "lam", ["--anchor_lambda", bad], f"lam{i}")
    refused(FileNotFoundError, "no such file", ["--anchor_lambda", "0.1", "--anchor_fisher", str(tmp_path / "missing.pt")], "nofile")
    refused(ValueError, "lora", ["--anchor_lambda", "0.1", "--lora_r", "4"], "lora")
    refused(NotImplementedError, "more than one", ["--anchor_lambda", "0.1", "--gpu", "0,1"], "gpus")
    refused(ValueError, "give --ckpt or --anchor_ckpt", ["--anchor_lambda", "0.1"], "scratch", base=base[:-2])
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "fp16")
    refused(NotImplementedError, "f16", ["--anchor_lambda", "0.1"], "f16")
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "bf16")
    assert V.anchor_settings(V.setup(V.parse_args(["--mode", "train", "--anchor_lambda", "0.1", "--postfix", "bf16"] + base))) == "l2sp"
    # gradient accumulation is allowed: the penalty is added once per optimiser step
    acc = V.setup(V.parse_args(["--mode", "train", "--anchor_lambda", "0.1", "--postfix", "acc", "--project", "p", "--dataset", "SYNTHETIC-CIFAR10",
                                "--batch", "64", "--epoch", "1", "--result", str(tmp_path), "-o", "--ckpt", "BASE"]))
    assert acc.gradient_accumulation_steps == 2 and V.anchor_settings(acc) == "l2sp"
    # the removal tool's flags
    import tools.remove_backdoor as T
    with pytest.raises(SystemExit):
        T.main(["--ckpt", "x", "--trigger", "t", "--steps", "1", "--batch", "1", "--out", "o", "--anchor_fisher", fisher])
