"""Activation-based channel pruning without a GPU: the tap table, the two scores against numpy, the selection and the mask on a device="cpu"
model, the refusals of `Trainer(keep_pruned=...)`, the tool's argument errors, the driver flag, and the library's new symbols with their host-only
plan -- none of them may ask for a kernel."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import actprune_ref as ref
from oracle.unet_ref import UNet2DModelRef
from villandiffusion_amd import actprune, anp, lib, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd import schedulers as S
from villandiffusion_amd.actprune import ActivationTable, ChannelStats, PruneMask
from villandiffusion_amd.loss import LossFn
from villandiffusion_amd.trainer import Trainer, check_keep_pruned
from villandiffusion_amd.unet import UNet2DModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_channel_stats_plan", "vd_channel_stats_ws_floats", "vd_channel_stats", "vd_neuron_keep_rows")
EINVAL = -22


def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


# ----------------------------------------------------------------------------------------------------------------------------------- the table
def test_activation_table_small_and_default(monkeypatch):
    _no_kernels(monkeypatch)
    small = UNet2DModel(**ref.SMALL, device="cpu")
    tab = actprune.activation_table(small)
    names, slices, n = tab
    assert names == ["down_blocks.0.resnets.0.conv1.weight", "down_blocks.1.resnets.0.conv1.weight", "mid_block.resnets.0.conv1.weight",
                     "mid_block.resnets.1.conv1.weight", "up_blocks.0.resnets.0.conv1.weight", "up_blocks.0.resnets.1.conv1.weight",
                     "up_blocks.1.resnets.0.conv1.weight", "up_blocks.1.resnets.1.conv1.weight"]
    assert [slices[k].stop - slices[k].start for k in names] == [32, 64, 64, 64, 64, 64, 32, 32] and n == 416
    assert [slices[k].start for k in names] == [0, 32, 96, 160, 224, 288, 352, 384]
    conv = anp.neuron_table(small, "conv").slices
    assert set(names) <= set(conv) and set(names) <= set(anp.neuron_table(small, "all").slices)
    assert names == [k for k, _ in ref.resnet_blocks(UNet2DModelRef(**ref.SMALL))]     # the oracle's hooks fire in the same order
    big = UNet2DModel(device="cpu")                                                     # the CIFAR10 network
    bt = actprune.activation_table(big)
    assert len(bt.names) == 22 and bt.n_channels == 4992
    assert set(bt.names) <= set(anp.neuron_table(big, "conv").slices)
    for name in bt.names:
        assert big._offs[name][2][0] == bt.slices[name].stop - bt.slices[name].start
    # the families that are not built say so
    from villandiffusion_amd.ncsnpp import NCSNppModel
    import anp_families_ref as fam
    with pytest.raises(NotImplementedError, match="NCSNppModel is not built.*tape layout"):
        actprune.activation_table(NCSNppModel(**dict(fam.SMALL_PP, layers_per_block=1), device="cpu"))
    with pytest.raises(TypeError, match="UNet2DModel or LDMPipeline"):
        actprune.activation_table(torch.nn.Linear(2, 2))


# --------------------------------------------------------------------------------------------------------------------------------- the scores
def synthetic_stats(seed, zero_var_channel=None, act="silu_gn", counts=(40, 10)):
    tab = ActivationTable(["a.conv1.weight", "b.conv1.weight"], {"a.conv1.weight": slice(0, 5), "b.conv1.weight": slice(5, 8)}, 8)
    rng = np.random.default_rng(seed)
    n = np.array([counts[0]] * 5 + [counts[1]] * 3, dtype=np.float64)
    mean, std = rng.normal(size=8), rng.uniform(0.1, 2.0, size=8)
    if zero_var_channel is not None:
        std[zero_var_channel] = 0.0
    return ChannelStats(table=tab, count={"a.conv1.weight": counts[0], "b.conv1.weight": counts[1]}, sum=mean * n,
                        sumsq=(std ** 2 + mean ** 2) * n, act=act), n


def test_scores_against_numpy():
    clean, n = synthetic_stats(1, zero_var_channel=3)
    trig, _ = synthetic_stats(2)
    assert np.allclose(clean.mean(), clean.sum / n) and np.allclose(clean.rms() ** 2, clean.sumsq / n)
    assert clean.var()[3] <= 1e-12 and (clean.var() >= 0).all()
    pl = clean.per_layer("b.conv1.weight")
    assert pl["count"] == 10 and np.array_equal(pl["sum"], clean.sum[5:8]) and np.array_equal(pl["rms"], clean.rms()[5:8])
    d = actprune.dormancy_scores(clean)
    want = ref.dormancy_np(clean.sumsq, n)
    assert list(d) == clean.table.names and d["a.conv1.weight"].dtype == torch.float32
    assert np.allclose(torch.cat(list(d.values())).numpy(), want, rtol=1e-6, atol=0)
    s = actprune.sensitivity_scores(clean, trig)
    want = ref.sensitivity_np(clean.sum, clean.sumsq, trig.sum, n)
    got = torch.cat(list(s.values())).numpy()
    assert np.allclose(got, want, rtol=1e-6, atol=0) and (got <= 0).all() and np.isfinite(got).all()
    # the zero-variance channel: finite, |dmean| / sqrt(eps), and the most sensitive of all here
    assert abs(got[3] + abs(trig.mean()[3] - clean.mean()[3]) / np.sqrt(max(clean.var()[3], 0) + 1e-6)) <= 1e-3 * abs(got[3])
    assert got.argmin() == 3
    s2 = actprune.sensitivity_scores(clean, trig, eps=1e-2)
    assert abs(float(s2["a.conv1.weight"][3])) < abs(got[3])
    # identical statistics: no channel is sensitive
    assert float(torch.cat(list(actprune.sensitivity_scores(clean, clean).values())).abs().max()) == 0.0


def test_mismatched_stats_raise():
    clean, _ = synthetic_stats(1)
    with pytest.raises(ValueError, match="different counts"):
        actprune.sensitivity_scores(clean, synthetic_stats(2, counts=(40, 12))[0])
    with pytest.raises(ValueError, match="different activations"):
        actprune.sensitivity_scores(clean, synthetic_stats(2, act="raw")[0])
    other, _ = synthetic_stats(2)
    other.table = ActivationTable(["a.conv1.weight", "c.conv1.weight"], {"a.conv1.weight": slice(0, 5), "c.conv1.weight": slice(5, 8)}, 8)
    other.count = {"a.conv1.weight": 40, "c.conv1.weight": 10}
    with pytest.raises(ValueError, match="different tables"):
        actprune.sensitivity_scores(clean, other)
    with pytest.raises(ValueError, match="eps"):
        actprune.sensitivity_scores(clean, clean, eps=0.0)


# ------------------------------------------------------------------------------------------------------------------------------ the selection
def scores_for(net, seed=3):
    tab = actprune.activation_table(net)
    gen = ref.g(seed)
    return tab, {name: torch.rand(tab.slices[name].stop - tab.slices[name].start, generator=gen) + 0.5 for name in tab.names}


def test_fine_prune_mask_round_trip_and_from_model(tmp_path, monkeypatch):
    _no_kernels(monkeypatch)
    net = UNet2DModel(**ref.SMALL, device="cpu")
    net.reset_parameters(seed=1)
    before = net.flat_param.detach().clone()
    tab, scores = scores_for(net)
    full = anp.neuron_table(net, "all")
    mask = actprune.fine_prune(net, scores, fraction=0.1)
    k = int(0.1 * tab.n_channels)
    assert mask.n_pruned == k == sum(mask.pruned.values()) and tuple(mask.keep.shape) == (full.n_neurons,)
    flat = torch.cat([scores[n] for n in tab.names])
    cut = torch.sort(flat).values[k - 1]
    changed = torch.zeros(net.flat_numel, dtype=torch.bool)
    for name in tab.names:
        w = net.P[name].detach()
        zero = (w.reshape(w.shape[0], -1) == 0).all(1)
        assert torch.equal(zero, scores[name] <= cut), name                      # exactly the smallest scores
        assert torch.equal(mask.keep[full.slices[name]] == 0, zero)
        off, n, shape = net._offs[name]
        rows = changed[off:off + n].view(shape[0], -1)
        rows[zero] = True
    assert torch.equal(net.flat_param.detach()[~changed].view(torch.int32), before[~changed].view(torch.int32))     # every other float keeps its bits
    assert float(net.flat_param.detach()[changed].abs().sum()) == 0.0 and int(changed.sum()) > 0
    outside = torch.ones(full.n_neurons, dtype=torch.bool)
    for name in tab.names:
        outside[full.slices[name]] = False
    assert bool((mask.keep[outside] == 1).all())
    # from_model finds exactly the zeroed rows
    found = PruneMask.from_model(net)
    assert torch.equal(found.keep, mask.keep) and found.pruned == mask.pruned
    assert torch.equal(PruneMask.from_model(net, tab.names).keep, mask.keep)
    assert PruneMask.from_model(net, tab.names[:1]).n_pruned == mask.pruned.get(tab.names[0], 0)
    with pytest.raises(ValueError, match="no neuron layer"):
        PruneMask.from_model(net, ["conv_out.weight"])
    # the file
    path = mask.save(str(tmp_path))
    assert os.path.basename(path) == "prune_mask.pt"
    for src in (path, str(tmp_path)):
        back = PruneMask.load(src)
        assert torch.equal(back.keep, mask.keep) and back.pruned == mask.pruned and back.keep.dtype == torch.float32
    torch.save({"keep": torch.tensor([0.0, 0.5])}, str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="zeros and ones"):
        PruneMask.load(str(tmp_path / "bad.pt"))
    torch.save(torch.zeros(3), str(tmp_path / "worse.pt"))
    with pytest.raises(ValueError, match="no prune mask"):
        PruneMask.load(str(tmp_path / "worse.pt"))
    # a threshold selects by value
    net2 = UNet2DModel(**ref.SMALL, device="cpu")
    net2.reset_parameters(seed=1)
    m2 = actprune.fine_prune(net2, scores, threshold=0.5 * (float(cut) + float(torch.sort(flat).values[k])))     # between the k-th and the next
    assert torch.equal(m2.keep, mask.keep)


def test_a_selection_that_empties_a_layer_raises_before_anything_is_written(monkeypatch):
    _no_kernels(monkeypatch)
    net = UNet2DModel(**ref.SMALL, device="cpu")
    net.reset_parameters(seed=1)
    before = net.flat_param.detach().clone()
    tab, scores = scores_for(net)
    scores[tab.names[0]] = torch.zeros_like(scores[tab.names[0]])                # all 32 channels of the first block score lowest
    with pytest.raises(ValueError, match=f"prunes every neuron of {tab.names[0]}"):
        actprune.fine_prune(net, scores, fraction=0.1)
    with pytest.raises(ValueError, match="exactly one of threshold and fraction"):
        actprune.fine_prune(net, scores)
    with pytest.raises(ValueError, match="exactly one of threshold and fraction"):
        actprune.fine_prune(net, scores, fraction=0.1, threshold=0.1)
    assert torch.equal(net.flat_param.detach().view(torch.int32), before.view(torch.int32))


# --------------------------------------------------------------------------------------------------------------------------- trainer refusals
def test_trainer_refusals_come_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    from villandiffusion_amd.lora import LoRAConfig
    from villandiffusion_amd.trainer import SAMConfig
    net = UNet2DModel(**ref.SMALL, device="cpu")
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    mask = PruneMask(keep=torch.ones(anp.neuron_table(net, "all").n_neurons), pruned={})
    kw = dict(lr=1e-3, total_steps=10)
    with pytest.raises(ValueError, match="keep_pruned together with lora is not built"):
        Trainer(net, lf, lora=LoRAConfig(r=4), keep_pruned=mask, **kw)
    with pytest.raises(ValueError, match="keep_pruned together with sam is not built"):
        Trainer(net, lf, sam=SAMConfig(rho=0.05), keep_pruned=mask, **kw)
    with pytest.raises(TypeError, match="PruneMask"):
        Trainer(net, lf, keep_pruned=torch.ones(3), **kw)
    with pytest.raises(NotImplementedError, match="keep_pruned in a process group of more than one rank is not built"):
        check_keep_pruned(mask, world=2)
    assert check_keep_pruned(None, lora=object(), sam=object(), world=8) is None
    assert check_keep_pruned(mask) is None


# --------------------------------------------------------------------------------------------------------------------------- tool and driver
def test_tool_argument_errors(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("fine_prune_tool", os.path.join(ROOT, "tools", "fine_prune.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--ckpt", "nowhere", "--dataset", "SYNTHETIC-CIFAR10", "--out", "nowhere-out"]

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            tool.main(base + argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err

    refused(["--score", "sensitivity", "--fraction", "0.1"], "--score sensitivity needs --trigger: the score is how far")
    refused([], "one of the arguments --fraction --threshold is required")
    refused(["--fraction", "0.1", "--threshold", "0.2"], "not allowed with argument")
    refused(["--fraction", "1.0"], "--fraction must lie in [0, 1)")
    refused(["--fraction", "0.1", "--sweep", "0.1,x"], "--sweep takes comma-separated fractions")
    refused(["--fraction", "0.1", "--sweep", "1.5"], "--sweep takes fractions in [0, 1)")
    refused(["--fraction", "0.1", "--trigger", "t.pt"], "--trigger is read by --score sensitivity only")
    refused(["--fraction", "0.1", "--n-clean", "0"], "must be positive")
    refused(["--fraction", "0.1", "--score", "anp"], "invalid choice")


def test_driver_flag_reaches_args_json(tmp_path, monkeypatch):
    import VillanDiffusion as V
    import rm_backdoor_VillanDiffusion as RM
    _no_kernels(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("VILLAN_MIXED_PRECISION", raising=False)
    assert RM.main is V.main
    net = UNet2DModel(**ref.SMALL, device="cpu")
    mask = PruneMask(keep=torch.ones(anp.neuron_table(net, "all").n_neurons), pruned={})
    mask.keep[3] = 0.0
    path = mask.save(str(tmp_path))
    base = ["--project", "p", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--result", str(tmp_path / "res"), "-o"]
    a = V.parse_args(["--mode", "train", "--keep_pruned", path] + base)
    assert a.keep_pruned == path and V.parse_args(["--mode", "train"]).keep_pruned is None
    cfg = V.setup(a)
    got = V.keep_pruned_mask(cfg)
    assert torch.equal(got.keep, mask.keep)
    for side in ("args.json", "config.json"):
        with open(os.path.join(cfg.output_dir, side)) as f:
            assert json.load(f)["keep_pruned"] == path, side
    # resume takes it from args.json, and refuses it on its own command line; sampling reads no mask
    r = V.setup(V.parse_args(["--mode", "resume", "--ckpt", cfg.output_dir]))
    assert r.keep_pruned == path and torch.equal(V.keep_pruned_mask(r).keep, mask.keep)
    assert V.keep_pruned_mask(V.setup(V.parse_args(["--mode", "sampling", "--ckpt", cfg.output_dir]))) is None
    for mode in ("resume", "sampling", "measure"):
        with pytest.raises(NotImplementedError, match="isn't supported in mode"):
            V.setup(V.parse_args(["--mode", mode, "--ckpt", cfg.output_dir, "--keep_pruned", path]))
    # without the flag the side files read as before the option existed
    plain = V.setup(V.parse_args(["--mode", "train", "--postfix", "plain"] + base))
    assert V.keep_pruned_mask(plain) is None
    with open(os.path.join(plain.output_dir, "config.json")) as f:
        assert "keep_pruned" not in json.load(f)

    def refused(exc, match, extra, tag):
        with pytest.raises(exc, match=match):
            V.setup(V.parse_args(["--mode", "train", "--postfix", tag] + extra + base))
        name = V.naming_fn(V.TrainingConfig(**{**{k: v for k, v in vars(plain).items() if k in V.TrainingConfig.__dataclass_fields__}, "postfix": tag}))
        assert not os.path.isdir(os.path.join(str(tmp_path / "res"), name)), f"{tag}: an argument error creates no run directory"

    refused(FileNotFoundError, "missing.pt", ["--keep_pruned", str(tmp_path / "missing.pt")], "missing")
    refused(ValueError, "lora", ["--keep_pruned", path, "--lora_r", "4"], "lora")
    refused(ValueError, "sam", ["--keep_pruned", path, "--sam_rho", "0.05"], "sam")
    refused(NotImplementedError, "more than one", ["--keep_pruned", path, "--gpu", "0,1"], "gpus")


# ------------------------------------------------------------------------------------------------------------------------------- the library
def test_header_prototypes_makefile_and_abi():
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    assert "#define VD_ABI_VERSION 12" in hdr and lib.load().vd_abi_version() == 12           # new functions only: the version stays
    for name, n_args in zip(NEW, (6, 2, 9, 6)):
        assert f" {name}(" in hdr and len(lib.PROTOTYPES[name][1]) == n_args and hasattr(lib.load(), name), name
    for fn in ("channel_stats_plan", "channel_stats_table", "channel_stats", "neuron_keep_rows"):
        assert callable(getattr(ops, fn))
    assert "ceil(L / 64) + 8 + (S - 1)" in hdr and "z = fma((x - mean[b][g]) * rstd[b][g], gamma[c], beta[c])" in hdr
    mk = open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")).read()
    assert "vd_actstat.hip" in mk and mk.split("vd_actstat.o: vd_actstat.hip")[1].split("\n\n")[0].count("-ffp-contract=off") == 1


def chain_of(B, HW):
    """The header's formula: ceil(L / 64) + 8 + (S - 1), L = ceil(B * I / S), I = ceil(HW / 4), S = clamp(ceil(B * I / 1024), 1, 256)."""
    items = B * (-(-HW // 4))
    S_ = min(max(-(-items // 1024), 1), 256)
    L_ = -(-items // S_)
    return -(-L_ // 64) + 8 + (S_ - 1), S_


def test_channel_stats_plan_is_host_only(monkeypatch):
    _no_kernels(monkeypatch)
    assert ops.channel_stats_plan(1, 1, 1) == (1, 1, 9)
    for B, Cc, HW in ((3, 8, 16), (2, 6, 49), (5, 32, 256), (128, 128, 1024), (128, 512, 16), (4, 3, 65536), (1, 1, 4 * 1024), (1, 1, 4 * 1024 + 1),
                      (64, 128, 65536)):
        wg, seg, chain = ops.channel_stats_plan(B, Cc, HW)
        want_chain, want_seg = chain_of(B, HW)
        assert (seg, chain) == (want_seg, want_chain) and wg == -(-Cc * seg // 4), (B, Cc, HW)
    assert ops.channel_stats_plan(1, 1, 4 * 1024)[1] == 1 and ops.channel_stats_plan(1, 1, 4 * 1024 + 1)[1] == 2      # where a channel is first cut
    assert ops.channel_stats_plan(128, 128, 65536)[1] == 256                                                           # the cap
    wg, seg, ch = C.c_int32(), C.c_int32(), C.c_int64()
    h = lib.load()
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert h.vd_channel_stats_plan(*bad, C.byref(wg), C.byref(seg), C.byref(ch)) == EINVAL
    assert h.vd_channel_stats_plan(1, 1, 1, None, C.byref(seg), C.byref(ch)) == EINVAL


def test_channel_stats_refusals_are_host_side():
    """Every VD_EINVAL of vd_channel_stats comes from the host copy of the table, before any launch: they return without a device."""
    h = lib.load()
    fake = 0x1000                                             # never dereferenced: every call below is refused first
    good = [fake, fake, fake, fake, fake, 2, 8, 16, 2, 0, 0]

    def call(rows, act=1, n_jobs=None, out=fake, ws=fake, out_channels=1 << 20):
        t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 11)
        return h.vd_channel_stats(t.data_ptr(), fake, len(rows) if n_jobs is None else n_jobs, act, out, out_channels, ws, 1 << 20, None)

    assert call([good], n_jobs=0) == EINVAL and "n_jobs" in lib.last_error()
    assert call([good], act=2) == EINVAL
    bad_g = list(good); bad_g[8] = 3
    assert call([bad_g]) == EINVAL and "no multiple of G" in lib.last_error()
    for k in (1, 2, 3, 4):
        null = list(good); null[k] = 0
        assert call([null]) == EINVAL and "act = 1 needs" in lib.last_error()
    nox = list(good); nox[0] = 0
    assert call([nox], act=0) == EINVAL
    second = list(good); second[9] = 4; second[10] = 2        # overlaps the first job's channels
    assert call([good, second]) == EINVAL and "first channel" in lib.last_error()
    second[9] = 8; second[10] = 3                             # wrong first workgroup (the first job owns 2)
    assert call([good, second]) == EINVAL
    assert call([good], out_channels=7) == EINVAL and "out holds" in lib.last_error()
    assert call([good], out=None) == EINVAL
    assert h.vd_channel_stats_ws_floats(None, 1) == -1
    t = torch.tensor([good], dtype=torch.int64)
    assert h.vd_channel_stats_ws_floats(t.data_ptr(), 1) == 0
    long = list(good); long[5] = 1; long[7] = 4 * 1024 + 4    # one image of 1025 items, cut in two: 8 channels x 2 segments = 4 workgroups of 8 floats
    t = torch.tensor([long], dtype=torch.int64)
    assert h.vd_channel_stats_ws_floats(t.data_ptr(), 1) == 32
    assert h.vd_neuron_keep_rows(None, fake, 1, 1, fake, None) == EINVAL
    assert h.vd_neuron_keep_rows(fake, fake, 0, 1, fake, None) == EINVAL and h.vd_neuron_keep_rows(fake, fake, 1, 0, fake, None) == EINVAL
