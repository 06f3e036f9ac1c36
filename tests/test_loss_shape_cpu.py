"""The shaped loss on the host: the three new entry points in the header and the bindings (ABI still 12), what the plan query says the GPU test's
shape table reaches, the min-SNR table, every argument error (raised before a device is touched), and the references of loss_shape_ref.py --
the float64 one against elem_ref's, and plain torch float32 inside the very bounds the GPU test applies to the kernel."""
import argparse
import os
import re

import pytest
import torch

import elem_ref as E
import loss_shape_ref as R
from villandiffusion_amd import lib as L
from villandiffusion_amd import ops
from villandiffusion_amd import schedulers as S
from villandiffusion_amd.loss import LossFn, min_snr_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_loss_sample_fwd_bwd", "vd_loss_sample_ws_floats", "vd_loss_sample_plan")


# ------------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_and_bindings_declare_the_three_functions():
    with open(os.path.join(ROOT, "include", "villan_hip.h")) as f:
        txt = f.read()
    assert re.search(r"#define VD_ABI_VERSION 12\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.PROTOTYPES, name
    assert all(n in txt.split("Unchanged by")[1].split("*/")[0] for n in NEW), "the ABI comment lists the additions"
    lib = L.load()
    assert lib.vd_abi_version() == 12
    assert len(L.PROTOTYPES["vd_loss_sample_fwd_bwd"][1]) == 19
    with open(os.path.join(ROOT, "villandiffusion_amd", "csrc", "Makefile")) as f:
        assert "vd_loss.hip" in f.read()


# ------------------------------------------------------------------------------------------------------------------------------ the plan
def test_the_shape_table_reaches_every_edge_of_the_plan():
    cap, max_seg = R.block_cap()
    assert cap >= 256 and max_seg >= 2
    plans = {s: R.plan(*s) for s in R.all_shapes()}
    for (B, chw), (seg, blocks, ws) in plans.items():
        assert 1 <= seg <= max_seg and blocks == min(B * seg, cap) and ws == B * seg, (B, chw, seg, blocks, ws)
    segs = {p[0] for p in plans.values()}
    assert 1 in segs and 2 in segs and max_seg in segs, segs
    assert plans[(1, 196608)][0] == max_seg, "one 256 x 256 image takes the largest segment count"
    at, beyond = R.tiny_shapes()
    assert at[0] * plans[at][0] == cap == plans[at][1], "exactly at the cap"
    assert beyond[0] * plans[beyond][0] > cap == plans[beyond][1], "asked beyond the cap"
    assert any(B * p[0] < cap and p[1] == B * p[0] for (B, _), p in plans.items()), "below the cap"
    assert any(chw % 4 for _, chw in plans) and any(chw % 4 == 0 and chw > 4 for _, chw in plans)
    # the segment count never shrinks as a sample grows, and stays at the largest from there on
    seq = [R.plan(1, n)[0] for n in (1, 2048, 2049, 4096, 4097, 10 ** 5, 10 ** 6, 10 ** 9)]
    assert seq == sorted(seq) and seq[0] == 1 and seq[-1] == max_seg
    lib = L.load()
    assert lib.vd_loss_sample_ws_floats(0, 5) == 0 and lib.vd_loss_sample_ws_floats(5, 0) == 0
    with pytest.raises(L.VillanHipError):
        ops.loss_sample_plan(0, 3)


# ------------------------------------------------------------------------------------------------------------------- the min-SNR table
def _f64_table(ac32, gamma):
    ac = ac32.double()
    snr = ac / (1 - ac)
    return torch.minimum(snr, torch.tensor(float(gamma), dtype=torch.float64)) / snr, snr


def test_min_snr_table_default_linear_schedule():
    ac = S.DDPMScheduler().alphas_cumprod
    w = min_snr_table(ac, 5.0)
    ref, snr = _f64_table(ac.float(), 5.0)
    assert w.dtype == torch.float32 and w.shape == (1000,)
    assert float(((w.double() - ref).abs() / ref).max()) <= 2.0 ** -22
    assert bool((w[1:] >= w[:-1]).all()), "non-decreasing in t"
    snr32 = ac.float() / (1 - ac.float())
    assert bool((w[snr32 <= 5.0] == 1.0).all()), "exactly 1 wherever snr <= gamma"
    below = (w < 1).nonzero().flatten().tolist()
    assert below == list(range(130)), (len(below), below[:3], below[-3:])
    assert abs(float(w[0]) - 5.0013e-4) < 1e-7, float(w[0])
    assert bool((min_snr_table(ac, 1e6) == 1.0).all()), "gamma above every snr: every entry exactly 1"


def test_min_snr_table_ldm_scaled_linear():
    ac = S.DDPMScheduler(beta_start=0.0015, beta_end=0.0195, beta_schedule="scaled_linear").alphas_cumprod        # the LDM schedule (model.py)
    w = min_snr_table(ac, 5.0)
    assert int((w < 1).sum()) == 95 and bool((w[1:] >= w[:-1]).all())
    ref, _ = _f64_table(ac.float(), 5.0)
    assert float(((w.double() - ref).abs() / ref).max()) <= 2.0 ** -22


def test_lossfn_keeps_the_table_and_its_shaping():
    sched = S.DDPMScheduler()
    lf = LossFn(sched, "SDE-VP", snr_gamma=5.0)
    assert lf.shaped and lf.shaping == (5.0, 1.0, False)
    assert torch.equal(lf.snr_table(), min_snr_table(sched.alphas_cumprod, 5.0)) and lf.snr_table() is lf.snr_table()
    lf.snr_gamma = 3.0
    assert torch.equal(lf.snr_table(), min_snr_table(sched.alphas_cumprod, 3.0)), "a new gamma is a new table"
    plain = LossFn(sched, "SDE-VP")
    assert not plain.shaped and plain.snr_table() is None and plain.last_split is None and plain.last_sample_loss is None
    assert LossFn(sched, "SDE-VP", poison_weight=2.0).shaped and LossFn(sched, "SDE-VP", track_split=True).shaped
    assert LossFn(sched, "SDE-VP", "l2", 1, "sde", 1.0, 1.0, 1.0, 0.0).shaping == (None, 1.0, False), "positional calls are unchanged"


# ---------------------------------------------------------------------------------------------------------------------- argument errors
class _NoDevice:
    """A model that must never be called."""
    device = torch.device("cpu")

    def __call__(self, *a, **k):
        raise AssertionError("the model ran before the argument check")


def test_argument_errors_before_any_launch(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))
    ve, vp = S.ScoreSdeVeScheduler(), S.DDPMScheduler()
    with pytest.raises(NotImplementedError, match="snr_gamma"):
        LossFn(ve, "SDE-VE", snr_gamma=5.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="snr_gamma"):
            LossFn(vp, "SDE-VP", snr_gamma=bad)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="poison_weight"):
            LossFn(vp, "SDE-VP", poison_weight=bad)
    assert LossFn(ve, "SDE-VE", poison_weight=2.0).shaped and LossFn(vp, "SDE-VP", poison_weight=0.0).shaped
    x = torch.zeros(4, 3, 8, 8)
    t = torch.zeros(4, dtype=torch.int64)
    for kw in (dict(poison_weight=2.0), dict(track_split=True)):
        lf = LossFn(vp, "SDE-VP", **kw)
        with pytest.raises(ValueError, match="flags"):
            lf.p_loss(_NoDevice(), x, x, t, noise=x)
        with pytest.raises(ValueError, match="flags"):
            lf.p_loss_by_keys({"target": x, "pixel_values": x}, _NoDevice(), "target", "pixel_values", t, noise=x)
        with pytest.raises(ValueError, match="entries"):
            lf.p_loss(_NoDevice(), x, x, t, noise=x, is_poison=torch.zeros(3, dtype=torch.bool))
    lf = LossFn(vp, "SDE-VP", poison_weight=2.0)
    lf.poison_weight = -1.0                                    # set after construction: caught at the call
    with pytest.raises(ValueError, match="poison_weight"):
        lf.p_loss(_NoDevice(), x, x, t, noise=x, is_poison=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="sample_weight"):
        LossFn(vp, "SDE-VP").p_loss(_NoDevice(), x, x, t, noise=x, sample_weight=torch.ones(3))


def test_cli_flags_and_their_errors(tmp_path, monkeypatch):
    import VillanDiffusion as V
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))
    base = ["--project", "p", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "128", "--epoch", "1", "--result", str(tmp_path), "-o"]
    a = V.parse_args(["--mode", "train", "--snr_gamma", "5", "--poison_loss_weight", "2", "--log_loss_split"] + base)
    assert (a.snr_gamma, a.poison_loss_weight, a.log_loss_split) == (5.0, 2.0, True)
    cfg = V.setup(a)
    assert V.loss_shaping(cfg) == {"snr_gamma": 5.0, "poison_weight": 2.0, "track_split": True}
    import json
    for side in ("args.json", "config.json"):
        with open(os.path.join(cfg.output_dir, side)) as f:
            d = json.load(f)
        assert (d["snr_gamma"], d["poison_loss_weight"], d["log_loss_split"]) == (5.0, 2.0, True), side
    # resume takes them from args.json, and refuses them on its own command line
    r = V.setup(V.parse_args(["--mode", "resume", "--ckpt", cfg.output_dir]))
    assert V.loss_shaping(r) == {"snr_gamma": 5.0, "poison_weight": 2.0, "track_split": True}
    for extra in (["--snr_gamma", "5"], ["--poison_loss_weight", "2"], ["--log_loss_split"]):
        for mode in ("resume", "sampling", "measure"):
            with pytest.raises(NotImplementedError, match="isn't supported in mode"):
                V.setup(V.parse_args(["--mode", mode, "--ckpt", cfg.output_dir] + extra))
    # at their defaults the side files read as before the options existed
    plain = V.setup(V.parse_args(["--mode", "train", "--postfix", "plain"] + base))
    assert V.loss_shaping(plain) == {}
    with open(os.path.join(plain.output_dir, "config.json")) as f:
        assert not {"snr_gamma", "poison_loss_weight", "log_loss_split"} & set(json.load(f))
    with pytest.raises(NotImplementedError, match="snr_gamma"):
        V.setup(V.parse_args(["--mode", "train", "--sde_type", "SDE-VE", "--snr_gamma", "5", "--postfix", "ve"] + base))
    with pytest.raises(ValueError, match="snr_gamma"):
        V.setup(V.parse_args(["--mode", "train", "--snr_gamma", "-1", "--postfix", "neg"] + base))
    with pytest.raises(ValueError, match="poison_weight"):
        V.setup(V.parse_args(["--mode", "train", "--poison_loss_weight", "-2", "--postfix", "negw"] + base))
    assert not os.path.isdir(os.path.join(str(tmp_path), V.naming_fn(argparse.Namespace(**{**vars(plain), "postfix": "neg"})))), "an argument error creates no run directory"
    assert V.split_fields([3.0, 2.0, 0.0, 0.0]) == " loss_clean 1.50000 loss_poison n/a"
    assert V.split_fields([0.0, 0.0, 1.0, 4.0]) == " loss_clean n/a loss_poison 0.25000"


# ----------------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("kind", R.KINDS)
def test_float64_reference_is_elem_refs_when_the_weights_are_one(kind):
    for B, chw in ((1, 1), (3, 85), (5, 4099)):
        for neg in (False, True):
            pred, y, ps = R.loss_inputs(B, chw, neg)
            loss, dpred, sl, stats = R.shaped_f64(pred, y, ps, gscale=0.5, kind=kind)
            rl, rd = E.loss_f64(pred, y, ps, 0.5, kind)
            assert abs(float(loss) - float(rl)) <= 1e-15 * abs(float(rl)) and float((dpred - rd).abs().max()) <= 1e-18 + 1e-15 * float(rd.abs().max())
            assert abs(float(sl.mean()) - float(rl)) <= 1e-15 * abs(float(rl))
            assert stats.tolist()[1::2] == [float(B), 0.0] and float(stats[2]) == 0.0
            ones = R.shaped_f64(pred, y, ps, torch.ones(B), torch.ones(4), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.bool), 1.0, 0.5, kind)
            assert float(ones[0]) == float(loss) and torch.equal(ones[1], dpred)
    w = R.weights(4, torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([0.5, 0.25]), torch.tensor([-3, 0, 1, 9]), torch.tensor([True, False, True, False]), 10.0)
    assert w.tolist() == [5.0, 1.0, 7.5, 1.0], "weight * table[clamped t] * poison weight"


def test_loss_inputs_for_any_batch_keep_the_exact_differences():
    pred, y, ps = R.loss_inputs(7, 85, True)
    assert pred.shape == y.shape == (7, 85) and ps.shape == (7,)
    d = (pred.double() * ps.double()[:, None] - y.double()).flatten()
    for v in E.LOSS_D:
        assert int((d == v).sum()) >= 1, v


@pytest.mark.parametrize("kind", R.KINDS)
def test_plain_torch_float32_passes_the_very_bounds(kind):
    """What the GPU test asks of the kernel, asked of torch float32 on the host: the figures, the bounds and the report are the same objects."""
    for B, chw in ((1, 1), (3, 85), (2, 257), (7, 3072), (5, 66603)):
        weight, wtab, t, flags = R.shaping_inputs(B)
        for neg in (False, True):
            pred, y, ps = R.loss_inputs(B, chw, neg)
            loss, dpred, sl = R.shaped_torch_f32(pred, y, ps, weight, wtab, t, flags, 2.5, 0.5, kind)
            stats = torch.stack([sl[~flags].sum(), (~flags).sum().float(), sl[flags].sum(), flags.sum().float()])
            ref = R.shaped_f64(pred, y, ps, weight, wtab, t, flags, 2.5, 0.5, kind)
            bound = R.sample_loss_bound(pred, y, ps, kind, R.plan(B, chw)[0])
            E.report(f"torch f32 {kind} B={B} chw={chw} neg={neg}", R.figures(float(loss), dpred, sl, stats, ref, bound))


def test_the_bound_follows_the_reduction_shape():
    assert R.chain_terms(1, 1) == 1 + 4 + 6 + 2 + 0 + 1
    assert R.chain_terms(3072, 2) == 1 + 8 + 6 + 2 + 1 + 1
    assert R.chain_terms(196608, 64) == 1 + 12 + 6 + 2 + 63 + 1


@pytest.mark.parametrize("kind", R.KINDS)
def test_integer_inputs_are_exact_in_float32(kind):
    for B, chw in ((2, 256), (8, 2048), (2, 8192)):
        pred, y, ps, weight, wtab, t, flags = R.integer_inputs(B, chw)
        d = pred.double() * ps.double()[:, None] - y.double()
        assert float(d.abs().max()) <= 3 and bool((d == d.round()).all())
        loss, dpred, sl, stats = R.shaped_f64(pred, y, ps, weight, wtab, t, flags, 2.0, 0.5, kind)
        for v in (loss.reshape(1), sl, stats):
            assert torch.equal(v.float().double(), v), "the float64 result is a float32 number"
        assert torch.equal(R.dpred_f32(pred, y, ps, weight, wtab, t, flags, 2.0, 0.5, kind).double(), dpred), "and so is the gradient"
