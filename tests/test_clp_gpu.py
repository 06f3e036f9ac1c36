"""Channel Lipschitzness-based Pruning (villandiffusion_amd.clp) on the GPU: vd_channel_lipschitz on synthetic Lipschitz tables (the Gram
output bit for bit against the ordered f32 oracle of tests/clp_ref.py at both alignments, the eigen stage alone against float64 on the kernel's
own Gram, the whole score inside the stated bound, the refusals before any launch), `channel_lipschitz` end to end on the three families, the
planted outlier, the masked fine-tune after `clp_prune`, and tools/clp_prune.py with --keep_pruned of the driver."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clp_ref as ref  # noqa: E402
import test_clp_cpu as host  # noqa: E402
from villandiffusion_amd import anp, clp, lib, ops  # noqa: E402
from villandiffusion_amd import pipelines as P  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.actprune import PruneMask  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.U
EINVAL = -22
CINS = (1, 3, 63, 64, 65, 130, 512)
ROWS = (1, 4, 5)                                             # 1 and 5: a workgroup's last rows are absent


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def launch(ws, shift=0, scale=None, want_gram=True):
    """One vd_channel_lipschitz launch over the jobs ws = [[rows, Cin, T] f32 numpy]; every job starts on a multiple of four floats of a
    buffer whose base is `shift` floats past 16-byte alignment, three unused floats between the jobs.  NaN sentinels lie before and behind
    `out` and `gram`; `w` must keep its bits.  -> (out [n] numpy, gram [n, 45] numpy or None, the jobs)."""
    jobs, cursor, neuron, block = [], 0, 0, 0
    for w in ws:
        rows, cin, taps = w.shape
        jobs.append((cursor, rows, cin, taps, neuron, block))
        cursor = (cursor + rows * cin * taps + 3 + 3) // 4 * 4
        neuron += rows
        block += (rows + 3) // 4
    flat = torch.full((cursor + 8,), float("nan"))
    for w, j in zip(ws, jobs):
        flat[j[0]:j[0] + w.size] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32).reshape(-1))
    buf = torch.empty(flat.numel() + 4, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    wd = buf[shift:shift + flat.numel()]
    wd.copy_(flat)
    assert wd.data_ptr() % 16 == 4 * shift
    n = neuron
    out_full = torch.full((n + 8,), float("nan"), device=DEV)
    gram_full = torch.full(((n + 2) * ref.GRAM,), float("nan"), device=DEV) if want_gram else None
    out = out_full[4:4 + n]
    gram = gram_full[ref.GRAM:(n + 1) * ref.GRAM] if want_gram else None
    sd = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).to(DEV)
    ops.channel_lipschitz(wd, torch.tensor(jobs, dtype=torch.int64), out, scale=sd, gram=gram)
    torch.cuda.synchronize()
    assert torch.equal(bits(wd), bits(flat))                                      # w is untouched (NaN gaps included)
    oh = out_full.cpu()
    assert bool(torch.isnan(oh[:4]).all()) and bool(torch.isnan(oh[4 + n:]).all()) and not bool(torch.isnan(oh[4:4 + n]).any())
    gh = None
    if want_gram:
        gf = gram_full.cpu()
        assert bool(torch.isnan(gf[:ref.GRAM]).all()) and bool(torch.isnan(gf[(n + 1) * ref.GRAM:]).all())
        gh = gf[ref.GRAM:(n + 1) * ref.GRAM].view(n, ref.GRAM).numpy()
    return oh[4:4 + n].numpy(), gh, jobs


def shape_sweep(make):
    """Every (Cin, T, rows) of the issue's sweep as one job: make((rows, Cin, T)) -> f32 numpy."""
    return [make((rows, cin, taps)) for taps in (9, 1) for cin in CINS for rows in ROWS]


def check_gram(ws, gram, jobs):
    """The kernel's gram against the ordered f32 oracle, bit for bit; the slots a T = 1 row does not own are untouched."""
    for w, j in zip(ws, jobs):
        got = gram[j[4]:j[4] + j[1]]
        want = ref.gram_ordered_f32(w)
        k = want.shape[1]
        assert np.array_equal(f32bits(got[:, :k]), f32bits(want)), (w.shape,)
        assert np.isnan(got[:, k:]).all(), (w.shape,)


@pytest.fixture(scope="module")
def sweep():
    """The sweep's data (integers and normal) with one launch each at both alignments: computed once, shared."""
    gen = g(1)
    ints = shape_sweep(lambda s: torch.randint(-4, 5, s, generator=gen).float().numpy())
    real = shape_sweep(lambda s: torch.randn(s, generator=gen).numpy())
    n = sum(w.shape[0] for w in real)
    scale = torch.randn(n, generator=gen).numpy()
    runs = {("int", s): launch(ints, s) for s in (0, 1)}
    runs |= {("real", s): launch(real, s, scale=scale) for s in (0, 1)}
    return ints, real, scale, runs


# ------------------------------------------------------------------------------------------------------------------- 1. the Gram, bit for bit
def test_gram_is_the_ordered_f32_sum_bit_for_bit_at_both_alignments(sweep):
    ints, real, scale, runs = sweep
    assert len(ints) == 42 and {w.shape[1] * w.shape[2] % 4 for w in real} == {0, 1, 2, 3}      # 16-byte and scalar loads at the aligned base
    for kind, ws in (("int", ints), ("real", real)):
        for s in (0, 1):
            out, gram, jobs = runs[(kind, s)]
            check_gram(ws, gram, jobs)
        assert np.array_equal(f32bits(runs[(kind, 0)][1][~np.isnan(runs[(kind, 0)][1])]), f32bits(runs[(kind, 1)][1][~np.isnan(runs[(kind, 1)][1])]))
        assert np.array_equal(f32bits(runs[(kind, 0)][0]), f32bits(runs[(kind, 1)][0]))
    # integers: the Gram is exact whatever the order
    out, gram, jobs = runs[("int", 0)]
    for w, j in zip(ints, jobs):
        G = ref.gram64(w)
        want = np.stack([G[:, a, b] for a, b in ref.entries(w.shape[2])], axis=1)
        assert np.array_equal(gram[j[4]:j[4] + j[1], :want.shape[1]].astype(np.float64), want)
    # a second run has the same bits; without gram nothing is written there and out is the same
    again = launch(real, 0, scale=scale)
    assert np.array_equal(f32bits(again[0]), f32bits(runs[("real", 0)][0]))
    assert np.array_equal(f32bits(np.nan_to_num(again[1])), f32bits(np.nan_to_num(runs[("real", 0)][1])))
    plain = launch(real, 0, scale=scale, want_gram=False)
    assert np.array_equal(f32bits(plain[0]), f32bits(again[0]))


# ------------------------------------------------------------------------------------------------------------------- 2. the eigen stage alone
def eigen_cases():
    """[name, [rows, Cin, 9] f32]: normal rows, rank-one rows, two equal top singular values, magnitudes 1e4 and 1e-4, Cin = 1."""
    rng = np.random.default_rng(2)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Q = np.linalg.qr(rng.standard_normal((9, 9)))[0]
    eq = np.zeros((6, 64, 9))
    eq[:, 0, 0] = eq[:, 1, 1] = 3.0
    eq[:, 2, 2] = np.linspace(0.5, 2.9, 6)
    return [("normal", f(rng.standard_normal((8, 130, 9)))), ("few channels", f(rng.standard_normal((8, 3, 9)))),
            ("rank one", f(rng.standard_normal((8, 64, 1)) * rng.standard_normal((8, 1, 9)))), ("one channel", f(rng.standard_normal((8, 1, 9)))),
            ("equal top", f(eq @ Q)), ("1e4", f(rng.standard_normal((8, 65, 9)) * 1e4)), ("1e-4", f(rng.standard_normal((8, 65, 9)) * 1e-4))]


def test_eigen_stage_against_float64_on_the_kernels_own_gram():
    """The kernel's largest relative lambda error over the set must be at most the larger of the header's bound (5760.5 * 2^-24) and 4x the
    largest relative error of numpy's float32 eigvalsh on the same Grams.  Measured on MI355X (README): 6.1 * 2^-24 (3.65e-7), 1.06e-3 of the header's
    bound; LAPACK's float32 eigvalsh 0.87 * 2^-24 on the same Grams."""
    cases = eigen_cases()
    out, gram, jobs = launch([w for _, w in cases])
    worst = lapack = 0.0
    for (name, w), j in zip(cases, jobs):
        gk = gram[j[4]:j[4] + j[1]]
        G = ref.full_from_slots(gk)
        lam64 = np.linalg.eigvalsh(G)[:, -1]
        lam32 = np.linalg.eigvalsh(G.astype(np.float32))[:, -1].astype(np.float64)
        got = out[j[4]:j[4] + j[1]].astype(np.float64) ** 2
        e, e32 = float((np.abs(got - lam64) / lam64).max()), float((np.abs(lam32 - lam64) / lam64).max())
        print(f"[clp] eigen stage, {name}: kernel {e / U:.2f} u, LAPACK f32 {e32 / U:.2f} u")
        worst, lapack = max(worst, e), max(lapack, e32)
    print(f"[clp] eigen stage: largest relative lambda error {worst:.3e} ({worst / U:.2f} u), {worst / ref.EIGEN_BOUND:.2e} of the header's bound; "
          f"LAPACK f32 {lapack:.3e} ({lapack / U:.2f} u)")
    assert worst <= max(ref.EIGEN_BOUND, 4 * lapack), (worst, ref.EIGEN_BOUND, lapack)
    # the equal-top rows: sigma_max is 3 (the float64 SVD says so too)
    k = [n for n, _ in cases].index("equal top")
    assert np.abs(out[jobs[k][4]:jobs[k][4] + 6] - 3.0).max() < 1e-5


def test_eigen_stage_is_exact_where_the_gram_is_diagonal_and_for_one_tap():
    rng = np.random.default_rng(3)
    diag = np.zeros((5, 70, 9), dtype=np.float32)
    for r in range(5):
        taps = rng.integers(0, 9, 70)
        diag[r, np.arange(70), taps] = rng.standard_normal(70).astype(np.float32)          # one nonzero tap per channel
    one = rng.standard_normal((5, 130, 1)).astype(np.float32)
    zero = rng.standard_normal((5, 3, 9)).astype(np.float32)
    zero[1] = 0.0
    zero[4] = 0.0
    zero1 = rng.standard_normal((4, 65, 1)).astype(np.float32)
    zero1[2] = 0.0
    out, gram, jobs = launch([diag, one, zero, zero1])
    gd = gram[:5]
    for a, b in ref.entries(9):
        if a != b:
            assert (gd[:, ref.slot(a, b)] == 0).all()
    dmax = np.stack([gd[:, ref.slot(i, i)] for i in range(9)], axis=1).max(axis=1)
    assert np.array_equal(f32bits(out[:5]), f32bits(np.sqrt(dmax.astype(np.float32))))     # to the bits of sqrtf(max_i G_ii)
    assert np.array_equal(f32bits(out[5:10]), f32bits(np.sqrt(gram[5:10, 0].astype(np.float32))))      # T = 1: sqrtf(G_00)
    z = out[10:15]
    assert f32bits(z[[1, 4]]).tolist() == [0, 0] and (z[[0, 2, 3]] > 0).all()              # a zero row: +0.0, never NaN
    assert f32bits(out[15:19])[2] == 0 and not np.isnan(out).any()
    # with a scale the zero row stays +0.0 (the factor's sign is dropped)
    out2, _, _ = launch([zero], scale=np.array([-2.0, -3.0, 0.5, 1.0, -1.0], dtype=np.float32), want_gram=False)
    assert f32bits(out2[[1, 4]]).tolist() == [0, 0]
    assert np.array_equal(f32bits(out2[[0, 2]]), f32bits(np.array([z[0] * np.float32(2.0), z[2] * np.float32(0.5)], dtype=np.float32)))


# ------------------------------------------------------------------------------------------------------------------------- 3. the whole score
def test_whole_score_inside_the_stated_bound(sweep):
    """|UCLC - UCLC_ref| / UCLC_ref against the float64 SVD, inside 1/2 [9 (chain + 1) 2^-24 + eigen bound] + 2 * 2^-24.  Measured on MI355X
    (README): the largest error / bound is 8.2e-4 (end to end on the three small networks 1.3e-3 to 1.6e-3)."""
    ints, real, scale, runs = sweep
    out, _, jobs = runs[("real", 0)]
    worst = 0.0
    for w, j in zip(real, jobs):
        sl = slice(j[4], j[4] + j[1])
        want = ref.sigma_max64(w) * np.abs(scale[sl].astype(np.float32).astype(np.float64))
        assert ops.channel_lipschitz_plan(j[2], j[3]) == ref.chain(j[2])
        err = np.abs(out[sl].astype(np.float64) - want) / want
        bound = ref.score_bound(j[2])
        assert (err <= bound).all(), (w.shape, float(err.max()), bound)
        worst = max(worst, float(err.max()) / bound)
    print(f"[clp] whole score: largest error / bound {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------- 4. refusals before any launch
def test_einval_before_any_launch():
    h = lib.load()
    w = torch.randn(4096, device=DEV)
    out = torch.full((16,), float("nan"), device=DEV)
    good = [(0, 5, 3, 9, 0, 0), (200, 4, 7, 1, 5, 2)]

    def call(jobs, blocks, wp=None, op=None):
        ht = torch.tensor(jobs, dtype=torch.int64).reshape(-1, 6)
        dt = ht.to(DEV)
        rc = h.vd_channel_lipschitz(w.data_ptr() if wp is None else wp[0], ht.data_ptr(), dt.data_ptr(), ht.shape[0], blocks, None,
                                    out.data_ptr() if op is None else op[0], None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    for jobs, blocks, msg in (([(0, 5, 3, 4, 0, 0)], 2, "T = 4 taps"), ([good[0], (200, 4, 7, 1, 4, 2)], 3, "first neuron 4 (expected 5)"),
                              ([good[0], (200, 4, 7, 1, 5, 1)], 3, "first workgroup 1 (expected 2)"), ([(0, 0, 3, 9, 0, 0)], 1, "rows, Cin = 0, 0, 3")):
        assert call(jobs, blocks) == EINVAL and msg in lib.last_error(), lib.last_error()
    assert call(good, 3, wp=(None,)) == EINVAL and "null pointer" in lib.last_error()
    assert call(good, 3, op=(None,)) == EINVAL and "null pointer" in lib.last_error()
    assert bool(torch.isnan(out).all())                                           # nothing ran
    assert call(good, 3) == 0
    assert not bool(torch.isnan(out[:9]).any()) and bool(torch.isnan(out[9:]).all())


# ------------------------------------------------------------------------------------------------------------------ 5. end to end, 3 families
def check_family(model, net, label):
    before = bits(net.flat_param)
    st = host.state_of(net)
    worst = 0.0
    for layers in clp.LAYERS:
        for scale in clp.SCALES:
            uclc, settings = clp.channel_lipschitz(model, layers=layers, scale=scale)
            tab = clp.lipschitz_table(net, layers)
            assert list(uclc) == tab.names and settings["layers"] == layers and settings["scale"] == scale
            assert settings["n_channels"] == tab.n_neurons and settings["scale_source"] == tab.scale_source
            for name, v in uclc.items():
                want = ref.uclc_ref(st, name, scale)
                assert v.dtype == torch.float32 and v.shape == want.shape
                got = v.double().numpy()
                err = np.where(want > 0, np.abs(got - want) / np.where(want > 0, want, 1.0), np.where(got == 0, 0.0, np.inf))     # a zero row: exactly 0
                bound = ref.score_bound(net._offs[name][2][1])
                assert (err <= bound).all(), (label, layers, scale, name, float(err.max()), bound)
                worst = max(worst, float(err.max()) / bound)
    assert torch.equal(bits(net.flat_param), before)                              # the weights are bit-unchanged
    print(f"[clp] {label}: largest error / bound over resnet, conv, all x gamma, none: {worst:.3e}")


def test_channel_lipschitz_end_to_end_on_the_small_unet():
    net = host.plant(host.small(DEV))
    check_family(net, net, "small UNet")


def perturb_norms(net, seed):
    """GroupNorm weights off their initial 1, so that the gamma factor is seen."""
    gen = g(seed)
    with torch.no_grad():
        for name in net._offs:
            if ".norm" in name and name.endswith(".weight"):
                net.P[name].add_((0.1 * torch.randn(net.P[name].shape, generator=gen)).to(DEV))
    return net


def test_channel_lipschitz_end_to_end_on_ncsnpp_and_the_latent_unet():
    pp = perturb_norms(host.small_pp(DEV), 5)
    check_family(pp, pp, "small NCSN++")
    pipe = host.small_ldm(DEV)
    perturb_norms(pipe.unet, 6)
    vq_before = bits(pipe.vqvae.flat_param)
    check_family(pipe, pipe.unet, "small latent UNet")
    assert torch.equal(bits(pipe.vqvae.flat_param), vq_before)


# ------------------------------------------------------------------------------------------------------- 6. the planted outlier, the fine-tune
def oracle_flags(net, u=3.0):
    st = host.state_of(net)
    return {name: ref.outliers(ref.uclc_ref(st, name, "gamma"), u)[1] for name in clp.lipschitz_table(net).names}


def batch_of(i):
    gen = g(100 + i)
    x0 = torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1
    Rr = torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1
    Rr[::2] = 0
    eps = torch.randn(4, 3, 32, 32, generator=gen)
    t = torch.randint(0, 1000, (4,), generator=gen)
    return {"target": x0.cuda(), "pixel_values": Rr.cuda()}, t.cuda(), eps.cuda()


def test_planted_outlier_is_pruned_and_stays_zero_through_the_fine_tune():
    net = host.plant(host.small(DEV))
    flags = oracle_flags(net)
    for name, v in ref_z(net).items():
        assert float((v - 3.0).abs().min()) > 1e-3, name                          # the condition of the test (tests/test_clp_cpu.py asserts it too)
    before = host.state_of(net)
    mask = clp.clp_prune(net, u=3.0)
    assert mask.pruned == {name: int(f.sum()) for name, f in flags.items() if int(f.sum())} and mask.n_pruned >= 3
    after = host.state_of(net)
    for name in before:
        f = flags.get(name)
        if f is None:
            assert torch.equal(bits(after[name]), bits(before[name])), name       # biases and every unscored layer keep their bits
        else:
            assert bool((bits(after[name][f]) == 0).all()) and torch.equal(bits(after[name][~f]), bits(before[name][~f])), name
    for name, rows in host.PLANTED.items():
        assert all(bool(flags[name][r]) for r in rows)
    assert torch.equal(PruneMask.from_model(net).keep, mask.keep)
    # two steps of the masked fine-tune: the rows stay +0.0 bit for bit in the weights and in both moments
    tr = Trainer(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), lr=1e-3, total_steps=20, warmup_steps=0, keep_pruned=mask)
    drop = torch.zeros(net.flat_numel, dtype=torch.bool)
    for off, rows, ln, _, n0, _ in tr._keep_tab.jobs:
        for j in (mask.keep[n0:n0 + rows] == 0).nonzero().reshape(-1).tolist():
            drop[off + j * ln:off + (j + 1) * ln] = True
    assert int(drop.sum()) == sum(int(f.sum()) * before[name][0].numel() for name, f in flags.items())
    for k in range(2):
        b, t, eps = batch_of(k)
        tr.train_step(b, t, noise=eps)
        torch.cuda.synchronize()
        for buf in (tr.model.flat_param, tr.opt.exp_avg, tr.opt.exp_avg_sq):
            assert bool((bits(buf)[drop] == 0).all()), k
    assert tr.opt.step_count == 2 and float(tr.opt.exp_avg[~drop.to(DEV)].abs().sum()) > 0
    assert torch.equal(PruneMask.from_model(tr.model).keep, mask.keep)


def ref_z(net):
    st = host.state_of(net)
    return {name: ref.outliers(ref.uclc_ref(st, name, "gamma"), 3.0)[0] for name in clp.lipschitz_table(net).names}


# ------------------------------------------------------------------------------------------------------------------- 7. the tool and the driver
def _tool():
    spec = importlib.util.spec_from_file_location("clp_prune_tool", os.path.join(ROOT, "tools", "clp_prune.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_end_to_end_and_the_driver_reads_its_mask(tmp_path, capsys, monkeypatch):
    import villandiffusion_amd.dataset as D
    full_set = D.synthetic_images
    monkeypatch.setattr(D, "synthetic_images", lambda n=60000, **k: full_set(n=64, **k))
    net = host.plant(host.small(DEV))
    flags = oracle_flags(net)
    root = tmp_path / "ckpts"
    ckpt, out = str(root / "SMALL-BASE"), str(root / "SMALL-CLP")
    P.DDPMPipeline(net, S.DDPMScheduler()).save_pretrained(ckpt)
    tool = _tool()
    tool.main(["--ckpt", ckpt, "--u", "3", "--sweep", "2,3,4", "--dataset", "SYNTHETIC-CIFAR10", "--n-clean", "8", "--batch", "8", "--out", out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    info = json.load(open(os.path.join(out, "clp.json")))
    mask = PruneMask.load(out)
    want = {name: int(f.sum()) for name, f in flags.items() if int(f.sum())}
    assert info["family"] == "vp" and info["u"] == 3.0 and info["layers"] == "resnet" and info["scale"] == "gamma" and info["n_layers"] == 8
    assert info["n_channels"] == 416 and info["pruned"] == want == mask.pruned and info["pruned_total"] == mask.n_pruned == line["pruned_total"]
    assert sum(rec["pruned"] for rec in info["per_layer"].values()) == mask.n_pruned
    for name, rec in info["per_layer"].items():
        assert rec["rows"] == flags[name].numel() and rec["pruned"] == want.get(name, 0) and rec["taps"] == 9
        assert rec["scale_source"] == name.replace("conv1.weight", "norm2.weight") and rec["std"] > 0 and rec["z_max"] <= info["z_max"]
    full = anp.neuron_table(net, "all")
    for name, f in flags.items():
        assert torch.equal(mask.keep[full.slices[name]] == 0, f)
    # the sweep: counts per u from the oracle, the clean loss of the unpruned model and at each u
    z = ref_z(net)
    assert [r["u"] for r in info["sweep"]] == [2.0, 3.0, 4.0]
    assert [r["pruned"] for r in info["sweep"]] == [sum(int((v > u).sum()) for v in z.values()) for u in (2.0, 3.0, 4.0)]
    assert info["sweep"][1]["pruned"] == mask.n_pruned and info["n_clean"] == 8
    assert all(np.isfinite(r["loss"]) for r in info["sweep"]) and np.isfinite(info["loss_unpruned"])
    pruned = P.DiffusionPipeline.from_pretrained(out).unet
    assert torch.equal(PruneMask.from_model(pruned).keep, mask.keep)              # the pruned checkpoint reloads with exactly those rows zero
    # without data: no sweep losses, the same mask
    out2 = str(tmp_path / "nodata")
    tool.main(["--ckpt", ckpt, "--sweep", "3", "--out", out2])
    info2 = json.load(open(os.path.join(out2, "clp.json")))
    assert "loss" not in info2["sweep"][0] and "loss_unpruned" not in info2 and torch.equal(PruneMask.load(out2).keep, mask.keep)
    # --keep_pruned of the driver accepts the written mask
    import VillanDiffusion as V
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = os.path.join(out, "prune_mask.pt")
    cfg = V.setup(V.parse_args(["--mode", "train", "--keep_pruned", path, "--project", "p", "--dataset", "SYNTHETIC-CIFAR10", "--batch", "128",
                                "--epoch", "1", "--result", str(tmp_path / "res"), "-o"]))
    assert cfg.keep_pruned == path and torch.equal(V.keep_pruned_mask(cfg).keep, mask.keep)
