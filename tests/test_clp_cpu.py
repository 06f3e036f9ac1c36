"""Channel Lipschitzness-based Pruning (villandiffusion_amd.clp) without a GPU: the Lipschitz table of the three families, the oracle of
tests/clp_ref.py against torch and float64, the outlier rule, the scores as a `prune_neurons` selection, the mask round trip, the planted
outlier's margin, every refusal, and the library's new symbols with their host-only checks."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import anp_families_ref as fam
import clp_ref as ref
from villandiffusion_amd import actprune, anp, clp, lib, ops
from villandiffusion_amd import pipelines as P
from villandiffusion_amd import schedulers as S
from villandiffusion_amd.actprune import PruneMask
from villandiffusion_amd.ncsnpp import NCSNppModel
from villandiffusion_amd.unet import UNet2DModel
from villandiffusion_amd.vqmodel import VQModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # tests/test_anp_gpu.py's
VQ_NET = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3,
              down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2, sample_size=16)
EINVAL = -22

# the planted outlier of tests/test_clp_gpu.py: two rows of one conv1 and one row of another, times 10
PLANT_SEED = 1
PLANTED = {"mid_block.resnets.0.conv1.weight": (5, 40), "up_blocks.1.resnets.1.conv1.weight": (17,)}


def small(device="cpu", seed=1):
    net = UNet2DModel(**SMALL, device=device)
    net.reset_parameters(seed=seed)
    return net


def small_pp(device="cpu"):
    net = NCSNppModel(**dict(fam.SMALL_PP, layers_per_block=1), device=device)
    net.reset_parameters(seed=2)
    return net


def small_ldm(device="cpu"):
    unet, vq = UNet2DModel(**fam.SMALL_LDM, device=device), VQModel(**VQ_NET, device=device)
    unet.reset_parameters(seed=3)
    vq.reset_parameters(seed=2)
    return P.LDMPipeline(vqvae=vq, unet=unet, scheduler=S.DDIMScheduler())


def plant(net, gen_seed=PLANT_SEED):
    """Norm weights off their initial 1 (so that the gamma factor is seen), then the planted rows times 10."""
    gen = torch.Generator().manual_seed(gen_seed)
    with torch.no_grad():
        for name in net._offs:
            if ".norm" in name and name.endswith(".weight"):
                net.P[name].add_((0.1 * torch.randn(net.P[name].shape, generator=gen)).to(net.P[name].device))
        for name, rows in PLANTED.items():
            for r in rows:
                net.P[name][r] *= 10.0
    return net


def state_of(net):
    return {k: net.flat_param[off:off + n].view(shape).detach().cpu().clone() for k, (off, n, shape) in net._offs.items()}


# --------------------------------------------------------------------------------------------------------------------------------- the table
def check_jobs(tab, net):
    neuron = block = 0
    for name, (off, rows, cin, taps, n0, b0) in zip(tab.names, tab.jobs):
        shape = net._offs[name][2]
        assert (off, rows, cin) == (net._offs[name][0], shape[0], shape[1]) and taps == int(np.prod(shape[2:])) == tab.taps[name]
        assert (n0, b0) == (neuron, block) and tab.slices[name] == slice(neuron, neuron + rows)
        neuron += rows
        block += (rows + 3) // 4
    assert (tab.n_neurons, tab.total_blocks, tab.n_jobs) == (neuron, block, len(tab.names))
    assert tab.host_table().shape == (len(tab.names), 6) and tab.host_table().dtype == torch.int64


def test_the_table_of_the_small_unet():
    net = small()
    res = clp.lipschitz_table(net)
    assert res.layers == "resnet" and res.names == actprune.activation_table(net).names and len(res.names) == 8
    assert all(res.taps[n] == 9 and res.scale_source[n] == n.replace("conv1.weight", "norm2.weight") for n in res.names)
    assert res.n_neurons == 416
    check_jobs(res, net)
    for layers in ("conv", "all"):
        tab = clp.lipschitz_table(net, layers)
        assert tab.names == list(anp.neuron_table(net, layers).slices) and tab.n_neurons == anp.neuron_table(net, layers).n_neurons
        check_jobs(tab, net)
        assert {n for n, s in tab.scale_source.items() if s is not None} == set(res.names)
        assert set(tab.taps.values()) == {1, 9}
    allt = clp.lipschitz_table(net, "all")
    assert allt.taps["time_embedding.linear_1.weight"] == 1 and allt.taps["down_blocks.1.attentions.0.to_q.weight"] == 1
    assert allt.taps["down_blocks.1.resnets.0.conv_shortcut.weight"] == 1 and allt.taps["conv_in.weight"] == 9
    assert "conv_out.weight" not in allt.slices


def test_the_table_of_ncsnpp_and_of_the_latent_unet():
    pp = small_pp()
    res = clp.lipschitz_table(pp)
    assert res.names == [n for n, s, _ in pp._layout if n.endswith(".conv1.weight")] and len(res.names) == 15
    assert "down_blocks.0.resnet_down.conv1.weight" in res.names and "up_blocks.0.resnet_up.conv1.weight" in res.names
    assert all(res.scale_source[n] == n.replace("conv1.weight", "norm2.weight") and res.scale_source[n] in pp._offs for n in res.names)
    check_jobs(res, pp)
    allt = clp.lipschitz_table(pp, "all")
    assert allt.names == list(anp.neuron_table(pp, "all").slices) and not set(fam.HEADS) & set(allt.names)
    assert allt.taps["down_blocks.0.skip_conv.weight"] == 1 and allt.scale_source["down_blocks.0.skip_conv.weight"] is None
    check_jobs(allt, pp)
    pipe = small_ldm()
    for layers in clp.LAYERS:
        a, b = clp.lipschitz_table(pipe, layers), clp.lipschitz_table(pipe.unet, layers)
        assert a.jobs == b.jobs and a.names == b.names
        check_jobs(a, pipe.unet)
    assert clp.lipschitz_table(pipe).names == actprune.activation_table(pipe).names


# -------------------------------------------------------------------------------------------------------------------------------- the oracle
def test_the_oracle_sigma_max_is_torch_svdvals():
    gen = torch.Generator().manual_seed(4)
    for Cin in (1, 3, 65, 130):
        w = torch.randn(6, Cin, 9, generator=gen)
        want = torch.linalg.svdvals(w.double())[:, 0].numpy()
        got = ref.sigma_max64(w.numpy())
        assert np.abs(got - want).max() <= 1e-12 * want.max()
    w = torch.randn(5, 70, 1, generator=gen)
    assert np.abs(ref.sigma_max64(w.numpy()) - w.double().reshape(5, -1).norm(dim=1).numpy()).max() <= 1e-12 * 10


def test_the_ordered_f32_gram_lies_inside_its_chain_bound():
    gen = torch.Generator().manual_seed(5)
    for Cin, T in ((1, 9), (3, 9), (63, 9), (64, 9), (65, 9), (130, 9), (512, 9), (130, 1), (512, 1)):
        w = torch.randn(5, Cin, T, generator=gen).numpy()
        got = ref.gram_ordered_f32(w).astype(np.float64)
        G, A = ref.gram64(w), ref.gram_abs64(w)
        for e, (i, j) in enumerate(ref.entries(T)):
            assert (np.abs(got[:, e] - G[:, i, j]) <= ref.chain(Cin) * ref.U * A[:, i, j]).all(), (Cin, T, i, j)
        assert got.shape == (5, T * (T + 1) // 2)
    assert [ref.slot(i, j) for i, j in ref.entries(9)] == list(range(45)) and ref.chain(1) == 7 and ref.chain(65) == 8
    # integers: every order gives the same bits
    w = torch.randint(-4, 5, (3, 130, 9), generator=gen).float().numpy()
    assert np.array_equal(ref.gram_ordered_f32(w), np.stack([ref.gram64(w)[:, i, j] for i, j in ref.entries(9)], axis=1).astype(np.float32))


def test_the_jacobi_schedule_converges_inside_its_sweeps():
    """The numpy restatement of the header's eigen stage: every case is done well inside 8 sweeps (288 rotations), the off-diagonal rest is below
    2^-26 lambda_max, a diagonal matrix comes back exactly, and the error is far inside the header's worst-case bound."""
    rng = np.random.default_rng(0)
    rows = [rng.standard_normal((4, 130, 9)), rng.standard_normal((4, 1, 9)), rng.standard_normal((3, 64, 1)) * rng.standard_normal((3, 1, 9)),
            rng.standard_normal((3, 65, 9)) * 1e4, rng.standard_normal((3, 65, 9)) * 1e-4]
    eq = np.zeros((2, 64, 9))
    eq[:, 0, 0] = eq[:, 1, 1] = 3.0
    eq[:, 2, 2] = 1.0
    rows.append(eq @ np.linalg.qr(rng.standard_normal((9, 9)))[0])
    worst = 0.0
    for w in rows:
        g = ref.gram_ordered_f32(w.astype(np.float32))
        lam64 = np.linalg.eigvalsh(ref.full_from_slots(g))[:, -1]
        for r in range(len(g)):
            lam, done, off = ref.jacobi_lambda_max_f32(g[r])
            assert done <= 36 * 6 and off < 2.0 ** -26
            worst = max(worst, abs(float(lam) - lam64[r]) / lam64[r])
    assert worst <= 16 * ref.U < ref.EIGEN_BOUND
    d = np.zeros(45, dtype=np.float32)
    for i in range(9):
        d[ref.slot(i, i)] = np.float32(0.3 + i * 0.37)
    assert ref.jacobi_lambda_max_f32(d) == (d.max(), 0, 0.0)
    assert ref.jacobi_lambda_max_f32(np.zeros(45, dtype=np.float32))[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------------- the rule
def test_the_rule():
    x = torch.tensor([1.0, 1.1, 0.9, 1.05, 0.95, 1.0, 1.02, 0.98, 1.0, 1.01, 0.99, 1.0, 1.03, 0.97, 1.0, 9.0])
    z = clp.clp_z({"a": x})["a"]
    want = (x.double() - x.double().mean()) / torch.std(x.double())                # unbiased
    assert z.dtype == torch.float64 and torch.allclose(z, want, rtol=0, atol=1e-12)
    assert abs(float(z[-1]) - 15 / 4.0) < 0.02                                     # close to the largest reachable (n - 1) / sqrt(n) at n = 16
    rz, flagged = ref.outliers(x.numpy(), 3.0)
    assert torch.equal(rz > 3.0, z > 3.0) and flagged.tolist() == [False] * 15 + [True]
    # strict: u equal to the largest z flags nothing, the next double below flags it
    name = "mid_block.resnets.0.conv1.weight"
    uc = {name: torch.ones(64)}
    uc[name][:16] = x.float()
    ztop = float(clp.clp_z(uc)[name].max())
    assert clp.layer_statistics(uc, ztop)[name]["pruned"] == 0 and clp.layer_statistics(uc, np.nextafter(ztop, 0))[name]["pruned"] == 1
    # zero rows: out of the statistics, never flagged, score +inf
    y = torch.cat([x, torch.zeros(4)])
    zy = clp.clp_z({"a": y})["a"]
    assert torch.equal(zy[:16], z) and bool(torch.isneginf(zy[16:]).all())
    s = clp.clp_scores({"a": y})["a"]
    assert torch.equal(s[:16], -z) and bool(torch.isposinf(s[16:]).all())
    assert ref.outliers(y.numpy(), -1e9)[1][16:].tolist() == [False] * 4
    # fewer than two live rows, or no spread: nothing is flagged at any u
    for v in (torch.tensor([0.0, 5.0, 0.0]), torch.tensor([2.0, 2.0, 2.0, 2.0]), torch.tensor([7.0])):
        zz = clp.clp_z({"a": v})["a"]
        assert bool(((zz == 0) | torch.isneginf(zz)).all()) and not bool((zz > 0).any())
        assert torch.equal(zz, ref.outliers(v.numpy(), 3.0)[0])
    rec = clp.layer_statistics({"a": y}, 3.0)["a"]
    assert rec["rows"] == 20 and rec["live"] == 16 and rec["pruned"] == 1 and abs(rec["std"] - float(torch.std(x.double()))) < 1e-12


def oracle_uclc(net, layers="resnet", scale="gamma"):
    st = state_of(net)
    return {name: torch.from_numpy(ref.uclc_ref(st, name, scale)) for name in clp.lipschitz_table(net, layers).names}


def test_scores_feed_the_selection_and_the_mask_round_trips(tmp_path):
    net = plant(small())
    uclc = oracle_uclc(net)
    scores = clp.clp_scores(uclc)
    full, dropped, picks = anp._selection("test", net, scores, threshold=-3.0)
    assert set(picks) == set(uclc) and int(dropped.sum()) == sum(int(v.numel()) for v in picks.values()) >= 3
    anp._selection("test", net, scores, fraction=0.05)
    before = state_of(net)
    mask = clp.clp_prune(net, u=3.0, uclc=uclc)                                   # plain torch writes: a device="cpu" model will do
    flagged = {name: ref.outliers(uclc[name].numpy(), 3.0)[1] for name in uclc}
    assert mask.pruned == {name: int(f.sum()) for name, f in flagged.items() if int(f.sum())}
    for name, rows in PLANTED.items():
        assert all(bool(flagged[name][r]) for r in rows)
    after = state_of(net)
    for name in before:
        if name in flagged:
            assert bool((after[name][flagged[name]] == 0).all()) and torch.equal(after[name][~flagged[name]], before[name][~flagged[name]])
        else:
            assert torch.equal(after[name], before[name])                         # biases and every other layer keep their bits
    assert torch.equal(PruneMask.from_model(net).keep, mask.keep) and mask.keep.numel() == anp.neuron_table(net, "all").n_neurons
    path = mask.save(str(tmp_path))
    again = PruneMask.load(path)
    assert torch.equal(again.keep, mask.keep) and again.pruned == mask.pruned and again.n_pruned == mask.n_pruned
    # a second pruning: the zero rows are left out and nothing new is flagged by them
    z2 = clp.clp_z(oracle_uclc(net))
    for name, f in flagged.items():
        assert bool(torch.isneginf(z2[name][f]).all())


def test_no_oracle_z_of_the_planted_network_lies_near_u():
    """The condition of the planted-outlier test on the GPU, on the oracle alone: a pass there cannot hide a tie."""
    net = plant(small())
    for layers, scale in (("resnet", "gamma"), ("resnet", "none")):
        uclc = oracle_uclc(net, layers, scale)
        for name, v in uclc.items():
            z, flagged = ref.outliers(v.numpy(), 3.0)
            assert float((z - 3.0).abs().min()) > 1e-3, (name, scale)
            assert v.numel() >= 16
            for r in PLANTED.get(name, ()):
                assert bool(flagged[r]), (name, r, scale)


# ------------------------------------------------------------------------------------------------------------------------------ the refusals
def test_every_refusal():
    net = small()
    with pytest.raises(ValueError, match="layers must be one of"):
        clp.lipschitz_table(net, "linear")
    with pytest.raises(TypeError, match="needs a villandiffusion_amd UNet2DModel, NCSNppModel or LDMPipeline"):
        clp.lipschitz_table(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="scale must be one of"):
        clp.channel_lipschitz(net, scale="beta")
    with pytest.raises(ValueError, match="u must be finite"):
        clp.clp_prune(net, u=float("nan"), uclc={"conv_in.weight": torch.ones(32)})
    with pytest.raises(TypeError, match="uclc must be a non-empty dict"):
        clp.clp_scores([])
    with pytest.raises(ValueError, match="must be finite and non-negative"):
        clp.clp_scores({"a": torch.tensor([1.0, -1.0])})
    with pytest.raises(ValueError, match="must be a 1-d tensor"):
        clp.clp_z({"a": torch.ones(2, 2)})
    with pytest.raises(ValueError, match="are not neuron layers"):
        clp.clp_prune(net, uclc={"conv_out.weight": torch.ones(3)})
    with pytest.raises(ValueError, match="must hold 64 entries"):
        clp.clp_prune(net, uclc={"mid_block.resnets.0.conv1.weight": torch.ones(5)})
    # a selection that would empty a layer raises before anything is written
    before = net.flat_param.detach().clone()
    uc = oracle_uclc(net)
    with pytest.raises(ValueError, match="prunes every neuron of"):
        clp.clp_prune(net, u=-1e9, uclc=uc)
    assert torch.equal(net.flat_param, before)
    # a weight with another tap count is refused by name
    odd = small()
    off, n, shape = odd._offs["conv_in.weight"]
    odd._offs["conv_in.weight"] = (off, n, (shape[0], 1, 27))
    with pytest.raises(ValueError, match=r"conv_in.weight has 27 taps"):
        clp.lipschitz_table(odd, "conv")
    with pytest.raises(ValueError, match="lipschitz table: job 0"):
        clp.LipschitzTable([(0, 4, 3, 4, 0, 0)], 4, {"a": slice(0, 4)}, {"a": None}, "conv")
    with pytest.raises(ValueError, match="lipschitz table: job 1"):
        clp.LipschitzTable([(0, 4, 3, 9, 0, 0), (200, 4, 3, 9, 4, 2)], 8, {"a": slice(0, 4), "b": slice(4, 8)}, {"a": None, "b": None}, "conv")
    # the trainer's refusal for NCSN++ stands: the mask helpers of actprune name it
    with pytest.raises(NotImplementedError, match="NCSNppModel is not built"):
        PruneMask.from_model(small_pp())
    if not torch.cuda.is_available():
        with pytest.raises(lib.VillanHipError, match="gfx950|device"):
            clp.channel_lipschitz(net)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_errors(capsys):
    tool = _tool("clp_prune")
    for argv, msg in ((["--ckpt", "x", "--out", "y", "--sweep", "a,b"], "--sweep takes comma-separated"),
                      (["--ckpt", "x", "--out", "y", "--u", "nan"], "--u must be finite"),
                      (["--ckpt", "x", "--out", "y", "--n-clean", "8"], "are read with --dataset"),
                      (["--ckpt", "x", "--out", "y", "--dataset", "SYNTHETIC-CIFAR10"], "--dataset is read with --sweep")):
        with pytest.raises(SystemExit):
            tool.main(argv)
        assert msg in capsys.readouterr().err, argv


# ------------------------------------------------------------------------------------------------------------- the library's host-only checks
def test_the_library_checks_the_table_on_the_host():
    h = lib.load()
    chain = C.c_int64(0)
    for Cin in (1, 63, 64, 65, 130, 512):
        for T in (1, 9):
            assert h.vd_channel_lipschitz_plan(Cin, T, C.byref(chain)) == 0 and chain.value == ref.chain(Cin) == ops.channel_lipschitz_plan(Cin, T)
    assert h.vd_channel_lipschitz_plan(64, 4, C.byref(chain)) == EINVAL and "T = 4" in lib.last_error()
    assert h.vd_channel_lipschitz_plan(0, 9, C.byref(chain)) == EINVAL and h.vd_channel_lipschitz_plan(64, 9, None) == EINVAL
    assert h.vd_abi_version() == 12
    assert ops.LIPSCHITZ_EIGEN_BOUND == ref.EIGEN_BOUND and ops.LIPSCHITZ_SWEEPS == ref.SWEEPS and ops.LIPSCHITZ_GRAM == ref.GRAM
    # every rule of the table is checked before any launch: with fake device addresses nothing may be dereferenced
    FAKE = 0x10000

    def call(jobs, blocks, w=FAKE, out=FAKE, table=FAKE):
        host = torch.tensor(jobs, dtype=torch.int64).reshape(-1, 6)
        return h.vd_channel_lipschitz(w, host.data_ptr(), table, host.shape[0], blocks, None, out, None, None)

    good = [(0, 5, 3, 9, 0, 0), (200, 4, 7, 1, 5, 2)]
    for jobs, blocks, msg in (([(0, 5, 3, 4, 0, 0)], 2, "T = 4 taps"), ([(0, 0, 3, 9, 0, 0)], 0, "rows, Cin = 0, 0, 3"),
                              ([(0, 5, 0, 9, 0, 0)], 2, "rows, Cin = 0, 5, 0"), ([good[0], (200, 4, 7, 1, 4, 2)], 3, "first neuron 4 (expected 5)"),
                              ([good[0], (200, 4, 7, 1, 5, 1)], 3, "first workgroup 1 (expected 2)"), ([(0, 5, 3, 9, 1, 0)], 2, "first neuron 1"),
                              (good, 4, "total_blocks = 4"), ([(-4, 5, 3, 9, 0, 0)], 2, "weight offset")):
        assert call(jobs, blocks) == EINVAL and msg in lib.last_error(), (jobs, lib.last_error())
    for kw in (dict(w=None), dict(out=None), dict(table=None)):
        assert call(good, 3, **kw) == EINVAL and "null pointer" in lib.last_error()
    host = torch.tensor(good, dtype=torch.int64)
    assert h.vd_channel_lipschitz(FAKE, None, FAKE, 2, 3, None, FAKE, None, None) == EINVAL
    assert h.vd_channel_lipschitz(FAKE, host.data_ptr(), FAKE, 0, 3, None, FAKE, None, None) == EINVAL and "n_jobs = 0" in lib.last_error()
