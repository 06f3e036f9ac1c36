"""villandiffusion_amd.anp_ve and villandiffusion_amd.anp_ldm without a GPU: the neuron tables, what each module refuses and where it sends it,
tests/anp_families_ref.py against a float64 finite difference and against itself in f32 (the reference alone must sit well inside the gates the
GPU tests hold the kernels to), no fallback, and the two tools' --help."""
import os
import subprocess
import sys

import pytest
import torch

import anp_families_ref as fam
from oracle.ncsnpp_ref import NCSNppRef
from oracle.unet_ref import UNet2DModelRef
from villandiffusion_amd import anp, anp_ldm, anp_ve
from villandiffusion_amd import pipelines as P
from villandiffusion_amd import schedulers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP_SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
                down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_anp_cpu.py's
VQ_NET = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3,
              down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2, sample_size=16)   # test_defense_ldm_gpu.py's


def _pp(layers_per_block=1):
    from villandiffusion_amd.ncsnpp import NCSNppModel
    net = NCSNppModel(**fam.SMALL_PP, layers_per_block=layers_per_block, device="cpu")
    net.reset_parameters(0)
    return net


def _unet(cfg, seed=0):
    from villandiffusion_amd.unet import UNet2DModel
    net = UNet2DModel(**cfg, device="cpu")
    net.reset_parameters(seed)
    return net


def _ldm():
    from villandiffusion_amd.vqmodel import VQModel
    return P.LDMPipeline(vqvae=VQModel(**VQ_NET, device="cpu"), unet=_unet(fam.SMALL_LDM), scheduler=S.DDIMScheduler())


def _ve_sched():
    return S.ScoreSdeVeScheduler(**fam.VE_SCHED)


# ------------------------------------------------------------------------------------------------------------------------------ 1. tables
def _check_cover(net, tab, names):
    """Every float of the weights in `names` is covered by exactly one job, nothing else is; biases are found where the model has them."""
    assert list(tab.slices) == [n for n, _, _ in net._layout if n in set(names)] and len(tab.jobs) == len(names)
    owner = torch.zeros(net.flat_numel, dtype=torch.int32)
    neuron = block = 0
    for (off, rows, ln, boff, n0, b0), (name, sl) in zip(tab.jobs, tab.slices.items()):
        o, numel, shape = net._offs[name]
        assert (off, rows, rows * ln) == (o, shape[0], numel) and (n0, b0) == (neuron, block) and sl == slice(neuron, neuron + rows)
        owner[off:off + rows * ln] += 1
        bias = name[:-6] + "bias"
        assert boff == (net._offs[bias][0] if bias in net._offs else -1)
        neuron += rows
        block += (rows + 3) // 4
    want = torch.zeros_like(owner)
    for name in names:
        o, numel, _ = net._offs[name]
        want[o:o + numel] = 1
    assert torch.equal(owner, want) and tab.n_neurons == neuron and tab.extent <= net.flat_numel


@pytest.mark.parametrize("layers_per_block,jobs,neurons", [(1, 73, 4256), (2, 98, 5632)])
def test_ncsnpp_neuron_table(layers_per_block, jobs, neurons):
    net = _pp(layers_per_block)
    ref = NCSNppRef(**fam.SMALL_PP, layers_per_block=layers_per_block)
    tabs = {layers: anp_ve.neuron_table(net, layers) for layers in ("conv", "all")}
    assert (tabs["all"].n_jobs, tabs["all"].n_neurons) == (jobs, neurons)
    for layers, tab in tabs.items():
        names = fam.selected(ref, layers)
        assert set(tab.slices) == set(names)
        _check_cover(net, tab, names)
        for head in fam.HEADS + ("time_proj.weight",):                                 # the image-channel heads and the Fourier features
            assert head in net._offs and head not in tab.slices
            o, numel, _ = net._offs[head]
            assert not any(off < o + numel and o < off + rows * ln for off, rows, ln, _, _, _ in tab.jobs)
            assert not any(o <= boff < o + numel for _, _, _, boff, _, _ in tab.jobs)
        for k in (0, 1):                                                               # rows of feature channels: an ordinary layer, 3-float rows
            name = f"down_blocks.{k}.skip_conv.weight"
            job = tab.jobs[list(tab.slices).index(name)]
            assert job[2] == 3 and job[3] == net._offs[name[:-6] + "bias"][0] and job[1] == net._offs[name][2][0]
    assert set(tabs["conv"].slices) < set(tabs["all"].slices)
    assert min(j[2] for j in tabs["all"].jobs) == 3


def test_ldm_and_vp_tables():
    pipe = _ldm()
    tab = anp_ldm.neuron_table(pipe, "all")
    assert (tab.n_jobs, tab.n_neurons) == (50, 2912) and tab.jobs == anp.neuron_table(pipe.unet, "all").jobs
    _check_cover(pipe.unet, tab, [n for n, sh, _ in pipe.unet._layout if len(sh) >= 2 and n != "conv_out.weight"])
    # the VP tables of anp.neuron_table are what they were: the rule of tests/anp_ref.py, conv_out.weight alone left out
    import anp_ref
    net, ref = _unet(VP_SMALL), UNet2DModelRef(**VP_SMALL)
    for layers, count in (("conv", None), ("all", (50, 2912))):
        tab = anp.neuron_table(net, layers)
        names = anp_ref.selected(ref, layers)
        assert set(tab.slices) == set(names)
        _check_cover(net, tab, names)
        if count:
            lens = [j[2] for j in tab.jobs]
            assert (tab.n_jobs, tab.n_neurons) == count and (min(lens), max(lens)) == (27, 1152)


def test_prune_neurons_on_ncsnpp_and_ldm():
    net = _pp()
    tab = anp_ve.neuron_table(net, "all")
    flat = torch.rand(tab.n_neurons, generator=torch.Generator().manual_seed(3)) * 0.7 + 0.3
    skip = tab.slices["down_blocks.0.skip_conv.weight"]
    flat[[skip.start + 1, 7]] = 0.1
    masks = {name: flat[sl].clone() for name, sl in tab.slices.items()}
    before = net.flat_param.clone()
    for head in fam.HEADS:                                                             # a mask naming an excluded weight
        with pytest.raises(ValueError, match=head.replace(".", r"\.")):
            anp_ve.prune_neurons(net, masks | {head: torch.ones(3)}, threshold=0.2)
    assert torch.equal(net.flat_param, before)
    counts = anp_ve.prune_neurons(net, masks, threshold=0.2)
    assert sum(counts.values()) == 2 and counts["down_blocks.0.skip_conv.weight"] == 1
    want = before.clone()
    for (off, rows, ln, _, n0, _) in tab.jobs:
        for r in (flat[n0:n0 + rows] < 0.2).nonzero().reshape(-1).tolist():
            want[off + r * ln:off + (r + 1) * ln] = 0.0
    assert torch.equal(net.flat_param.view(torch.int32), want.view(torch.int32))       # the rows are zero, every other float has its bits
    with pytest.raises(TypeError, match="NCSNppModel"):
        anp_ve.prune_neurons(_unet(VP_SMALL), masks, threshold=0.2)
    pipe = _ldm()
    ltab = anp_ldm.neuron_table(pipe, "conv")
    lflat = torch.rand(ltab.n_neurons, generator=torch.Generator().manual_seed(4)) * 0.7 + 0.3
    vq_before, twin = pipe.vqvae.flat_param.clone(), _unet(fam.SMALL_LDM)
    lmasks = {name: lflat[sl].clone() for name, sl in ltab.slices.items()}
    assert anp_ldm.prune_neurons(pipe, lmasks, fraction=0.05) == anp.prune_neurons(twin, lmasks, fraction=0.05)
    assert torch.equal(pipe.unet.flat_param, twin.flat_param) and torch.equal(pipe.vqvae.flat_param, vq_before)


# ------------------------------------------------------------------------------------------------------------------------------ 2. refusals
def test_each_module_refuses_the_other_families(monkeypatch):
    from villandiffusion_amd import lib
    monkeypatch.setattr(lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device touched before validation")))
    assert set(anp_ve.__all__) >= {"neuron_table", "anp_objective", "learn_neuron_mask", "prune_neurons", "NeuronMask", "pruning_curve"}
    assert set(anp_ldm.__all__) >= {"neuron_table", "anp_objective", "learn_neuron_mask", "prune_neurons", "NeuronMask", "pruning_curve"}
    assert anp_ve.NeuronMask is anp.NeuronMask is anp_ldm.NeuronMask and callable(anp.pruning_curve)
    pp, unet, ldm = _pp(), _unet(VP_SMALL), _ldm()
    ok = dict(steps=2, batch=4)
    img32, img16, lat = torch.zeros(8, 3, 32, 32), torch.zeros(8, 3, 16, 16), torch.zeros(8, 3, 8, 8)
    t4, masks = torch.zeros(8, dtype=torch.int64), {"conv_in.weight": torch.ones(32)}
    # anp: the pairs tests/test_anp_cpu.py pins, now saying where to go
    with pytest.raises(NotImplementedError, match=r"NCSNppModel.*anp_ve"):
        anp.learn_neuron_mask(pp, S.DDPMScheduler(), img16, **ok)
    with pytest.raises(NotImplementedError, match=r"ScoreSdeVeScheduler.*anp_ve"):
        anp.learn_neuron_mask(unet, _ve_sched(), img32, **ok)
    with pytest.raises(NotImplementedError, match="anp_ve"):
        anp.pruning_curve(pp, S.DDPMScheduler(), img16, masks, fractions=(0.1,))
    # anp_ve: a VP network, a VP scheduler, a pipeline
    for call in (lambda m, s, x: anp_ve.learn_neuron_mask(m, s, x, **ok),
                 lambda m, s, x: anp_ve.anp_objective(m, s, x, t4, x, torch.ones(5)),
                 lambda m, s, x: anp_ve.pruning_curve(m, s, x, masks, fractions=(0.1,))):
        with pytest.raises(NotImplementedError, match=r"UNet2DModel.*villandiffusion_amd\.anp "):
            call(unet, _ve_sched(), img32)
        with pytest.raises(NotImplementedError, match=r"DDPMScheduler.*villandiffusion_amd\.anp "):
            call(pp, S.DDPMScheduler(), img16)
        with pytest.raises(NotImplementedError, match="anp_ldm"):
            call(ldm, _ve_sched(), img16)
        with pytest.raises(TypeError):
            call(torch.nn.Linear(2, 2), _ve_sched(), img16)
        for mode in ("f16", "bf16"):                                                   # the arithmetic defense_ve refuses
            pp.conv_math = mode
            with pytest.raises(NotImplementedError, match=mode):
                call(pp, _ve_sched(), img16)
        pp.conv_math = "bf16x3"
    # anp_ldm: a pixel-space pipeline, a score-SDE pipeline, the bare networks
    for call in (lambda p, x: anp_ldm.learn_neuron_mask(p, x, **ok), lambda p, x: anp_ldm.anp_objective(p, x, t4, x, torch.ones(5)),
                 lambda p, x: anp_ldm.pruning_curve(p, x, masks, fractions=(0.1,)), lambda p, x: anp_ldm.prune_neurons(p, masks, threshold=0.2),
                 lambda p, x: anp_ldm.neuron_table(p)):
        for bad in (P.DDIMPipeline(unet, S.DDIMScheduler()), unet):
            with pytest.raises(NotImplementedError, match=r"villandiffusion_amd\.anp "):
                call(bad, img32)
        for bad in (P.ScoreSdeVePipeline(pp, _ve_sched()), pp):
            with pytest.raises(NotImplementedError, match="anp_ve"):
                call(bad, img16)
        with pytest.raises(TypeError):
            call(torch.nn.Linear(2, 2), lat)
    ldm.unet.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16"):
        anp_ldm.learn_neuron_mask(ldm, lat, **ok)
    ldm.unet.conv_math = "bf16x3"
    # anp_ldm: clean is latent-shaped or pixel-shaped, told apart by its shape; anything else names both
    assert anp_ldm.clean_space(ldm, lat) == "latent" and anp_ldm.clean_space(ldm, img16) == "pixel"
    n = anp_ldm.neuron_table(ldm, "conv").n_neurons
    for bad in (img32, torch.zeros(8, 3, 8, 16), torch.zeros(3, 8, 8), torch.zeros(0, 3, 8, 8), [lat], torch.zeros(8, 3, 8, 8, dtype=torch.uint8)):
        for call in (lambda x: anp_ldm.learn_neuron_mask(ldm, x, **ok), lambda x: anp_ldm.pruning_curve(ldm, x, masks, fractions=(0.1,)),
                     lambda x: anp_ldm.anp_objective(ldm, x, t4, lat, torch.ones(n))):
            with pytest.raises(ValueError, match=r"3, 8, 8\].*3, 16, 16\]"):
                call(bad)
    # the shared checks reach the new modules, before the device, for a pixel-shaped clean set too
    for bad in (dict(steps=0, batch=4), ok | dict(anp_steps=0), ok | dict(momentum=1.0), ok | dict(layers="linear"),
                ok | dict(noise=torch.zeros(2, 4, 3, 16, 16)), ok | dict(timesteps=torch.full((2, 4), 1000))):
        for x in (lat, img16):
            with pytest.raises(ValueError):
                anp_ldm.learn_neuron_mask(ldm, x, **bad)
    for bad in (dict(steps=0, batch=4), ok | dict(anp_alpha=1.5), ok | dict(timesteps=torch.full((2, 4), 2000)), ok | dict(noise=torch.zeros(2, 4, 3, 8, 8))):
        with pytest.raises(ValueError):
            anp_ve.learn_neuron_mask(pp, _ve_sched(), img16, **bad)
    with pytest.raises(ValueError, match="clean"):
        anp_ve.learn_neuron_mask(pp, _ve_sched(), img32, **ok)
    nv = anp_ve.neuron_table(pp, "all").n_neurons
    with pytest.raises(ValueError, match="sigma table"):
        anp_ve.anp_objective(pp, _ve_sched(), img16, torch.full((8,), 2000), img16, torch.ones(nv))
    with pytest.raises(ValueError, match="delta"):
        anp_ve.anp_objective(pp, _ve_sched(), img16, t4, img16, torch.ones(nv), delta=torch.zeros(nv - 1))
    # pruning_curve: the candidates are checked before anything runs -- one that empties a layer names it
    tab = anp_ve.neuron_table(pp, "conv")
    flat = torch.rand(tab.n_neurons, generator=torch.Generator().manual_seed(5)) * 0.5 + 0.5
    victim = "down_blocks.1.skip_conv.weight"
    flat[tab.slices[victim]] = 0.0
    res = {name: flat[sl].clone() for name, sl in tab.slices.items()}
    rows = tab.slices[victim].stop - tab.slices[victim].start
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        anp_ve.pruning_curve(pp, _ve_sched(), img16, res, fractions=(0.001, (rows + 0.5) / tab.n_neurons))
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        anp_ve.pruning_curve(pp, _ve_sched(), img16, res, thresholds=(0.2,))
    for kw in (dict(), dict(thresholds=(0.2,), fractions=(0.1,))):
        with pytest.raises(ValueError, match="exactly one"):
            anp_ve.pruning_curve(pp, _ve_sched(), img16, res, **kw)
    with pytest.raises(ValueError):
        anp_ve.pruning_curve(pp, _ve_sched(), img16, res, fractions=(0.001,), timesteps=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        anp_ve.pruning_curve(pp, _ve_sched(), img16, res, fractions=(0.001,), noise=torch.zeros(8, 3, 8, 8))


def test_training_sigma_table_not_the_inference_one():
    """The VE family's loss tables are rebuilt from the scheduler's configuration: a set_sigmas(5) left behind by a pipeline is not read."""
    sched = _ve_sched()
    want = sched.sigmas.flip([0]).float().clone()
    sched.set_timesteps(5)
    sched.set_sigmas(5)                                                                # what a 5-step pipeline call leaves behind
    assert sched.sigmas.numel() == 5
    f = anp_ve._family(_pp(), sched)
    assert f.T_train == 2000 and torch.equal(f.loss._sigmas_asc, want)
    assert 0.01 <= float(want[0]) < 0.0101 and abs(float(want[-1]) - 380.0) < 1e-3 and bool((want[1:] > want[:-1]).all())
    assert len(f.skip) == 1 and f.skip[0].shape == (32,)                               # time_proj.weight: never unfrozen


# ------------------------------------------------------------------------------------------------------------------------------ 3. the VE oracle
def test_ve_reference_gradients_equal_a_float64_central_difference():
    ref = fam.small_ncsnpp(1).double()
    tab = anp_ve.neuron_table(_pp(1), "all")
    n, slices = tab.n_neurons, tab.slices
    d = fam.ve_inputs(n, seed=5)
    clean, eps, t = d["clean"][:2].double(), d["noise"][0, :2].double(), torch.tensor([700, 1999])
    mask, delta, xi = d["mask"].double(), d["pert"][0, 0].double(), d["pert"][0, 1].double()
    loss, gmask, gxi = fam.objective("ve", ref, slices, n, clean, t, eps, mask, delta, xi)
    assert loss.dtype == torch.float64 and float(loss) > 0
    longest = max(slices, key=lambda name: tab.jobs[list(slices).index(name)][2])
    skip = "down_blocks.0.skip_conv.weight"
    assert tab.jobs[list(slices).index(skip)][2] == 3 and tab.jobs[list(slices).index(longest)][2] == 1152
    # As tests/test_anp_cpu.py does for the VP oracle: in each of three layers -- 27-float rows, the 3-float rows of the input-image pyramid, the
    # longest rows -- the neuron with the largest gradient, held to 1e-3 of it at h = 1e-2 (truncation h^2 / 6 times the third derivative; the
    # oracle's attention softmax is float32 whatever the dtype, ~1e-8 on the quotient).
    h = 1e-2
    for layer in ("conv_in.weight", skip, longest):
        sl = slices[layer]
        for vec, grad, what in ((mask, gmask, "mask"), (xi, gxi, "xi")):
            j = sl.start + int(grad[sl].abs().argmax())
            up, dn = vec.clone(), vec.clone()
            up[j] += h
            dn[j] -= h
            args = (lambda v: (v, delta, xi)) if vec is mask else (lambda v: (mask, delta, v))
            fd = (float(fam.objective("ve", ref, slices, n, clean, t, eps, *args(up))[0]) -
                  float(fam.objective("ve", ref, slices, n, clean, t, eps, *args(dn))[0])) / (2 * h)
            err = abs(fd - float(grad[j])) / abs(float(grad[j]))
            print(f"[parity] anp_families_ref VE {layer} neuron {j} ({what}): autograd {float(grad[j]):.6e}, central difference {fd:.6e}, rel {err:.1e}")
            assert abs(float(grad[j])) >= 1e-4 and err <= 1e-3


# ------------------------------------------------------------------------------------------------------------------------------ 4. f32 vs float64
def _reference_alone(family, ref, tab, d, label):
    """The f32 oracle against the float64 one on the GPU tests' inputs: a tenth of the gates (loss 1e-5, gradients 1e-3 per layer), and at most
    10 % of the neurons with a float64 gradient within 1e-2 of zero on their layer's scale (the share the sign test may exclude)."""
    n, slices = tab.n_neurons, tab.slices
    ref64 = __import__("copy").deepcopy(ref).double()
    for case in ("ones", "random"):
        args = fam.case_args(d, n, case)
        l32, m32, x32 = fam.objective(family, ref, slices, n, d["clean"][:4], d["timesteps"][0], d["noise"][0], *args)
        l64, m64, x64 = fam.objective(family, ref64, slices, n, d["clean"][:4], d["timesteps"][0], d["noise"][0], *args)
        assert l32.dtype == torch.float32 and l64.dtype == torch.float64
        e_l = abs(float(l32) - float(l64)) / abs(float(l64))
        e_m, e_x = fam.layer_errors(m32, m64, slices), fam.layer_errors(x32, x64, slices)
        share, firm = fam.near_zero_share(m64, slices)
        flips = int((torch.sign(m32.double()[firm]) != torch.sign(m64[firm])).sum())
        print(f"[parity] {label} ({case}): f32 vs float64 oracle loss {e_l:.1e}, gmask {e_m[0]:.1e} at {e_m[1]}, gxi {e_x[0]:.1e} at {e_x[1]}; "
              f"near-zero share {share:.1%}, sign flips on the rest {flips}")
        assert e_l <= 1e-6 and e_m[0] <= 1e-4 and e_x[0] <= 1e-4
        assert share <= 0.10


def test_ve_reference_alone_stays_inside_the_gates():
    tab = anp_ve.neuron_table(_pp(1), "all")
    _reference_alone("ve", fam.small_ncsnpp(1), tab, fam.ve_inputs(tab.n_neurons), "NCSN++ layers_per_block=1, t = [0, 700, 1400, 1999] of 2000")


def test_ldm_reference_alone_stays_inside_the_gates():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**fam.SMALL_LDM)
    fam.perturb_norms(ref)
    tab = anp.neuron_table(_unet(fam.SMALL_LDM), "all")
    _reference_alone("ldm", ref, tab, fam.ldm_inputs(tab.n_neurons), "LDM small UNet 3x8x8, t = [10, 300, 600, 950]")


# ------------------------------------------------------------------------------------------------------------------------------ 5. no fallback
@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_gpu():
    from villandiffusion_amd import lib
    pp, ldm = _pp(), _ldm()
    starts = [pp.flat_param.clone(), ldm.unet.flat_param.clone(), ldm.vqvae.flat_param.clone()]
    img, lat, t = torch.zeros(4, 3, 16, 16), torch.zeros(4, 3, 8, 8), torch.zeros(4, dtype=torch.int64)
    nv, nl = anp_ve.neuron_table(pp, "all").n_neurons, anp_ldm.neuron_table(ldm, "all").n_neurons
    mv = {name: torch.rand(sl.stop - sl.start) for name, sl in anp_ve.neuron_table(pp, "conv").slices.items()}
    ml = {name: torch.rand(sl.stop - sl.start) for name, sl in anp_ldm.neuron_table(ldm, "conv").slices.items()}
    for call in (lambda: anp_ve.learn_neuron_mask(pp, _ve_sched(), img, steps=1, batch=4),
                 lambda: anp_ve.anp_objective(pp, _ve_sched(), img, t, img, torch.ones(nv)),
                 lambda: anp_ve.pruning_curve(pp, _ve_sched(), img, mv, fractions=(0.02,)),
                 lambda: anp_ldm.learn_neuron_mask(ldm, lat, steps=1, batch=4), lambda: anp_ldm.learn_neuron_mask(ldm, img, steps=1, batch=4),
                 lambda: anp_ldm.anp_objective(ldm, lat, t, lat, torch.ones(nl)), lambda: anp_ldm.anp_objective(ldm, img, t, lat, torch.ones(nl)),
                 lambda: anp_ldm.pruning_curve(ldm, lat, ml, fractions=(0.02,)), lambda: anp_ldm.pruning_curve(ldm, img, ml, fractions=(0.02,)),
                 lambda: anp.pruning_curve(_unet(VP_SMALL), S.DDPMScheduler(), torch.zeros(4, 3, 32, 32),
                                           {"conv_in.weight": torch.rand(32)}, fractions=(0.1,))):
        with pytest.raises(lib.VillanHipError):
            call()
    for net, start in zip((pp, ldm.unet, ldm.vqvae), starts):
        assert torch.equal(net.flat_param, start)
    assert not pp.time_proj.weight.requires_grad and all(p.requires_grad for n, p in pp.named_parameters() if n != "time_proj.weight")


# ------------------------------------------------------------------------------------------------------------------------------ 6. the tools
def test_tools_help():
    for tool, flags in (("anp_defense.py", ("--sweep", "--fraction", "--threshold", "--layers")), ("anp_step_ab.py", ("--family", "--rounds"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        for flag in flags:
            assert flag in out.stdout, (tool, flag)
        assert "are refused" not in out.stdout                                          # the header no longer turns the two families away
