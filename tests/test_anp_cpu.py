"""villandiffusion_amd.anp without a GPU: the neuron table, pruning, argument validation before the device is touched, no fallback, the tool's
--help, and tests/anp_ref.py against a float64 finite difference."""
import os
import subprocess
import sys

import pytest
import torch

import anp_ref
from oracle.unet_ref import UNet2DModelRef
from villandiffusion_amd import anp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # test_mitigation_gpu.py


def _model(seed=0):
    from villandiffusion_amd.unet import UNet2DModel
    net = UNet2DModel(**SMALL, device="cpu")
    net.reset_parameters(seed)
    return net


# ------------------------------------------------------------------------------------------------------------------------------ neuron_table
def test_neuron_table_covers_every_selected_row_once():
    net = _model()
    ref = UNet2DModelRef(**SMALL)
    tabs = {}
    for layers in ("conv", "all"):
        tab = tabs[layers] = anp.neuron_table(net, layers)
        jobs, n, slices = tab                                                     # unpacks as the issue states
        assert set(slices) == set(anp_ref.selected(ref, layers)) and "conv_out.weight" not in slices
        assert len(jobs) == len(slices) == tab.n_jobs
        owner = torch.zeros(net.flat_numel, dtype=torch.int32)                    # how many jobs' rows cover each float
        neuron = block = 0
        for (off, rows, ln, boff, n0, b0), (name, sl) in zip(jobs, slices.items()):
            o, numel, shape = net._offs[name]
            assert (off, rows, rows * ln) == (o, shape[0], numel) and (n0, b0) == (neuron, block) and sl == slice(neuron, neuron + rows)
            owner[off:off + rows * ln] += 1
            bias = name[:-6] + "bias"
            if bias in net._offs:
                assert boff == net._offs[bias][0] and net._offs[bias][1] == rows
            else:
                assert boff == -1
            neuron += rows
            block += (rows + 3) // 4
        assert n == neuron == sum(net._offs[name][2][0] for name in slices) and tab.total_blocks == block
        want = torch.zeros_like(owner)
        for name in slices:
            o, numel, _ = net._offs[name]
            want[o:o + numel] = 1
        assert torch.equal(owner, want)                                           # every selected float once, nothing else
        assert tab.extent <= net.flat_numel and tab.weight_floats == int(want.sum())
    assert set(tabs["conv"].slices) < set(tabs["all"].slices)
    assert (tabs["all"].n_jobs, tabs["all"].n_neurons) == (50, 2912)
    lens = [j[2] for j in tabs["all"].jobs]
    assert (min(lens), max(lens)) == (27, 1152)
    assert all(j[3] >= 0 for j in tabs["all"].jobs)                               # every layer of this network has a bias
    with pytest.raises(ValueError, match="layers"):
        anp.neuron_table(net, "linear")


def test_neuron_table_object_rejects_inconsistent_jobs():
    good = [(0, 3, 27, 84, 0, 0), (96, 5, 4, -1, 3, 1)]
    tab = anp.NeuronTable(good, 8, {"a": slice(0, 3), "b": slice(3, 8)})
    assert (tab.n_jobs, tab.total_blocks, tab.weight_floats, tab.n_bias, tab.extent) == (2, 3, 101, 3, 116)
    for bad in ([(0, 3, 27, 84, 0, 0), (96, 5, 4, -1, 3, 2)], [(0, 3, 27, 84, 0, 0), (96, 5, 4, -1, 4, 1)], [(-4, 3, 27, 84, 0, 0)],
                [(0, 0, 27, -1, 0, 0)], []):
        with pytest.raises(ValueError):
            anp.NeuronTable(bad, sum(j[1] for j in bad), {})
    with pytest.raises(ValueError):
        anp.NeuronTable(good, 9, {})


# ------------------------------------------------------------------------------------------------------------------------------ prune_neurons
def _masks(net, layers="conv", seed=3):
    tab = anp.neuron_table(net, layers)
    flat = torch.rand(tab.n_neurons, generator=torch.Generator().manual_seed(seed)) * 0.7 + 0.3
    return tab, flat, {name: flat[sl].clone() for name, sl in tab.slices.items()}


def _check_pruned(net, before, tab, drop):
    """Rows in `drop` (a bool per neuron) are exactly zero; every other float of the flat buffer has its bits."""
    want = before.clone()
    for (off, rows, ln, _, n0, _) in tab.jobs:
        for r in drop[n0:n0 + rows].nonzero().reshape(-1).tolist():
            want[off + r * ln:off + (r + 1) * ln] = 0.0
    assert torch.equal(net.flat_param.view(torch.int32), want.view(torch.int32))


def test_prune_by_threshold_and_by_fraction():
    net = _model()
    tab, flat, masks = _masks(net)
    flat[[0, 5, 40, 1215]] = torch.tensor([0.1, 0.0, 0.19, 0.05])
    masks = {name: flat[sl].clone() for name, sl in tab.slices.items()}
    before = net.flat_param.clone()
    calls = []
    net.weights_changed = lambda: calls.append(1)
    counts = anp.prune_neurons(net, masks, threshold=0.2)
    assert sum(counts.values()) == 4 and set(counts) == set(tab.slices) and calls == [1]
    _check_pruned(net, before, tab, flat < 0.2)
    first = next(iter(tab.slices))
    assert counts[first] == 2 and float(net.P[first][0].abs().max()) == 0.0 and float(net.P[first[:-6] + "bias"].abs().min()) > 0.0     # the bias stays

    # by fraction, with a NeuronMask, ties broken by neuron index: five neurons share the smallest value, k = 3 takes the first three
    net = _model()
    tab, flat, _ = _masks(net, "all", seed=4)
    tie = [2900, 7, 1500, 33, 800]
    flat[tie] = 0.25
    k = 3
    fraction = (k + 0.5) / tab.n_neurons
    res = anp.NeuronMask(masks={name: flat[sl].clone() for name, sl in tab.slices.items()}, natural=[], robust=[], layers="all", steps=1, batch=1,
                         anp_eps=0.4, anp_steps=1, anp_alpha=0.2, lr=0.2, momentum=0.9, seed=0)
    assert torch.equal(res.flat(), flat) and res.n_neurons == tab.n_neurons and res.settings()["layers"] == "all"
    before = net.flat_param.clone()
    counts = anp.prune_neurons(net, res, fraction=fraction)
    drop = torch.zeros(tab.n_neurons, dtype=torch.bool)
    drop[sorted(tie)[:k]] = True
    assert sum(counts.values()) == k
    _check_pruned(net, before, tab, drop)
    # fraction 0 prunes nothing; a dict in another order gives the same selection
    net2 = _model()
    assert sum(anp.prune_neurons(net2, res, fraction=0.0).values()) == 0 and torch.equal(net2.flat_param, before)
    anp.prune_neurons(net2, dict(reversed(list(res.masks.items()))), fraction=fraction)
    assert torch.equal(net2.flat_param, net.flat_param)


def test_prune_refuses_an_emptied_layer_and_bad_arguments():
    net = _model()
    tab, flat, masks = _masks(net)
    victim = list(tab.slices)[3]
    masks[victim] = torch.zeros_like(masks[victim])
    before = net.flat_param.clone()
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        anp.prune_neurons(net, masks, threshold=0.2)
    assert torch.equal(net.flat_param, before)                                   # nothing was written
    rows = masks[victim].numel()
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        anp.prune_neurons(net, masks, fraction=(rows + 0.5) / tab.n_neurons)     # the smallest `rows` masks are exactly that layer
    assert torch.equal(net.flat_param, before)
    _, _, masks = _masks(net)
    for kw in (dict(), dict(threshold=0.2, fraction=0.1)):
        with pytest.raises(ValueError, match="exactly one"):
            anp.prune_neurons(net, masks, **kw)
    for kw in (dict(fraction=1.0), dict(fraction=-0.1), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            anp.prune_neurons(net, masks, **kw)
    with pytest.raises(ValueError, match="conv_out"):
        anp.prune_neurons(net, masks | {"conv_out.weight": torch.ones(3)}, threshold=0.2)
    with pytest.raises(ValueError, match="entries"):
        anp.prune_neurons(net, masks | {victim: torch.ones(3)}, threshold=0.2)
    with pytest.raises(TypeError):
        anp.prune_neurons(net, torch.ones(4), threshold=0.2)
    assert torch.equal(net.flat_param, before)


# ------------------------------------------------------------------------------------------------------------------------------ validation
def test_anp_validates_before_touching_the_device(monkeypatch):
    from villandiffusion_amd import lib
    from villandiffusion_amd import schedulers as S
    assert set(anp.__all__) == {"NeuronTable", "neuron_table", "anp_objective", "NeuronMask", "learn_neuron_mask", "prune_neurons"}
    monkeypatch.setattr(lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device touched before validation")))
    net, sched = _model(), S.DDPMScheduler()
    clean = torch.zeros(8, 3, 32, 32)
    n = anp.neuron_table(net, "conv").n_neurons
    ok = dict(steps=2, batch=4)
    for bad in (dict(steps=0, batch=4), dict(steps=2.5, batch=4), dict(steps=2, batch=0), dict(steps=2, batch="4"), ok | dict(lr=0.0),
                ok | dict(lr=float("inf")), ok | dict(anp_eps=-0.1), ok | dict(anp_eps=float("nan")), ok | dict(anp_steps=0),
                ok | dict(anp_steps=1.5), ok | dict(anp_alpha=1.5), ok | dict(anp_alpha=-0.1), ok | dict(momentum=1.0), ok | dict(momentum=-0.5),
                ok | dict(layers="linear"), ok | dict(noise=torch.zeros(2, 4, 3, 16, 16)), ok | dict(noise=torch.zeros(3, 4, 3, 32, 32)),
                ok | dict(timesteps=torch.zeros(2, 3, dtype=torch.int64)), ok | dict(timesteps=torch.zeros(2, 4)),
                ok | dict(timesteps=torch.full((2, 4), 1000)), ok | dict(timesteps=torch.full((2, 4), -1)),
                ok | dict(perturbation=torch.zeros(2, 2, n + 1)), ok | dict(perturbation=torch.full((2, 2, n), 0.5))):
        with pytest.raises(ValueError):
            anp.learn_neuron_mask(net, sched, clean, **bad)
    for bad in (torch.zeros(8, 3, 16, 16), torch.zeros(3, 32, 32), torch.zeros(0, 3, 32, 32), [clean], torch.zeros(8, 3, 32, 32, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="clean"):
            anp.learn_neuron_mask(net, sched, bad, **ok)
    for bad in (dict(noise=3), dict(timesteps=3), dict(perturbation=3)):
        with pytest.raises(TypeError):
            anp.learn_neuron_mask(net, sched, clean, **ok, **bad)
    with pytest.raises(NotImplementedError, match="ScoreSdeVeScheduler"):
        anp.learn_neuron_mask(net, S.ScoreSdeVeScheduler(), clean, **ok)
    from villandiffusion_amd.ncsnpp import NCSNppModel
    pp = NCSNppModel(sample_size=16, block_out_channels=(32, 64, 64), layers_per_block=1, device="cpu",
                     down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                     up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"))
    with pytest.raises(NotImplementedError, match="NCSNppModel"):
        anp.learn_neuron_mask(pp, sched, torch.zeros(8, 3, 16, 16), **ok)
    net.conv_math = "f16"
    with pytest.raises(NotImplementedError, match="f16"):
        anp.learn_neuron_mask(net, sched, clean, **ok)
    with pytest.raises(NotImplementedError, match="f16"):
        anp.anp_objective(net, sched, clean[:2], torch.zeros(2, dtype=torch.int64), clean[:2], torch.ones(n))
    net.conv_math = "bf16x3"
    t2, m = torch.zeros(2, dtype=torch.int64), torch.ones(n)
    for args in ((clean[:2], t2, clean[:3], m), (clean[:2], torch.zeros(3, dtype=torch.int64), clean[:2], m), (clean[:2], t2, clean[:2], torch.ones(n + 1)),
                 (clean[:2], t2, clean[:2], torch.ones(1, n))):
        with pytest.raises(ValueError):
            anp.anp_objective(net, sched, *args)
    with pytest.raises(ValueError, match="delta"):
        anp.anp_objective(net, sched, clean[:2], t2, clean[:2], m, delta=torch.zeros(n - 1))


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box WITHOUT a GPU")
def test_no_fallback_without_a_gpu():
    from villandiffusion_amd import lib, ops
    from villandiffusion_amd import schedulers as S
    net = _model()
    start = net.flat_param.clone()
    with pytest.raises(lib.VillanHipError):
        anp.learn_neuron_mask(net, S.DDPMScheduler(), torch.zeros(8, 3, 32, 32), steps=1, batch=4)
    n = anp.neuron_table(net, "all").n_neurons
    with pytest.raises(lib.VillanHipError):
        anp.anp_objective(net, S.DDPMScheduler(), torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, 32, 32), torch.ones(n))
    with pytest.raises(lib.VillanHipError):
        ops.neuron_step(torch.zeros(4), torch.zeros(4), lr=0.1, lo=0.0, hi=1.0)
    assert torch.equal(net.flat_param, start)


def test_tool_help_and_header():
    for tool, flags in (("anp_defense.py", ("--ckpt", "--dataset", "--n-clean", "--steps", "--batch", "--anp-eps", "--anp-steps", "--anp-alpha", "--lr",
                                            "--layers", "--threshold", "--fraction", "--seed", "--out")),
                        ("anp_step_ab.py", ("--rounds", "--steps", "--out"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        for flag in flags:
            assert flag in out.stdout, (tool, flag)
    from villandiffusion_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "villan_hip.h")).read()
    for name, n_args in (("vd_neuron_scale", 9), ("vd_neuron_grad", 10), ("vd_neuron_step", 10)):
        assert f"int {name}(" in hdr and len(lib.PROTOTYPES[name][1]) == n_args and callable(getattr(ops, name[3:]))


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_mask_gradient_equals_a_float64_central_difference():
    torch.manual_seed(0)
    ref = UNet2DModelRef(**SMALL).double()
    tab = anp.neuron_table(_model(), "all")
    n, slices = tab.n_neurons, tab.slices
    gen = torch.Generator().manual_seed(5)
    clean = torch.rand(2, 3, 32, 32, generator=gen, dtype=torch.float64) * 2 - 1
    eps = torch.randn(2, 3, 32, 32, generator=gen, dtype=torch.float64)
    t = torch.tensor([300, 950])
    mask = torch.rand(n, generator=gen, dtype=torch.float64) * 0.5 + 0.5
    delta = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * 0.4
    xi = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * 0.4
    loss, gmask, gxi = anp_ref.objective(ref, slices, n, clean, t, eps, mask, delta, xi)
    assert loss.dtype == torch.float64 and float(loss) > 0
    # The oracle's attention softmax runs in float32 whatever the model's dtype (as upstream's does), which leaves ~1e-10 of rounding noise on the
    # float64 loss: ~1e-8 on the difference quotient at h = 1e-2, beside a truncation error of h^2 / 6 = 1.7e-5 times the third derivative.  The
    # check takes, in each of three layers (27-float rows, an attention projection, the longest rows), the neuron with the largest gradient -- 1e-4
    # and more, so the noise is below 1e-4 of it -- and holds the quotient to 1e-3 of it: the gate the GPU tests then hold the kernels to
    # against this reference.
    h = 1e-2
    for layer in ("conv_in.weight", "mid_block.attentions.0.to_v.weight", "up_blocks.0.resnets.0.conv1.weight"):
        sl = slices[layer]
        for vec, grad, what in ((mask, gmask, "mask"), (xi, gxi, "xi")):
            j = sl.start + int(grad[sl].abs().argmax())
            up, dn = vec.clone(), vec.clone()
            up[j] += h
            dn[j] -= h
            args = (lambda v: (v, delta, xi)) if vec is mask else (lambda v: (mask, delta, v))
            fd = (float(anp_ref.objective(ref, slices, n, clean, t, eps, *args(up))[0]) -
                  float(anp_ref.objective(ref, slices, n, clean, t, eps, *args(dn))[0])) / (2 * h)
            err = abs(fd - float(grad[j])) / abs(float(grad[j]))
            print(f"[parity] anp_ref {layer} neuron {j} ({what}): autograd {float(grad[j]):.6e}, central difference {fd:.6e}, rel {err:.1e}")
            assert abs(float(grad[j])) >= 1e-4 and err <= 1e-3
    # the step's restatement: sign(+-0) = 0, the momentum buffer, both clamps
    x, _ = anp_ref.step(torch.tensor([0.5, 0.5, 0.5, 0.39]), torch.tensor([0.0, -0.0, -2.0, 3.0]), None, -0.4, 0.0, -0.4, 0.4, True)
    lim = float(torch.tensor(0.4, dtype=torch.float32))
    assert x[[0, 1, 3]].tolist() == [lim] * 3 and abs(float(x[2]) - 0.1) < 1e-6
    x, b = anp_ref.step(torch.tensor([1.0, 0.0]), torch.tensor([-1.0, 1.0]), torch.tensor([2.0, 2.0]), 0.5, 0.5, 0.0, 1.0, False)
    assert x.tolist() == [1.0, 0.0] and b.tolist() == [0.0, 2.0]
