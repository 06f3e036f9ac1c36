"""Interleaved timing on one box for one mask-learning step of Adversarial Neuron Pruning (villandiffusion_amd.anp) on config #2's network
(CIFAR10 32x32 UNet, 35.7 M parameters) at batch 64, layers="all", anp_steps = 1: three forward + backward passes, each after a write of the
neuron-scaled weights, three mask-gradient reductions and the projected steps:
 * "kernels": `anp._Passes.step` as `learn_neuron_mask` runs it -- vd_neuron_scale, vd_neuron_grad and vd_neuron_step, one launch each for the
   whole network;
 * "torch": the same step with the scale and the row dots written as per-layer torch ops on the parameter views (one multiply per weight and
   per bias, one multiply + row sum per weight gradient; the projected steps stay on vd_neuron_step) -- ms per step, alternating inside every
   round; the spread of each over the rounds is the same-box run-to-run spread the difference is to be read against;
 * the two kernels alone over the full flat buffer, bytes over time against the 8 TB/s HBM peak: vd_neuron_scale (8 B/selected float) and
   vd_neuron_grad (8 B/selected float).
   python tools/anp_step_ab.py [--rounds 3] [--steps 20] [--out profiles/r11_anp_ab.json]
--family ve / ldm measures the other two families' step instead (villandiffusion_amd.anp_ve on the default NCSN++, 32x32 at batch 64;
villandiffusion_amd.anp_ldm's loss on config #5's latent UNet, 3x64x64 latents at batch 8): the mask-learning step ("kernels") alternating with
its three forward + backward passes alone, without the neuron kernels ("passes"), and the two kernels over the whole flat buffer; the record
goes under the family's name into profiles/r12_anp_families.json, beside whatever that file already holds.  Information only: no gate.
Run it under a time limit of its own (`timeout -k 10 300 python tools/anp_step_ab.py`)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="default 64 (vp, ve), 8 (ldm)")
    ap.add_argument("--family", choices=("vp", "ve", "ldm"), default="vp",
                    help="vp: config #2's UNet against the per-layer torch leg (the default, as ever); ve / ldm: the family's step against its bare passes")
    ap.add_argument("--out", default=None, help="default profiles/r11_anp_ab.json (vp), profiles/r12_anp_families.json (ve, ldm)")
    args = ap.parse_args()
    assert args.rounds >= 3
    if args.batch is None:
        args.batch = 8 if args.family == "ldm" else 64
    if args.out is None:
        args.out = os.path.join("profiles", "r11_anp_ab.json" if args.family == "vp" else "r12_anp_families.json")

    import torch
    from villandiffusion_amd import anp, ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.defense import _trainable
    from villandiffusion_amd.unet import UNet2DModel

    class TorchPasses(anp._Passes):
        """Leg B: the write of the scaled weights and the row dots as per-layer torch ops."""

        def write(self, mask, delta, xi):
            net = self.model
            s = mask if delta is None else mask + delta
            for name, sl in self.tab.slices.items():
                off, n, shape = net._offs[name]
                torch.mul(self.w0[off:off + n].view(shape[0], -1), s[sl].unsqueeze(1), out=net.P[name].view(shape[0], -1))
                bias = name[:-6] + "bias"
                if bias in net._offs:
                    bo, bn, _ = net._offs[bias]
                    if xi is None:
                        net.P[bias].copy_(self.w0[bo:bo + bn])
                    else:
                        torch.mul(self.w0[bo:bo + bn], 1.0 + xi[sl], out=net.P[bias])
            ops.WEIGHTS_EPOCH += 1
            net.weights_changed()

        def grad(self, gmask, gxi, scale=1.0, accumulate=False):
            net = self.model
            for name, sl in self.tab.slices.items():
                off, n, shape = net._offs[name]
                d = (net.flat_grad[off:off + n].view(shape[0], -1) * self.w0[off:off + n].view(shape[0], -1)).sum(1) * scale
                gmask[sl] = gmask[sl] + d if accumulate else d
                bias = name[:-6] + "bias"
                if gxi is not None and bias in net._offs:
                    bo, bn, _ = net._offs[bias]
                    d = net.flat_grad[bo:bo + bn] * self.w0[bo:bo + bn] * scale
                    gxi[sl] = gxi[sl] + d if accumulate else d

    class BarePasses(anp._Passes):
        """The other families' leg B: the step's three forward + backward passes at the base weights, no neuron kernel."""

        def write(self, mask, delta, xi):
            pass

        def step(self, st, x_t, y, t, start, cfg, curves):
            for k in range(3):
                self.run(x_t, y, t, st.mask, None, None, curves[k:k + 1])

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    family, label, leg_b = None, "UNet2DModel CIFAR10 32x32", TorchPasses
    if args.family == "ve":
        from villandiffusion_amd import anp_ve
        from villandiffusion_amd.ncsnpp import NCSNppModel
        net, sched, label, leg_b = NCSNppModel(), S.ScoreSdeVeScheduler(), "NCSNppModel 32x32 (the default)", BarePasses
    elif args.family == "ldm":
        from villandiffusion_amd.loss import SDE_LDM, LossFn
        from villandiffusion_amd.model import LDM_CELEBA_UNET_ARCH
        net, sched = UNet2DModel(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in LDM_CELEBA_UNET_ARCH.items()}), S.DDIMScheduler()
        label, leg_b = "LDM-CELEBA-HQ-256 latent UNet, 3x64x64 latents", BarePasses
    else:
        net, sched = UNet2DModel(), S.DDPMScheduler()
    net.reset_parameters(0)
    if args.family == "ve":
        family = anp_ve._family(net, sched)
    elif args.family == "ldm":
        family = anp._vp_family(sched, LossFn(sched, SDE_LDM, psi=1))
    b_key = "torch_ms" if args.family == "vp" else "passes_ms"
    tab = anp.neuron_table(net, "all")
    n, B = tab.n_neurons, args.batch
    Sz = int(net.sample_size)
    gen = torch.Generator().manual_seed(0)
    x0 = torch.rand(B, 3, Sz, Sz, generator=gen)
    x0 = (x0 if args.family == "ve" else x0 * 2 - 1).to(dev)           # the family's value range
    eps = torch.randn(B, 3, Sz, Sz, generator=gen).to(dev)
    t = torch.randint(0, int(sched.config.num_train_timesteps), (B,), generator=gen).to(dev)
    start = ((torch.rand(2, n, generator=gen) * 2 - 1) * 0.4).to(dev)
    cfg = SimpleNamespace(anp_eps=0.4, anp_steps=1, anp_alpha=0.2, lr=0.0, momentum=0.9)       # lr 0: every step of both legs sees the mask at 1
    curves = torch.zeros(3, device=dev)
    before = net.flat_param.clone()
    rows = {"kernels_ms": [], b_key: []}
    with _trainable(net, family.skip if family is not None else ()):
        legs = {"kernels_ms": anp._Passes(net, sched, tab, family), b_key: leg_b(net, sched, tab, family)}
        states = {k: anp._state(n, dev) for k in legs}
        try:
            x_t, y = legs["kernels_ms"].inputs(x0, eps, t)
            fns = {k: (lambda k=k: legs[k].step(states[k], x_t, y, t, start, cfg, curves)) for k in legs}
            for rnd in range(args.rounds):
                for key, fn in fns.items():
                    for _ in range(args.warmup):
                        fn()
                    rows[key].append(timed(torch, fn, args.steps))
                print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
            # the two legs computed the same step: delta after the ascent, and the mask gradient up to the order of the row sums
            a, b = states["kernels_ms"], states[b_key]
            if args.family == "vp":
                same_delta = float((a.delta != b.delta).float().mean())
                gm_rel = float((a.gm - b.gm).abs().max() / b.gm.abs().max())

            # ---- the kernels alone ----
            ps = legs["kernels_ms"]
            g = net.flat_grad
            kern = {"neuron_scale": {"bytes": 8.0 * (tab.weight_floats + tab.n_bias) + 12.0 * n, "us": []},
                    "neuron_grad": {"bytes": 8.0 * (tab.weight_floats + tab.n_bias) + 8.0 * n, "us": []}}
            calls = {"neuron_scale": lambda: ops.neuron_scale(ps.w0, net.flat_param, tab, a.mask, a.delta, a.xi),
                     "neuron_grad": lambda: ops.neuron_grad(g, ps.w0, tab, a.gd, a.gx)}
            for rnd in range(args.rounds):
                for name, f in calls.items():
                    for _ in range(3):
                        f()
                    kern[name]["us"].append(1e3 * timed(torch, f, 20))
        finally:
            for leg in legs.values():
                leg.restore()
    assert torch.equal(net.flat_param, before)
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kern.items():
        kk["us_median"] = med(kk["us"])
        kk["TB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e12
        kk["fraction_of_8TBps"] = kk["TB_per_s"] / 8.0
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['TB_per_s']:.3f} TB/s", flush=True)
    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    if args.family == "vp":
        summary["kernels_over_torch"] = summary["kernels_ms_median"] / summary["torch_ms_median"]
        summary["delta_mismatch_share"] = same_delta
        summary["mask_gradient_max_rel_diff"] = gm_rel
    else:
        summary["kernels_over_passes"] = summary["kernels_ms_median"] / summary["passes_ms_median"]
    out = {"config": {"model": label, "parameters": net.flat_numel, "batch": B, "layers": "all", "neurons": n,
                      "jobs": tab.n_jobs, "selected_floats": tab.weight_floats, "anp_steps": 1, "passes_per_step": 3, "rounds": args.rounds,
                      "steps": args.steps, "warmup": args.warmup, "conv_math": net.conv_math, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kern, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    if args.family != "vp":                                # one file for both families: this run's record replaces its own, the other stays
        held = json.load(open(args.out)) if os.path.exists(args.out) else {}
        out = held | {args.family: out}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
