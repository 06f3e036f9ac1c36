"""Interleaved timing on one box for the sharpness-aware optimiser step, on config #2 (CIFAR10 32x32 UNet, 35.7 M parameters, batch 128), one
network shared by the arms (lr = 1e-6: it barely moves):
 * "plain":  `Trainer.train_step` -- one forward + backward, the norm kernel, the Adam kernel;
 * "floor":  two plain forward + backward passes and one optimiser step -- what a SAM step costs before any whole-buffer pass;
 * "sam" / "asam" / "neuron": `Trainer(sam=SAMConfig(...))` with the kernels of vd_sam.hip (norm, perturb + backup, restore);
 * "torch_ops": SAM with the norm, the perturbation, the backup and the restore written as per-parameter torch ops (what the kernels replace)
   -- ms per step, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are
   to be read against;
 * the new kernels alone over the whole flat buffer, GB/s against their algorithmic bytes, beside vd_l2norm_sq and vd_swap in the same run.
   python tools/sam_step_ab.py [--rounds 3] [--steps 10] [--out profiles/r16_sam_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/sam_step_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import anp, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.trainer import SAMConfig, Trainer  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join("profiles", "r16_sam_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    n, B = net.flat_numel, args.batch
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
    R = torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
    R[: B // 2] = 0
    eps = torch.randn(B, 3, 32, 32, device="cuda", generator=gen)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=gen)
    batch = {"target": x0, "pixel_values": R}
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    mk = lambda sam=None: Trainer(net, lf, lr=1e-6, total_steps=10 ** 6, warmup_steps=0, sam=sam)
    plain = mk()
    cfgs = {"sam": SAMConfig(rho=0.05), "asam": SAMConfig(rho=0.5, mode="asam"), "neuron": SAMConfig(rho=0.5, mode="neuron")}
    sams = {k: mk(c) for k, c in cfgs.items()}
    params = [p for p in net.parameters()]

    def one_pass():
        loss = lf.p_loss_by_keys(batch, net, target_latent_key="target", poison_latent_key="pixel_values", timesteps=t, noise=eps)
        loss.backward()

    def finish(tr):
        tr.opt.step(lr=tr.lr)
        tr.sched_step += 1
        net.zero_grad()

    def floor():
        one_pass()
        net.zero_grad()
        one_pass()
        finish(plain)

    def torch_ops():
        one_pass()
        with torch.no_grad():
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
            c = 0.05 / (norm + 1e-12)
            backup = [p.detach().clone() for p in params]
            for p in params:
                p.add_(p.grad * c)
        ops.WEIGHTS_EPOCH += 1
        net.weights_changed()
        net.zero_grad()
        one_pass()
        with torch.no_grad():
            for p, b in zip(params, backup):
                p.copy_(b)
        ops.WEIGHTS_EPOCH += 1
        net.weights_changed()
        finish(plain)

    steps = {"plain_ms": lambda: plain.train_step(batch, t, noise=eps), "floor_ms": floor}
    steps.update({k + "_ms": (lambda tr=tr: tr.train_step(batch, t, noise=eps)) for k, tr in sams.items()})
    steps["torch_ops_ms"] = torch_ops
    rows = {key: [] for key in steps}
    for rnd in range(args.rounds):
        for key, fn in steps.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)

    # ---- the kernels alone, over the whole flat buffer ----
    w, keep = net.flat_param, net.flat_param.detach().clone()
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    backup, other = torch.empty_like(w), torch.empty_like(w)
    partial, nsq = torch.empty(1024, device="cuda"), torch.ones(1, device="cuda")
    tab = anp.neuron_table(net, "conv")
    wsq, gsq, coef = (torch.zeros(tab.n_neurons, device="cuda") for _ in range(3))
    rows_b = 4.0 * tab.weight_floats + 4.0 * tab.n_neurons      # vd_neuron_grad(g, g): both operands are the same rows, read from HBM once
    kern = {"l2norm_sq": (4.0 * n, lambda: ops.l2norm_sq(g, partial, nsq)),
            "sam_norm_sq_asam": (8.0 * n, lambda: ops.sam_norm_sq(g, w, partial, nsq, "asam", 0.01)),
            "sam_perturb_sam": (16.0 * n, lambda: ops.sam_perturb(w, g, backup, nsq, 1e-6, "sam")),
            "sam_perturb_asam": (16.0 * n, lambda: ops.sam_perturb(w, g, backup, nsq, 1e-6, "asam", 0.01)),
            "neuron_grad_rows": (rows_b, lambda: ops.neuron_grad(g, g, tab, gsq)),
            "sam_neuron_coef": (20.0 * tab.n_neurons, lambda: ops.sam_neuron_coef(wsq, gsq, tab, coef, nsq, 1e-6, 0.01)),
            "neuron_axpy": (12.0 * tab.weight_floats + 4.0 * tab.n_neurons, lambda: ops.neuron_axpy(w, g, tab, coef)),
            "restore_copy": (8.0 * n, lambda: other.copy_(backup)),
            "swap": (16.0 * n, lambda: ops.swap(other, backup))}
    ops.neuron_grad(w, w, tab, wsq)
    kernels = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(2):
                f()
            kernels[name]["us"].append(1e3 * timed(f, 2 * max(1, args.steps)))
    w.copy_(keep)
    ops.WEIGHTS_EPOCH += 1
    net.weights_changed()
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kernels.items():
        kk["us_median"] = med(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)

    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    for k in ("sam", "asam", "neuron", "torch_ops"):
        summary[k + "_over_floor"] = summary[k + "_ms_median"] / summary["floor_ms_median"]
        summary[k + "_minus_floor_ms"] = summary[k + "_ms_median"] - summary["floor_ms_median"]
    summary["sam_over_plain"] = summary["sam_ms_median"] / summary["plain_ms_median"]
    summary["kernels_beat_torch_ops"] = summary["sam_ms_median"] < summary["torch_ops_ms_median"]
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "batch": B, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "neurons": tab.n_neurons, "neuron_weight_floats": tab.weight_floats,
                      "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kernels, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
