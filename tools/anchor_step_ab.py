"""Interleaved timing on one box for the anchored optimiser step, on config #2 (CIFAR10 32x32 UNet, 35.7 M parameters, batch 128), one
network shared by the arms (lr = 1e-6: it barely moves):
 * "plain":     `Trainer.train_step` -- one forward + backward, the norm kernel, the Adam kernel;
 * "l2sp":      `Trainer(anchor=AnchorConfig(lam))` -- the same plus one vd_anchor_grad launch (16 B/float) and its one-workgroup finish;
 * "ewc":       `Trainer(anchor=AnchorConfig(lam, "ewc", F))` -- the launch reads F too (20 B/float);
 * "torch_ops": the plain step with EWC written as torch ops on the flat buffers before the norm, g.add_(lam * F * (w - w0)) plus the penalty
   sum (what the kernel replaces)
   -- ms per step, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are
   to be read against;
 * vd_fisher_accum and vd_anchor_grad alone over the whole flat buffer, GB/s against their algorithmic bytes, beside vd_sam_perturb and
   vd_l2norm_sq in the same run.
   python tools/anchor_step_ab.py [--rounds 3] [--steps 10] [--out profiles/r18_anchor_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/anchor_step_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.anchor import AnchorConfig  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.trainer import Trainer  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join("profiles", "r18_anchor_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    n, B, lam = net.flat_numel, args.batch, 0.1
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
    R = torch.rand(B, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
    R[: B // 2] = 0
    eps = torch.randn(B, 3, 32, 32, device="cuda", generator=gen)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=gen)
    batch = {"target": x0, "pixel_values": R}
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    F = torch.exp(1.5 * torch.randn(n, device="cuda", generator=gen) - 1.125)
    w0 = net.flat_param.detach() + 0.005 * torch.randn(n, device="cuda", generator=gen)
    mk = lambda a=None: Trainer(net, lf, lr=1e-6, total_steps=10 ** 6, warmup_steps=0, anchor=a, anchor_weights=None if a is None else w0)
    plain, l2sp, ewc = mk(), mk(AnchorConfig(lam=lam)), mk(AnchorConfig(lam=lam, mode="ewc", fisher=F))
    pen = torch.zeros(1, device="cuda")

    def torch_ops():
        loss = lf.p_loss_by_keys(batch, net, target_latent_key="target", poison_latent_key="pixel_values", timesteps=t, noise=eps)
        loss.backward()
        with torch.no_grad():
            d = net.flat_param - w0
            td = F * d
            net.flat_grad.add_(td, alpha=lam)
            pen.copy_((td * d).sum())
        plain.opt.step(lr=plain.lr)
        plain.sched_step += 1
        net.zero_grad()

    steps = {"plain_ms": lambda: plain.train_step(batch, t, noise=eps), "l2sp_ms": lambda: l2sp.train_step(batch, t, noise=eps),
             "ewc_ms": lambda: ewc.train_step(batch, t, noise=eps), "torch_ops_ms": torch_ops}
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
    Facc, backup = torch.zeros_like(w), torch.empty_like(w)
    partial, nsq = torch.empty(1024, device="cuda"), torch.ones(1, device="cuda")
    kern = {"l2norm_sq": (4.0 * n, lambda: ops.l2norm_sq(g, partial, nsq)),
            "sam_perturb_sam": (16.0 * n, lambda: ops.sam_perturb(w, g, backup, nsq, 1e-6, "sam")),
            "fisher_accum": (12.0 * n, lambda: ops.fisher_accum(Facc, g, 1e-3)),
            "anchor_grad_l2sp": (16.0 * n, lambda: ops.anchor_grad(g, w, w0, None, 1e-6, partial, pen)),
            "anchor_grad_ewc": (20.0 * n, lambda: ops.anchor_grad(g, w, w0, F, 1e-6, partial, pen)),
            "anchor_grad_ewc_no_penalty": (20.0 * n, lambda: ops.anchor_grad(g, w, w0, F, 1e-6))}
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
    for k in ("l2sp", "ewc", "torch_ops"):
        summary[k + "_minus_plain_ms"] = summary[k + "_ms_median"] - summary["plain_ms_median"]
        summary[k + "_over_plain"] = summary[k + "_ms_median"] / summary["plain_ms_median"]
    summary["kernel_beats_torch_ops"] = summary["ewc_ms_median"] < summary["torch_ops_ms_median"]
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "batch": B, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "lambda": lam, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kernels, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
