"""Interleaved timing on one box for the curve (Mode Connectivity Repair) optimiser step, on config #2 (CIFAR10 32x32 UNet, 35.7 M parameters,
batch 128), one network shared by the arms (lr = 1e-6: nothing moves far):
 * "plain":     one eager step -- forward + backward, the norm kernel, the Adam kernel on the weights (`trainer.FusedAdam`);
 * "curve":     `curve.curve_step` with a `CurveAdam` -- the same with Adam on the bend, plus one vd_curve_point launch (16 B/float);
 * "torch_ops": the curve step with the point formed by torch ops on the flat buffers, (ca * A + cm * theta) + cb * B and a copy into
   flat_param (what the kernel replaces: three temporaries the size of the network)
   -- ms per step, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are
   to be read against;
 * vd_curve_point and vd_curve_geometry alone over the whole flat buffer, GB/s against their algorithmic bytes, beside vd_anchor_grad (L2-SP,
   also 16 B/float) and vd_sam_norm_sq in the same run.  vd_curve_point below 0.8x vd_anchor_grad's rate is flagged in the summary.
   python tools/curve_step_ab.py [--rounds 3] [--steps 10] [--out profiles/r20_curve_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/curve_step_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n):
    import torch
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join("profiles", "r20_curve_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    from villandiffusion_amd import ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.curve import Curve, CurveAdam, CurveConfig, coefficients, curve_step, draw_t
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import FusedAdam
    from villandiffusion_amd.unet import UNet2DModel

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
    start = net.flat_param.detach().clone()
    end_a = start + 0.005 * torch.randn(n, device="cuda", generator=gen)
    end_b = start + 0.005 * torch.randn(n, device="cuda", generator=gen)
    # t in [0.4, 0.6]: every arm trains a network close to `start`, whichever arm ran before it
    cfg = CurveConfig(t_min=0.4, t_max=0.6)
    lf.grad_scale = 1.0
    plain = FusedAdam(net, 1e-6)
    cv = Curve(net, end_a, end_b, cfg)
    opt = CurveAdam(cv, 1e-6)

    def backward():
        loss = lf.p_loss_by_keys(batch, net, target_latent_key="target", poison_latent_key="pixel_values", timesteps=t, noise=eps)
        loss.backward()

    def plain_step():
        backward()
        plain.step()
        net.zero_grad()

    def torch_ops():
        backward()
        opt.step_count += 1
        ops.l2norm_sq(net.flat_grad, opt._partial, opt.grad_norm_sq)
        ops.adam_step(cv.theta, net.flat_grad, opt.exp_avg, opt.exp_avg_sq, opt.grad_norm_sq, 1.0, opt.cm, 1e-6, 0.9, 0.999, 1e-8,
                      opt.step_count, skipped=opt.skipped, weights=False)
        opt.t = draw_t(opt.gen, cfg)
        ca, cm, cb = coefficients(cfg.kind, opt.t)
        opt.cm = cm
        with torch.no_grad():
            net.flat_param.copy_((ca * cv.wa + cm * cv.theta) + cb * cv.wb)
        ops.WEIGHTS_EPOCH += 1
        net.weights_changed()
        net.zero_grad()

    steps = {"plain_ms": plain_step, "curve_ms": lambda: curve_step(net, opt, lf, x0, R, t, noise=eps), "torch_ops_ms": torch_ops}
    rows = {key: [] for key in steps}
    for rnd in range(args.rounds):
        for key, fn in steps.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)

    # ---- the kernels alone, over the whole flat buffer ----
    w = net.flat_param
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    out = torch.empty_like(w)
    partial, nsq, out3 = torch.empty(3 * 1024, device="cuda"), torch.ones(1, device="cuda"), torch.zeros(3, device="cuda")
    kern = {"curve_point": (16.0 * n, lambda: ops.curve_point(out, cv.wa, cv.theta, cv.wb, 0.25, 0.5, 0.25, weights=False)),
            "curve_geometry": (12.0 * n, lambda: ops.curve_geometry(cv.wa, cv.theta, cv.wb, partial, out3)),
            "anchor_grad_l2sp": (16.0 * n, lambda: ops.anchor_grad(g, w, end_a, None, 1e-6, partial, nsq)),
            "anchor_grad_l2sp_no_penalty": (16.0 * n, lambda: ops.anchor_grad(g, w, end_a, None, 1e-6)),
            "sam_norm_sq_asam": (8.0 * n, lambda: ops.sam_norm_sq(g, w, partial, nsq, "asam")),
            "l2norm_sq": (4.0 * n, lambda: ops.l2norm_sq(g, partial, nsq))}
    kernels = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(2):
                f()
            kernels[name]["us"].append(1e3 * timed(f, 2 * max(1, args.steps)))
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kernels.items():
        kk["us_median"] = med(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)

    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    for k in ("curve", "torch_ops"):
        summary[k + "_minus_plain_ms"] = summary[k + "_ms_median"] - summary["plain_ms_median"]
        summary[k + "_over_plain"] = summary[k + "_ms_median"] / summary["plain_ms_median"]
    summary["kernel_beats_torch_ops"] = summary["curve_ms_median"] < summary["torch_ops_ms_median"]
    summary["curve_point_over_anchor_grad_rate"] = kernels["curve_point"]["GB_per_s"] / kernels["anchor_grad_l2sp_no_penalty"]["GB_per_s"]
    summary["curve_point_below_0.8x_anchor_grad"] = summary["curve_point_over_anchor_grad_rate"] < 0.8
    res = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "batch": B, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kernels, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
