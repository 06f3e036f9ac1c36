"""Interleaved timing on one box for the optimiser step with an EMA of the weights, on config #2's flat buffer (CIFAR10 32x32 UNet, 35.7 M
parameters; the gradient is random data: every kernel here is a stream over flat f32 buffers, whatever they hold):
 * "adam": `FusedAdam.step()` without EMA -- the norm kernel (4 B/parameter) and adam_kernel (28 B/parameter);
 * "fused": the same step with `ema=EMAConfig()` -- the norm kernel and adam_ema_kernel (36 B/parameter), one launch for both updates;
 * "two_launch": "adam" followed by the shadow update as it could be written without a new kernel, `ops.lincomb(ema, [ema, p], [d, 1 - d])`
   (12 B/parameter more in a second launch: 40 B/parameter after the norm) -- ms per step, alternating inside every round; the spread of each
   over the rounds is the same-box run-to-run spread the differences are to be read against;
 * the kernels alone, bytes over time: vd_adam_step, vd_adam_ema_step and vd_swap (16 B/element) on the same buffers.
   python tools/ema_step_ab.py [--rounds 3] [--steps 20] [--out profiles/r10_ema_ab.json]
Run it under a time limit of its own (`timeout -k 10 300 python tools/ema_step_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.trainer import EMAConfig, FusedAdam, ema_decay_at  # noqa: E402
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r10_ema_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    n = net.flat_numel
    net.flat_grad.copy_(torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 1e-3)
    cfg = EMAConfig()
    plain = FusedAdam(net, 1e-6, max_grad_norm=1.0)
    fused = FusedAdam(net, 1e-6, max_grad_norm=1.0, ema=cfg)
    shadow = [net.flat_param.detach().clone(), torch.empty_like(net.flat_param)]      # lincomb's output must not alias a source: two buffers, in turn
    k = [0]

    def two_launch():
        plain.step()
        k[0] += 1
        d = ema_decay_at(k[0], cfg)
        ops.lincomb(shadow[1], [shadow[0], net.flat_param], [d, 1.0 - d])
        shadow.reverse()

    steps = {"adam_ms": plain.step, "fused_ms": fused.step, "two_launch_ms": two_launch}
    rows = {key: [] for key in steps}
    for rnd in range(args.rounds):
        for key, fn in steps.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.4f} ms" for key, v in rows.items()), flush=True)

    # ---- the kernels alone ----
    p, g, m, v, e = net.flat_param, net.flat_grad, plain.exp_avg, plain.exp_avg_sq, fused.ema
    kern = {"adam_step": {"bytes": 28.0 * n, "us": []}, "adam_ema_step": {"bytes": 36.0 * n, "us": []}, "swap": {"bytes": 16.0 * n, "us": []}}
    calls = {"adam_step": lambda: ops.adam_step(p, g, m, v, None, 1.0, 1.0, 1e-6, 0.9, 0.999, 1e-8, 10),
             "adam_ema_step": lambda: ops.adam_ema_step(p, g, m, v, e, None, 1.0, 1.0, 1e-6, 0.9, 0.999, 1e-8, 10, 1e-4),
             "swap": lambda: ops.swap(p, e)}
    for rnd in range(args.rounds):
        for name, f in calls.items():
            for _ in range(2 * ((args.warmup + 1) // 2)):                          # even counts, warm-up and timed: the swaps cancel
                f()
            kern[name]["us"].append(1e3 * timed(f, 2 * (args.steps // 2)))
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kern.items():
        kk["us_median"] = med(kk["us"])
        kk["TB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e12
        kk["fraction_of_8TBps"] = kk["TB_per_s"] / 8.0
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['TB_per_s']:.3f} TB/s", flush=True)

    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    summary["fused_over_adam"] = summary["fused_ms_median"] / summary["adam_ms_median"]
    summary["fused_over_adam_from_bytes"] = (4.0 + 36.0) / (4.0 + 28.0)            # the norm kernel's read of the gradient is in both
    summary["fused_over_two_launch"] = summary["fused_ms_median"] / summary["two_launch_ms_median"]
    summary["fused_beats_two_launch"] = summary["fused_ms_median"] < summary["two_launch_ms_median"]
    summary["kernel_adam_ema_over_adam"] = kern["adam_ema_step"]["us_median"] / kern["adam_step"]["us_median"]
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kern, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
