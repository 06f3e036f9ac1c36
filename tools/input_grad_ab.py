"""Interleaved A/B on one box for the input-gradient work (config #2: CIFAR10 32x32 UNet, B = 128, default arithmetic):
 * "full": forward + the full backward (weight gradients into the flat gradient, no sample gradient: a training step's pass) against "input": forward + the
   input-gradient pass of the frozen network -- ms per pass, alternating inside every round;
 * conv_in's input gradient (dY[B, 128, 32, 32] -> dX[B, 3, 32, 32]) on the flipped-tap few-output kernel against the generic exact-f32 MFMA
   tiles (vd_gemm_desc.tile forced), us per launch;
 * one trigger-inversion iteration at batch 100, ms (information only).
   python tools/input_grad_ab.py [--rounds 3] [--steps 10] [--out profiles/r08_input_grad_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/input_grad_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import defense, ops  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.lib import B_CONV3_T  # noqa: E402
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r08_input_grad_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    B = 128
    net = UNet2DModel()
    net.reset_parameters(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=gen)
    w = torch.randn(B, 3, 32, 32, device="cuda", generator=gen)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=gen)

    def one_pass(frozen):
        net.requires_grad_(not frozen)
        if frozen:                                        # forward + the input-gradient pass
            xx = x.detach().requires_grad_(True)
            torch.autograd.grad(net(xx, t)[0], xx, w)
        else:                                             # forward + the full backward as a training step runs it (no sample gradient)
            net(x, t)[0].backward(w)

    rows = {"full_ms": [], "input_ms": []}
    for rnd in range(args.rounds):
        for key, frozen in (("full_ms", False), ("input_ms", True)):
            for _ in range(args.warmup):
                one_pass(frozen)
            rows[key].append(timed(lambda: one_pass(frozen), args.steps))
        net.zero_grad()
        print(f"round {rnd}: full {rows['full_ms'][-1]:.3f} ms, input-gradient pass {rows['input_ms'][-1]:.3f} ms", flush=True)
    net.requires_grad_(True)

    # ---- conv_in's input gradient: the flipped-tap kernel against the generic tiles ----
    dy = torch.randn(B, 128, 32, 32, device="cuda", generator=gen)
    wt = torch.randn(3, 128 * 9, device="cuda", generator=gen)
    dx = torch.empty(B, 3, 32, 32, device="cuda")
    conv = {}
    for rnd in range(args.rounds):
        for name, tile in (("fewout_flip", 0), ("generic_tile2", 2), ("generic_tile3", 3)):
            f = lambda: ops.conv3x3(dy, wt, None, dx, mode=B_CONV3_T, tile=tile)
            for _ in range(args.warmup):
                f()
            conv.setdefault(name, {"us": [], "vd_gemm_tile": None})
            conv[name]["us"].append(1e3 * timed(f, 20))
            conv[name]["vd_gemm_tile"] = int(ops.LAST_GEMM_TILE)
        print(f"round {rnd}: conv_in dgrad " + ", ".join(f"{k} {v['us'][-1]:.1f} us" for k, v in conv.items()), flush=True)

    # ---- one trigger-inversion iteration at batch 100 ----
    n_it = 6
    sched = S.DDPMScheduler()
    defense.invert_trigger(net, sched, steps=2, batch=100)                      # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    defense.invert_trigger(net, sched, steps=n_it, batch=100)
    e1.record()
    torch.cuda.synchronize()
    inv_ms = e0.elapsed_time(e1) / n_it

    med = lambda v: sorted(v)[len(v) // 2]
    summary = {"full_ms_median": med(rows["full_ms"]), "input_ms_median": med(rows["input_ms"]),
               "input_faster_in_every_round": all(i < f for i, f in zip(rows["input_ms"], rows["full_ms"])),
               "conv_in_dgrad_us_median": {k: med(v["us"]) for k, v in conv.items()},
               "inversion_iteration_ms_batch100": inv_ms}
    summary["input_vs_full"] = summary["input_ms_median"] / summary["full_ms_median"]
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "batch": B, "conv_math": net.conv_math, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "conv_in_dgrad": conv, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
