"""Interleaved A/B of the three bf16-matrix-core arithmetics on one box: "bf16x3" (default), "bf16" (one bf16 product per term, opt-in) and "f16"
(one f16 product in the forward / input-gradient convolutions, opt-in).  Per round and mode: training ms/step at the bench's configuration (CIFAR10
32x32 UNet, B = 128, SDE-VP loss, Adam) and sampling img/s of a DDIM-50 loop over 1 024 images in chunks of 128 (a proxy for DDPM-1000: the same
forward per step, 1/20 of the steps).  The modes alternate inside every round, so clock / thermal drift hits all of them alike.
   python tools/bf16_mode_ab.py [--rounds 3] [--steps 10] [--out profiles/r07_bf16_mode_ab.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.pipelines import DDIMPipeline  # noqa: E402
from villandiffusion_amd.trainer import Trainer  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

MODES = ("bf16x3", "bf16", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="timed training steps per round and mode")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024, help="sampled images per round and mode (0: training only)")
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--infer-steps", type=int, default=50)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset (e.g. one mode under a kernel-trace profiler)")
    ap.add_argument("--out", default=os.path.join("profiles", "r07_bf16_mode_ab.json"))
    args = ap.parse_args()
    modes = tuple(args.modes.split(","))
    assert modes and all(m in MODES for m in modes), modes
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = 128
    net = UNet2DModel()
    net.reset_parameters(0)
    tr = Trainer(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), lr=2e-4, total_steps=10_000)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn(B, 3, 32, 32, device="cuda", generator=gen).clamp(-1, 1)
    R = torch.zeros_like(x0)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=gen)
    inits = torch.randn(args.images, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    rows = {m: {"train_ms": [], "sample_img_s": [], "loss": []} for m in modes}
    for rnd in range(args.rounds):
        for mode in modes:
            net.conv_math = mode
            for _ in range(args.warmup):
                tr.train_step({"target": x0, "pixel_values": R}, t)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                loss = tr.train_step({"target": x0, "pixel_values": R}, t)
            e1.record()
            torch.cuda.synchronize()
            rows[mode]["train_ms"].append(e0.elapsed_time(e1) / args.steps)
            rows[mode]["loss"].append(float(loss))
            if args.images <= 0:                                # training only (a kernel-trace run of the step)
                print(f"round {rnd} {mode:7s}: train {rows[mode]['train_ms'][-1]:7.2f} ms/step", flush=True)
                continue
            pipe = DDIMPipeline(net, S.DDIMScheduler(clip_sample=False))
            pipe(batch_size=args.chunk, init=inits[:args.chunk], num_inference_steps=2, return_tensor=True)   # graph capture outside the timing
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c0 in range(0, args.images, args.chunk):
                pipe(batch_size=args.chunk, init=inits[c0:c0 + args.chunk], num_inference_steps=args.infer_steps, return_tensor=True)
            torch.cuda.synchronize()
            rows[mode]["sample_img_s"].append(args.images / (time.perf_counter() - t0))
            print(f"round {rnd} {mode:7s}: train {rows[mode]['train_ms'][-1]:7.2f} ms/step, DDIM-{args.infer_steps} "
                  f"{rows[mode]['sample_img_s'][-1]:7.1f} img/s", flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {m: {"train_ms_median": med(rows[m]["train_ms"])} for m in modes}
    for m in modes:
        if rows[m]["sample_img_s"]:
            summary[m]["sample_img_s_median"] = med(rows[m]["sample_img_s"])
        if "bf16x3" in summary:
            summary[m]["train_vs_bf16x3"] = summary["bf16x3"]["train_ms_median"] / summary[m]["train_ms_median"]
            if rows[m]["sample_img_s"]:
                summary[m]["sample_vs_bf16x3"] = summary[m]["sample_img_s_median"] / summary["bf16x3"]["sample_img_s_median"]
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "batch": B, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
                      "sampler": f"DDIM-{args.infer_steps}", "images": args.images, "chunk": args.chunk,
                      "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
