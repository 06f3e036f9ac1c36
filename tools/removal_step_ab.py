"""Interleaved timing on one box for the backdoor-removal step (config #2: CIFAR10 32x32 UNet, default arithmetic):
 * "removal": one step of mitigation.remove_backdoor at batch 64 -- the frozen teacher's captured forward at 64, the training forward and
   backward at 128, the input build, vd_removal_loss and clip + Adam;
 * "parts": what the project already had for the same work -- one Trainer.train_step at batch 128 (q-sample, forward, MSE, backward, clip +
   Adam) plus one pipelines.sampler_forward at 64 -- ms per step, alternating inside every round; the spread of each over the rounds is the
   same-box run-to-run spread the difference is to be read against;
 * the two new kernels alone, bytes over time: vd_removal_loss at B = 64 and vd_image_set_stats at N = 1024, 3 x 32 x 32.
   python tools/removal_step_ab.py [--rounds 3] [--steps 10] [--out profiles/r09_mitigation.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/removal_step_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from villandiffusion_amd import mitigation, ops  # noqa: E402
from villandiffusion_amd.defense import _noise_of  # noqa: E402
from villandiffusion_amd import schedulers as S  # noqa: E402
from villandiffusion_amd.loss import LossFn  # noqa: E402
from villandiffusion_amd.pipelines import sampler_forward  # noqa: E402
from villandiffusion_amd.trainer import FusedAdam, Trainer  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join("profiles", "r09_mitigation.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    B = 64
    gen = torch.Generator(device="cuda").manual_seed(0)
    shape = (3, 32, 32)

    # ---- the removal step, as remove_backdoor runs it: the two calls mitigation._run_removal makes per iteration ----
    net = UNet2DModel()
    net.reset_parameters(0)
    tau = torch.rand(shape, device="cuda", generator=gen)
    frozen = mitigation._frozen_copy(net)
    teacher = sampler_forward(frozen, B)
    opt = FusedAdam(net, 1e-5, max_grad_norm=1.0)
    terms = torch.zeros(3, device="cuda")
    partial = torch.empty(2048, device="cuda")
    t2 = torch.full((2 * B,), 999.0, device="cuda")
    eps = torch.empty((B,) + shape, device="cuda")
    per_iter = (eps.numel() + 3) // 4
    it = [0]

    def removal_step():
        it[0] += 1
        mitigation._removal_step(net, teacher, opt, tau, _noise_of("removal_step_ab", None, it[0] - 1, eps, 0, per_iter, "cuda"), t2, 1.0, 1.0,
                                 terms, partial)

    # ---- the parts it is made of, as they existed: a training step at 2B and a sampler forward at B (a network of its own) ----
    net2 = UNet2DModel()
    net2.reset_parameters(0)
    lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
    tr = Trainer(net2, lf, lr=1e-5, total_steps=10 ** 6, warmup_steps=0)
    x0 = torch.rand((2 * B,) + shape, device="cuda", generator=gen) * 2 - 1
    batch = {"target": x0, "pixel_values": torch.zeros_like(x0)}
    tt = torch.randint(0, 1000, (2 * B,), device="cuda", generator=gen)
    net3 = mitigation._frozen_copy(net2)
    fwd = sampler_forward(net3, B)
    xs = torch.randn((B,) + shape, device="cuda", generator=gen)

    def train_step():
        tr.train_step(batch, tt)

    def parts_step():
        train_step()
        fwd(xs, t2[:B])

    rows = {"removal_ms": [], "parts_ms": [], "train_step_128_ms": [], "sampler_forward_64_ms": []}
    for rnd in range(args.rounds):
        for key, fn in (("removal_ms", removal_step), ("parts_ms", parts_step), ("train_step_128_ms", train_step),
                        ("sampler_forward_64_ms", lambda: fwd(xs, t2[:B]))):
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{k[:-3]} {v[-1]:.3f} ms" for k, v in rows.items()), flush=True)

    # ---- the two kernels alone ----
    pred = torch.randn((2 * B,) + shape, device="cuda", generator=gen)
    ref = torch.randn((B,) + shape, device="cuda", generator=gen)
    dpred = torch.empty_like(pred)
    N = 1024
    imgs = torch.randn((N,) + shape, device="cuda", generator=gen)
    mean, stats = torch.empty(shape, device="cuda"), torch.empty(2, device="cuda")
    kern = {"removal_loss_B64": {"bytes": 4.0 * 5 * ref.numel(), "us": []},                       # pred 2B + ref B read, dpred 2B written
            "image_set_stats_N1024": {"bytes": 4.0 * (2 * imgs.numel() + 2 * mean.numel()), "us": []}}   # x read by both passes
    calls = {"removal_loss_B64": lambda: ops.removal_loss(pred, ref, 1.0, 1.0, dpred, terms, partial),
             "image_set_stats_N1024": lambda: ops.image_set_stats(imgs, mean, stats, partial)}
    for rnd in range(args.rounds):
        for name, f in calls.items():
            for _ in range(args.warmup):
                f()
            kern[name]["us"].append(1e3 * timed(f, 50))
    med = lambda v: sorted(v)[len(v) // 2]
    for name, k in kern.items():
        k["us_median"] = med(k["us"])
        k["TB_per_s"] = k["bytes"] / (k["us_median"] * 1e-6) / 1e12
        k["fraction_of_8TBps"] = k["TB_per_s"] / 8.0
        print(f"{name}: {k['us_median']:.1f} us, {k['bytes'] / 1e6:.2f} MB, {k['TB_per_s']:.3f} TB/s", flush=True)

    spread = lambda v: max(v) - min(v)
    summary = {k + "_median": med(v) for k, v in rows.items()} | {k + "_spread": spread(v) for k, v in rows.items()}
    summary["removal_minus_parts_ms"] = summary["removal_ms_median"] - summary["parts_ms_median"]
    summary["within_run_to_run_spread"] = summary["removal_minus_parts_ms"] <= max(summary["removal_ms_spread"], summary["parts_ms_spread"])
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "batch": B, "conv_math": net.conv_math, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kern, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
