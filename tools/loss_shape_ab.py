"""Interleaved timing on one box of the shaped loss (vd_loss_sample_fwd_bwd; LossFn snr_gamma / poison_weight / track_split):
 (a) the kernel alone against vd_loss_fwd_bwd at [128, 3, 32, 32] and [8, 3, 256, 256], forward + gradient: microseconds, and achieved bytes/s
     over the algorithmic bytes 4 * 3 * B * chw (pred and y read, dpred written), alternating inside every round;
 (b) one optimiser step of the fine-tune on the CIFAR10 32x32 UNet at batch 128, gradient accumulation 1, three arms alternating inside every
     round: "unshaped", "unshaped_again" (the same configuration a second time: the run's own A/A spread) and "shaped" (gamma 5, poison weight 2,
     the split on).  The learning rate is 0 in every arm and the three arms train ONE network.  shaped / unshaped is reported beside the A/A
     ratio and the spreads over the rounds; "no measurable cost" is said only when it lies inside the A/A spread.
   python tools/loss_shape_ab.py [--rounds 3] [--steps 10] [--out profiles/r15_loss_shape_ab.json]
Information only: no gate.  Run it under a time limit of its own (`timeout -k 10 600 python tools/loss_shape_ab.py`)."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "r15_loss_shape_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    from villandiffusion_amd import ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import Trainer
    from villandiffusion_amd.unet import UNet2DModel

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    med = lambda x: sorted(x)[len(x) // 2]                      # noqa: E731
    spread = lambda x: max(x) - min(x)                          # noqa: E731
    gen = torch.Generator().manual_seed(0)

    # ---- (a) the kernel alone ----
    kern = {}
    for Bk, shape in ((128, (3, 32, 32)), (8, (3, 256, 256))):
        chw = shape[0] * shape[1] * shape[2]
        pred, y = torch.randn(Bk, chw, generator=gen).to(dev), torch.randn(Bk, chw, generator=gen).to(dev)
        dpred, loss = torch.empty_like(pred), torch.empty(1, device=dev)
        partial = torch.empty(1024, device=dev)
        seg, blocks, wsn = ops.loss_sample_plan(Bk, chw)
        ws, sl, st = torch.empty(wsn, device=dev), torch.empty(Bk, device=dev), torch.empty(4, device=dev)
        wtab = torch.rand(1000, generator=gen).to(dev)
        t = torch.randint(0, 1000, (Bk,), generator=gen).to(dev)
        flags = (torch.arange(Bk) % 10 == 0).to(dev)
        calls = {"vd_loss_fwd_bwd": lambda: ops.mse_fwd_bwd(pred, y, dpred, loss, partial),
                 "vd_loss_sample_fwd_bwd": lambda: ops.loss_sample_fwd_bwd(pred, y, dpred, loss, ws, wtab=wtab, t=t, flags=flags, poison_weight=2.0,
                                                                           sample_loss=sl, stats=st)}
        rec = {name: {"us": []} for name in calls}
        for _ in range(args.rounds):
            for name, f in calls.items():
                for _ in range(5):
                    f()
                rec[name]["us"].append(1e3 * timed(torch, f, args.kernel_iters))
        nbytes = 4.0 * 3 * Bk * chw
        for name, r in rec.items():
            r["us_median"], r["us_spread"] = med(r["us"]), spread(r["us"])
            r["GB_per_s"] = nbytes / (r["us_median"] * 1e-6) / 1e9
            print(f"[{Bk}, {shape}] {name}: {r['us_median']:.1f} us, {r['GB_per_s']:.0f} GB/s", flush=True)
        kern[f"{Bk}x{chw}"] = {"B": Bk, "chw": chw, "algorithmic_bytes": nbytes, "segments": seg, "blocks": blocks, **rec,
                               "sample_over_plain": rec["vd_loss_sample_fwd_bwd"]["us_median"] / rec["vd_loss_fwd_bwd"]["us_median"]}

    # ---- (b) the training step ----
    B = args.batch
    x0 = (torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).to(dev)
    poison = torch.arange(B) % 10 == 0
    R = (torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1)
    R[~poison] = 0
    eps = torch.randn(B, 3, 32, 32, generator=gen).to(dev)
    t = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    batch = {"target": x0, "pixel_values": R.to(dev), "is_clean": (~poison).to(dev)}
    net = UNet2DModel()
    net.reset_parameters(0)
    shaping = dict(snr_gamma=5.0, poison_weight=2.0, track_split=True)
    trs = {name: Trainer(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1, **kw), lr=0.0, total_steps=10 ** 6, warmup_steps=0)
           for name, kw in (("unshaped", {}), ("unshaped_again", {}), ("shaped", shaping))}
    fns = {k: (lambda tr=tr: tr.train_step(batch, t, noise=eps)) for k, tr in trs.items()}
    rows = {k: [] for k in trs}
    for rnd in range(args.rounds):
        for key, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(torch, fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    summary = {k + "_ms_median": med(v) for k, v in rows.items()} | {k + "_ms_spread": spread(v) for k, v in rows.items()}
    summary["shaped_over_unshaped"] = summary["shaped_ms_median"] / summary["unshaped_ms_median"]
    summary["aa_ratio"] = summary["unshaped_again_ms_median"] / summary["unshaped_ms_median"]
    both = rows["unshaped"] + rows["unshaped_again"]
    summary["aa_spread_rel"] = spread(both) / med(both)           # every unshaped round of both arms: the run's own noise
    summary["inside_aa_spread"] = abs(summary["shaped_over_unshaped"] - 1.0) <= summary["aa_spread_rel"]
    split = trs["shaped"].loss_fn.last_split.tolist()
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": net.flat_numel, "batch": B, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "kernel_iters": args.kernel_iters, "conv_math": net.conv_math, "shaping": shaping,
                      "device": torch.cuda.get_device_name(0)},
           "kernels": kern, "rounds": rows, "summary": summary, "last_split": split}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
