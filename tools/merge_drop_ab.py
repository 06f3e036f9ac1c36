"""Interleaved timing on one box for a DARE merge (villandiffusion_amd.merge with drop > 0) over the flat buffer of config #2 (CIFAR10 32x32 UNet,
35.7 M parameters) with K = 3 synthetic task vectors, DARE-linear at p = 0.9 (density 1, rescale on):
 * "kernel":    the one vd_merge_apply_drop launch (three Philox4x32-10 calls per item of four floats);
 * "torch_ops": the same merge as torch ops on the device -- per task a difference, a `torch.rand` mask, `where`, the rescale, the coefficient
   and an add, then the base -- with temporaries the size of the network.  Time only: the masks, and so the bits, differ by construction
   -- ms per merge, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the difference is to be
   read against;
 * the kernels alone, in the same run: vd_merge_apply_drop at p = 0.9 beside vd_merge_apply (K = 3, linear, the same buffers: the ratio is the
   price of the Philox calls) and beside itself with every drop_thr = 0 (no draw: what the rest of the new kernel costs); VD_DROP_COPY at K = 1
   (12 B/float) beside vd_curve_point (16 B/float); vd_randn over the same n (4 B/float written: the Philox rate, with Box-Muller on top).
Nothing is gated on these numbers.
   python tools/merge_drop_ab.py [--rounds 3] [--reps 20] [--out profiles/r22_merge_drop_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/merge_drop_ab.py`)."""
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
    ap.add_argument("--reps", type=int, default=20, help="merges timed per arm and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--drop", type=float, default=0.9)
    ap.add_argument("--out", default=os.path.join("profiles", "r22_merge_drop_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3 and 0.0 < args.drop < 1.0

    import torch
    from villandiffusion_amd import ops
    from villandiffusion_amd.merge import MergeConfig, coefficients, drop_threshold, rescale_of
    from villandiffusion_amd.unet import UNet2DModel

    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    n, K, lam, p, seed = net.flat_numel, 3, 1.0, args.drop, 2024
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = net.flat_param.detach().clone()
    shared = 0.01 * torch.randn(n, device="cuda", generator=gen)
    tasks = [base + shared + 0.005 * torch.randn(n, device="cuda", generator=gen) for _ in range(K)]
    del shared
    out_k, out_t = torch.empty_like(base), torch.empty_like(base)
    thr = torch.zeros(K, device="cuda")
    lams = coefficients(MergeConfig(method="linear", lam=lam), K)
    T, rs = [drop_threshold(p)] * K, [rescale_of(p)] * K
    partial = torch.empty(ops.MERGE_DROP_PARTIAL, device="cuda", dtype=torch.int32)
    stats, stats_old = torch.zeros(3 * K + 2, device="cuda", dtype=torch.int64), torch.zeros(2 * K + 2, device="cuda", dtype=torch.int64)
    zero = torch.zeros((), device="cuda")

    def kernel():
        ops.merge_apply_drop(out_k, base, tasks, lams, thr, "linear", lam, T, rs, list(range(K)), seed, partial, stats, weights=False)

    def torch_ops():
        acc = torch.zeros_like(base)
        for i in range(K):
            d = tasks[i] - base
            keep = torch.rand(n, device="cuda", generator=gen) >= p
            acc = acc + lams[i] * torch.where(keep, d * rs[i], zero)
        torch.add(base, acc, out=out_t)

    arms = {"kernel_ms": kernel, "torch_ops_ms": torch_ops}
    rows = {key: [] for key in arms}
    for rnd in range(args.rounds):
        for key, fn in arms.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.reps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    torch.cuda.synchronize()
    st = [int(v) for v in stats.cpu()]
    del out_t
    torch.cuda.empty_cache()

    # ---- the kernels alone, over the whole flat buffer ----
    noise = torch.empty_like(base)
    kern = {"merge_apply_drop_linear_K3": (4.0 * (K + 2) * n, kernel),
            "merge_apply_drop_linear_K3_no_draw": (4.0 * (K + 2) * n, lambda: ops.merge_apply_drop(
                out_k, base, tasks, lams, thr, "linear", lam, [0] * K, rs, list(range(K)), seed, partial, stats, weights=False)),
            "merge_apply_drop_ties_K3": (4.0 * (K + 2) * n, lambda: ops.merge_apply_drop(
                out_k, base, tasks, None, thr, "ties", lam, T, rs, list(range(K)), seed, partial, stats, weights=False)),
            "merge_apply_linear_K3": (4.0 * (K + 2) * n, lambda: ops.merge_apply(out_k, base, tasks, lams, thr, "linear", lam, partial, stats_old,
                                                                                  weights=False)),
            "merge_copy_K1": (12.0 * n, lambda: ops.merge_apply_drop(out_k, base, tasks[:1], None, None, "linear", 0.0, [drop_threshold(0.7)], None, [0],
                                                                     seed, partial, stats, copy=True, weights=False)),
            "curve_point": (16.0 * n, lambda: ops.curve_point(out_k, tasks[0], tasks[1], tasks[2], 0.25, 0.5, 0.25, weights=False)),
            "randn": (4.0 * n, lambda: ops.randn(noise, seed, 0))}
    kernels_alone = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(3):
                f()
            kernels_alone[name]["us"].append(1e3 * timed(f, 5 * max(1, args.reps)))
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kernels_alone.items():
        kk["us_median"] = med(kk["us"])
        kk["us_spread"] = max(kk["us"]) - min(kk["us"])
        kk["TB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e12
        print(f"{name}: {kk['us_median']:.1f} us (spread {kk['us_spread']:.1f}), {kk['bytes'] / 1e6:.1f} MB, {kk['TB_per_s']:.3f} TB/s", flush=True)

    us = lambda name: kernels_alone[name]["us_median"]
    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    summary["torch_ops_over_kernel"] = summary["torch_ops_ms_median"] / summary["kernel_ms_median"]
    summary["drop_over_apply_time"] = us("merge_apply_drop_linear_K3") / us("merge_apply_linear_K3")
    summary["no_draw_over_apply_time"] = us("merge_apply_drop_linear_K3_no_draw") / us("merge_apply_linear_K3")
    summary["copy_over_curve_point_rate"] = kernels_alone["merge_copy_K1"]["TB_per_s"] / kernels_alone["curve_point"]["TB_per_s"]
    summary["philox_calls_per_us_in_drop"] = K * ((n + 3) // 4) / us("merge_apply_drop_linear_K3")
    summary["philox_calls_per_us_in_randn"] = ((n + 3) // 4) / us("randn")
    res = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "K": K, "method": "linear", "density": 1.0, "drop": p, "seed": seed,
                      "drop_threshold": T[0], "rescale": rs[0], "lam": lam, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0)},
           "merge": {"drawn": st[:K], "kept": st[K:2 * K], "won": st[2 * K:3 * K], "support": st[3 * K], "conflict": st[3 * K + 1]},
           "rounds": rows, "kernels": kernels_alone, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
