"""Interleaved timing on one box for a checkpoint merge (villandiffusion_amd.merge) over the flat buffer of config #2 (CIFAR10 32x32 UNet, 35.7 M
parameters) with K = 3 synthetic task vectors (a shared dense part plus private parts), TIES at density 0.2:
 * "kernels":   the three selections (vd_merge_select, four passes of 8 bits each) and the one vd_merge_apply launch;
 * "torch_ops": the same merge as torch ops on the device -- `kthvalue` over |task - base| per task, `where`, explicit sequential adds, the sign
   election and a division -- with a dozen temporaries the size of the network
   -- ms per merge, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the difference is to be
   read against.  Whether the two give the same bits is recorded ("bit_equal": expected, not required);
 * the kernels alone: one vd_merge_select (all four passes; us and GB/s against 8 B/float per pass) and vd_merge_apply in both modes
   (4 (K + 2) B/float), beside vd_curve_point (16 B/float) and vd_l2norm_sq (4 B/float) in the same run.
Nothing is gated on these numbers.
   python tools/merge_ab.py [--rounds 3] [--reps 5] [--out profiles/r21_merge_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/merge_ab.py`)."""
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
    ap.add_argument("--reps", type=int, default=5, help="merges timed per arm and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join("profiles", "r21_merge_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    from villandiffusion_amd import ops
    from villandiffusion_amd.merge import rank_of
    from villandiffusion_amd.unet import UNet2DModel

    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    n, K, lam = net.flat_numel, 3, 0.7
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = net.flat_param.detach().clone()
    shared = 0.01 * torch.randn(n, device="cuda", generator=gen)
    tasks = [base + shared + 0.005 * torch.randn(n, device="cuda", generator=gen) for _ in range(K)]
    del shared
    k = rank_of(args.density, n)
    out_k, out_t = torch.empty_like(base), torch.empty_like(base)
    ws = torch.empty(ops.merge_plan(n)[3], device="cuda", dtype=torch.uint8)
    thr, rec = torch.zeros(K, device="cuda"), torch.zeros((K, 3), device="cuda", dtype=torch.int64)
    partial, stats = torch.empty(ops.MERGE_PARTIAL, device="cuda", dtype=torch.int32), torch.zeros(2 * K + 2, device="cuda", dtype=torch.int64)

    def kernels():
        for i in range(K):
            ops.merge_select(tasks[i], base, k, ws, thr[i:i + 1], rec[i])
        ops.merge_apply(out_k, base, tasks, None, thr, "ties", lam, partial, stats, weights=False)

    def torch_ops():
        ts = []
        for i in range(K):
            d = tasks[i] - base
            a = d.abs()
            t = a.kthvalue(n - k + 1).values                                  # the k-th largest
            ts.append(torch.where(a >= t, d, torch.zeros((), device="cuda")))
        s = torch.zeros_like(base)
        for t in ts:
            s = s + t
        plus = s >= 0
        m, c = torch.zeros_like(base), torch.zeros_like(base)
        for t in ts:
            on = (t != 0) & ((t > 0) == plus)
            m = torch.where(on, m + t, m)
            c = c + on
        tau = torch.where(c > 0, m / c, torch.zeros((), device="cuda"))
        torch.add(base, lam * tau, out=out_t)

    arms = {"kernels_ms": kernels, "torch_ops_ms": torch_ops}
    rows = {key: [] for key in arms}
    for rnd in range(args.rounds):
        for key, fn in arms.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.reps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    torch.cuda.synchronize()
    bit_equal = bool(torch.equal(out_k.view(torch.int32), out_t.view(torch.int32)))
    differing = int((out_k.view(torch.int32) != out_t.view(torch.int32)).sum())
    rec_host = rec.cpu()
    st = [int(v) for v in stats.cpu()]
    del out_t
    torch.cuda.empty_cache()

    # ---- the kernels alone, over the whole flat buffer ----
    p1024, nsq = torch.empty(3 * 1024, device="cuda"), torch.ones(1, device="cuda")
    lams = [lam / K] * K
    kern = {"merge_select_4_passes": (32.0 * n, lambda: ops.merge_select(tasks[0], base, k, ws, thr[0:1], rec[0])),
            "merge_select_k0_1_pass": (8.0 * n, lambda: ops.merge_select(tasks[0], base, 0, ws, nsq, rec[0])),
            "merge_apply_ties_K3": (4.0 * (K + 2) * n, lambda: ops.merge_apply(out_k, base, tasks, None, thr, "ties", lam, partial, stats, weights=False)),
            "merge_apply_linear_K3": (4.0 * (K + 2) * n, lambda: ops.merge_apply(out_k, base, tasks, lams, thr, "linear", lam, partial, stats, weights=False)),
            "curve_point": (16.0 * n, lambda: ops.curve_point(out_k, tasks[0], tasks[1], tasks[2], 0.25, 0.5, 0.25, weights=False)),
            "l2norm_sq": (4.0 * n, lambda: ops.l2norm_sq(base, p1024, nsq))}
    kernels_alone = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(2):
                f()
            kernels_alone[name]["us"].append(1e3 * timed(f, 4 * max(1, args.reps)))
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kernels_alone.items():
        kk["us_median"] = med(kk["us"])
        kk["TB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e12
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['TB_per_s']:.3f} TB/s", flush=True)

    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    summary["torch_ops_over_kernels"] = summary["torch_ops_ms_median"] / summary["kernels_ms_median"]
    summary["bit_equal"] = bit_equal
    summary["differing_floats"] = differing
    summary["select_pass_TB_per_s"] = kernels_alone["merge_select_4_passes"]["TB_per_s"]
    summary["select_over_l2norm_rate"] = kernels_alone["merge_select_4_passes"]["TB_per_s"] / kernels_alone["l2norm_sq"]["TB_per_s"]
    summary["apply_over_curve_point_rate"] = kernels_alone["merge_apply_ties_K3"]["TB_per_s"] / kernels_alone["curve_point"]["TB_per_s"]
    res = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": n, "K": K, "method": "ties", "density": args.density, "k": k, "lam": lam,
                      "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
           "merge": {"n_gt": [int(v) for v in rec_host[:, 0]], "n_eq": [int(v) for v in rec_host[:, 1]], "kept": st[:K], "won": st[K:2 * K],
                     "support": st[2 * K], "conflict": st[2 * K + 1]},
           "rounds": rows, "kernels": kernels_alone, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
