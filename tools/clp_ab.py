"""Interleaved timing on one box for the channel Lipschitz scores of clp.channel_lipschitz, over the "conv" Lipschitz table of config #2's
network (CIFAR10 32x32 UNet), one network shared by the arms:
 * "launch":     the one vd_channel_lipschitz launch over the table (table and scale vector resident: what the defence runs once);
 * "call":       clp.channel_lipschitz itself: the table upload, the scale vector, the launch and the one read of the result;
 * "torch":      per layer on the device, reshape to [rows, Cin, T] and torch.linalg.matrix_norm(ord=2), times |gamma| (what the launch
                 replaces).  Where this torch build has no batched solver on the device the arm is torch.bmm for the Gram on the device plus
                 numpy's eigvalsh on the host, and the record says so ("torch_arm");
   -- ms per pass, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are
   to be read against;
 * the kernel alone in bytes per second of its one read against the 8 TB/s HBM peak, with vd_neuron_grad over the same rows in the same run
   beside it as the bandwidth yardstick (two reads of every row).
   python tools/clp_ab.py [--rounds 3] [--steps 10] [--out profiles/r19_clp_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/clp_ab.py`)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from villandiffusion_amd import anp, clp, ops  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

HBM_PEAK = 8.0e12


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
    ap.add_argument("--layers", default="conv", choices=clp.LAYERS)
    ap.add_argument("--out", default=os.path.join("profiles", "r19_clp_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    tab = clp.lipschitz_table(net, args.layers)
    w = net.flat_param.detach()
    host_table, dev_table = tab.host_table(), tab.device_table(w.device)
    scale = clp._gamma(net, tab, w.device)
    out = torch.empty(tab.n_neurons, device="cuda")
    ref_out = torch.empty(tab.n_neurons, device="cuda")

    def launch():
        ops.channel_lipschitz(w, host_table, out, scale=scale, table=dev_table)

    def call():
        clp.channel_lipschitz(net, layers=args.layers, scale="gamma")

    def torch_svd():
        with torch.no_grad():
            for name, sl in tab.slices.items():
                p = net.P[name]
                ref_out[sl] = torch.linalg.matrix_norm(p.reshape(p.shape[0], p.shape[1], -1), ord=2)
            ref_out.mul_(scale.abs())

    def torch_gram_host_eig():
        with torch.no_grad():
            grams = []
            for name in tab.slices:
                p = net.P[name]
                a = p.reshape(p.shape[0], p.shape[1], -1)
                grams.append(torch.bmm(a.transpose(1, 2), a).cpu().numpy())
            lam = np.concatenate([np.linalg.eigvalsh(G)[:, -1] for G in grams])
            ref_out.copy_(torch.from_numpy(np.sqrt(np.maximum(lam, 0.0))).to("cuda"))
            ref_out.mul_(scale.abs())

    torch_arm, torch_fn, why = "torch.linalg.matrix_norm(ord=2) per layer on the device", torch_svd, None
    t0 = time.time()
    try:
        torch_svd()
        torch.cuda.synchronize()
    except RuntimeError as e:                              # no batched solver on the device in this torch build
        torch_arm, torch_fn, why = "torch.bmm Gram per layer on the device + numpy eigvalsh on the host", torch_gram_host_eig, str(e)[:200]
        t0 = time.time()
        torch_gram_host_eig()
        torch.cuda.synchronize()
    once = time.time() - t0
    torch_steps = max(1, min(args.steps, int(5.0 / max(once, 1e-3))))         # a slow solver gets fewer passes per round, never fewer rounds
    print(f"torch arm: {torch_arm}; first pass {once * 1e3:.1f} ms, {torch_steps} passes per round", flush=True)

    arms = {"launch_ms": (launch, args.steps, args.warmup), "call_ms": (call, args.steps, args.warmup), "torch_ms": (torch_fn, torch_steps, 1)}
    rows = {key: [] for key in arms}
    for rnd in range(args.rounds):
        for key, (fn, n, warm) in arms.items():
            for _ in range(warm):
                fn()
            rows[key].append(timed(fn, n))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    launch()
    torch.cuda.synchronize()
    agree = float(((out - ref_out).abs() / ref_out).max())

    # ---- the kernels alone ----
    ntab = anp.neuron_table(net, args.layers if args.layers != "resnet" else "conv")
    g = torch.randn_like(w)
    w0 = w.clone()
    gmask = torch.empty(ntab.n_neurons, device="cuda")
    kern = {"channel_lipschitz": (4.0 * tab.weight_floats + 8.0 * tab.n_neurons, launch),
            "channel_lipschitz_no_scale": (4.0 * tab.weight_floats + 4.0 * tab.n_neurons,
                                           lambda: ops.channel_lipschitz(w, host_table, out, table=dev_table)),
            "neuron_grad": (8.0 * (ntab.weight_floats + ntab.n_bias) + 4.0 * ntab.n_neurons, lambda: ops.neuron_grad(g, w0, ntab, gmask))}
    kernels = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(2):
                f()
            kernels[name]["us"].append(1e3 * timed(f, 2 * max(1, args.steps)))
    med = lambda v: sorted(v)[len(v) // 2]
    for name, kk in kernels.items():
        kk["us_median"] = med(kk["us"])
        kk["us_spread"] = max(kk["us"]) - min(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        kk["fraction_of_hbm_peak"] = kk["GB_per_s"] * 1e9 / HBM_PEAK
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)

    spread = lambda v: max(v) - min(v)
    summary = {key + "_median": med(v) for key, v in rows.items()} | {key + "_spread": spread(v) for key, v in rows.items()}
    summary["torch_over_launch"] = summary["torch_ms_median"] / summary["launch_ms_median"]
    summary["arms_agree_max_rel"] = agree
    res = {"config": {"model": "UNet2DModel CIFAR10 32x32", "layers": args.layers, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
                      "torch_arm": torch_arm, "torch_arm_fallback_reason": why, "torch_steps": torch_steps, "jobs": tab.n_jobs,
                      "rows": tab.n_neurons, "rows_of_nine_taps": sum(j[1] for j in tab.jobs if j[3] == 9), "weight_floats": tab.weight_floats,
                      "neuron_grad_rows": ntab.n_neurons, "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kernels, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
