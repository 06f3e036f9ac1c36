"""Interleaved timing on one box for the activation statistics of actprune.channel_stats, on config #2 (CIFAR10 32x32 UNet, batch 128), one
network shared by the arms:
 * "forward":   the no-grad save=True forward alone (what the statistics ride on);
 * "stats":     that forward plus the job table and the one vd_channel_stats launch over its tape (what channel_stats runs per batch);
 * "torch_ops": that forward plus, per ResnetBlock, torch's group_norm, silu, mean and mean of squares on the saved h1 (what the launch
                replaces)
   -- ms per pass, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are
   to be read against;
 * vd_channel_stats alone over the tape of one forward (both activations), bytes per second of its one read against the 8 TB/s HBM peak, and
   vd_neuron_keep_rows beside vd_neuron_scale over the same neuron table with a mask that drops every tenth row.
   python tools/actprune_ab.py [--rounds 3] [--steps 10] [--out profiles/r17_actprune_ab.json]
Run it under a time limit of its own (`timeout -k 10 600 python tools/actprune_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from villandiffusion_amd import actprune, anp, ops  # noqa: E402
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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join("profiles", "r17_actprune_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    net = UNet2DModel()
    net.reset_parameters(0)
    B = args.batch
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=gen)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=gen).float()
    tab = actprune.activation_table(net)
    out = torch.zeros((tab.n_channels, 2), device="cuda")
    ref_out = torch.zeros((tab.n_channels, 2), device="cuda")

    def forward():
        with torch.no_grad():
            return net._run_forward(x, t, save=True)[1]

    def stats():
        st = forward()
        ops.channel_stats(actprune._taps(net, st, tab, "silu_gn"), out, "silu_gn", keep=[])

    def torch_ops():
        st = forward()
        with torch.no_grad():
            for name, tp in zip(tab.names, actprune._taps(net, st, tab, "silu_gn")):
                h1, _, _, gamma, beta, G, c0 = tp
                a = F.silu(F.group_norm(h1, G, gamma, beta, net.eps))
                ref_out[c0:c0 + a.shape[1], 0] = a.mean(dim=(0, 2, 3))
                ref_out[c0:c0 + a.shape[1], 1] = (a * a).mean(dim=(0, 2, 3))

    arms = {"forward_ms": forward, "stats_ms": stats, "torch_ops_ms": torch_ops}
    rows = {key: [] for key in arms}
    for rnd in range(args.rounds):
        for key, fn in arms.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    # the two arms computed the same thing
    n_per = torch.cat([torch.full((tab.slices[nm].stop - tab.slices[nm].start,), float(tp[0].numel() // tp[0].shape[1]))
                       for nm, tp in zip(tab.names, actprune._taps(net, forward(), tab, "raw"))]).cuda()
    agree = float(((out / n_per[:, None]) - ref_out).abs().max() / ref_out.abs().max())

    # ---- the kernels alone ----
    st = forward()                                         # one tape, kept alive: the launches below read it again and again
    taps = {act: actprune._taps(net, st, tab, act) for act in ("silu_gn", "raw")}
    x_bytes = 4.0 * sum(tp[0].numel() for tp in taps["raw"])
    keep_alive = []
    full = anp.neuron_table(net, "all")
    w0 = net.flat_param.detach().clone()
    w = torch.empty_like(w0)
    mask = torch.ones(full.n_neurons, device="cuda")
    mask[::10] = 0.0
    dropped_bytes = 4.0 * sum(ln * int((mask[n0:n0 + rows_] == 0).sum()) for _, rows_, ln, _, n0, _ in full.jobs)
    kern = {"channel_stats_silu_gn": (x_bytes + 8.0 * tab.n_channels, lambda: ops.channel_stats(taps["silu_gn"], out, "silu_gn", keep=keep_alive)),
            "channel_stats_raw": (x_bytes + 8.0 * tab.n_channels, lambda: ops.channel_stats(taps["raw"], out, "raw", keep=keep_alive)),
            "neuron_keep_rows": (dropped_bytes + 4.0 * full.n_neurons, lambda: ops.neuron_keep_rows(w, full, mask)),
            "neuron_scale": (8.0 * (full.weight_floats + full.n_bias) + 4.0 * full.n_neurons, lambda: ops.neuron_scale(w0, w, full, mask))}
    kernels = {name: {"bytes": b, "us": []} for name, (b, _) in kern.items()}
    for rnd in range(args.rounds):
        for name, (_, f) in kern.items():
            for _ in range(2):
                f()
            kernels[name]["us"].append(1e3 * timed(f, 2 * max(1, args.steps)))
            del keep_alive[:]
    med = lambda v: sorted(v)[len(v) // 2]
    for name, kk in kernels.items():
        kk["us_median"] = med(kk["us"])
        kk["us_spread"] = max(kk["us"]) - min(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        kk["fraction_of_hbm_peak"] = kk["GB_per_s"] * 1e9 / HBM_PEAK
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)

    spread = lambda v: max(v) - min(v)
    summary = {key + "_median": med(v) for key, v in rows.items()} | {key + "_spread": spread(v) for key, v in rows.items()}
    summary["stats_minus_forward_ms"] = summary["stats_ms_median"] - summary["forward_ms_median"]
    summary["torch_ops_minus_forward_ms"] = summary["torch_ops_ms_median"] - summary["forward_ms_median"]
    summary["arms_agree_max_rel"] = agree
    res = {"config": {"model": "UNet2DModel CIFAR10 32x32", "batch": B, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
                      "layers": len(tab.names), "channels": tab.n_channels, "tapped_bytes": x_bytes, "neurons": full.n_neurons,
                      "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kernels, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
