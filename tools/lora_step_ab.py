"""Interleaved timing on one box for one optimiser step of the fine-tune on config #2's network (CIFAR10 32x32 UNet, 35.7 M parameters) at
batch 128, gradient accumulation 1:
 * "full":   `Trainer(...)` -- every parameter trained (vd_l2norm_sq + vd_adam_step over the flat buffer);
 * "lora":   `Trainer(..., lora=LoRAConfig(r=4, target="all"))` -- vd_lora_grad, vd_l2norm_sq + vd_adam_step over the adapter, vd_lora_merge;
 * "torch":  the same LoRA step with the merge and the adapter gradient written as per-layer torch ops on the parameter views (one `addmm` per
   layer for the merge, two `mm` per layer for the gradient)
-- ms per step, alternating inside every round; the spread of each over the rounds is the same-box run-to-run spread the differences are to be
read against.  The learning rate is 0 in every arm: all kernels move the bytes they always move and every step sees the same weights.  The
three arms train ONE network (the same buffers and addresses), so they differ in the optimiser's part alone; that part is also timed by
itself, and the host's time to enqueue a step is recorded beside it ("parts").
Then the two kernels alone over the whole flat buffer, algorithmic bytes over time: vd_lora_merge (8 B per adapted weight float: w0 read, w
written), vd_lora_grad (8 B per adapted weight float: g is read twice, once by rows for B, once by columns for A), and beside them vd_neuron_scale
(8 B per selected float) on the same buffer in the same run.  The adapter itself (r rows of A per layer) is re-read from cache by every row and
is not counted.
   python tools/lora_step_ab.py [--rounds 3] [--steps 10] [--out profiles/r13_lora_ab.json]
Information only: no gate.  Run it under a time limit of its own (`timeout -k 10 600 python tools/lora_step_ab.py`)."""
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
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "r13_lora_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    from villandiffusion_amd import anp, ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.lora import LoRAAdapter, LoRAConfig
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import Trainer
    from villandiffusion_amd.unet import UNet2DModel

    class TorchAdapter(LoRAAdapter):
        """Arm "torch": the merge and the chain rule as per-layer torch ops on views of the flat buffers."""

        def _views(self):
            if not hasattr(self, "_v"):
                net, r, self._v = self.model, self.cfg.r, []
                for name, (a, b) in self.table.slices.items():
                    off, n, shape = net._offs[name]
                    M = shape[0]
                    self._v.append((self.base[off:off + n].view(M, -1), net.flat_param[off:off + n].view(M, -1), net.flat_grad[off:off + n].view(M, -1),
                                    self.param[a].view(r, -1), self.param[b].view(M, r), self.grad[a].view(r, -1), self.grad[b].view(M, r)))
            return self._v

        def merge_(self):
            s = self.table.s
            with torch.no_grad():
                for w0, w, _, A, B, _, _ in self._views():
                    torch.addmm(w0, B, A, alpha=s, out=w)
            self._weights_written()

        def backward_(self, accumulate=False):
            s = self.table.s
            with torch.no_grad():
                for _, _, G, A, B, gA, gB in self._views():
                    torch.mm(B.t(), G, out=gA)
                    torch.mm(G, A.t(), out=gB)
                    if s != 1.0:
                        gA.mul_(s)
                        gB.mul_(s)

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = LoRAConfig(r=args.rank, target="all")
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).to(dev)
    R = torch.zeros_like(x0)
    eps = torch.randn(B, 3, 32, 32, generator=gen).to(dev)
    t = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    batch = {"target": x0, "pixel_values": R}

    # ONE network for the three arms: the same weights, gradient buffer, workspaces and addresses, so that the arms differ in the optimiser's
    # part alone.  The adapters are built before the first merge (their base is the untouched network) and hold the same non-zero B.
    net = UNet2DModel()
    net.reset_parameters(0)

    def trainer(kind):
        tr = Trainer(net, LossFn(S.DDPMScheduler(), "SDE-VP", psi=1), lr=0.0, total_steps=10 ** 6, warmup_steps=0,
                     lora=None if kind == "full" else cfg)
        if kind == "torch":
            tr.adapter.__class__ = TorchAdapter
        return tr

    trs = {k + "_ms": trainer(k) for k in ("full", "lora", "torch")}
    for key in ("lora_ms", "torch_ms"):
        ad = trs[key].adapter
        gb = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for _, b in ad.table.slices.values():
                ad.param[b] = 0.01 * torch.randn(b.stop - b.start, generator=gb).to(dev)
        ad.merge_()                                        # (the "full" arm, at lr 0, trains on these merged weights too)
    fns = {k: (lambda tr=tr: tr.train_step(batch, t, noise=eps)) for k, tr in trs.items()}
    rows = {k: [] for k in trs}
    for rnd in range(args.rounds):
        for key, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(torch, fn, args.steps))
        print(f"round {rnd}: " + ", ".join(f"{key[:-3]} {v[-1]:.3f} ms" for key, v in rows.items()), flush=True)
    # the optimiser's part of the step alone (on whatever gradient the last step left; lr 0), and the host's time to enqueue a whole step
    import time
    parts = {}
    for key, tr in trs.items():
        f = lambda tr=tr: tr.opt.step(lr=0.0, grad_inv_scale=1.0)
        for _ in range(3):
            f()
        opt_ms = [timed(torch, f, 20) for _ in range(args.rounds)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fns[key]()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.steps          # no synchronise inside: the enqueue, as long as the queue does not fill
        torch.cuda.synchronize()
        parts[key[:-3]] = {"optimiser_alone_ms": sorted(opt_ms)[len(opt_ms) // 2], "host_enqueue_ms_per_step": host_ms}
    print("parts:", json.dumps(parts), flush=True)
    a, b = trs["lora_ms"].adapter, trs["torch_ms"].adapter
    agree = {"adapter_gradient_max_rel_diff": float((a.grad - b.grad).abs().max() / b.grad.abs().max())}
    kept = net.flat_param.clone()
    b.merge_()
    agree["merged_weights_max_abs_diff"] = float((net.flat_param - kept).abs().max())       # the torch arm's merge against the kernel's
    a.merge_()

    # ---- the kernels alone, on the LoRA arm's buffers ----
    tab = a.table
    ntab = anp.neuron_table(net, "all")
    mask = torch.ones(ntab.n_neurons, device=dev)
    kern = {"lora_merge": {"bytes": 8.0 * tab.weight_floats, "us": []},
            "lora_grad": {"bytes": 8.0 * tab.weight_floats, "us": []},
            "neuron_scale": {"bytes": 8.0 * (ntab.weight_floats + ntab.n_bias) + 4.0 * ntab.n_neurons, "us": []}}
    calls = {"lora_merge": lambda: ops.lora_merge(a.base, net.flat_param, tab, a.param),
             "lora_grad": lambda: ops.lora_grad(net.flat_grad, tab, a.param, a.grad),
             "neuron_scale": lambda: ops.neuron_scale(a.base, net.flat_param, ntab, mask)}
    for rnd in range(args.rounds):
        for name, f in calls.items():
            for _ in range(5):
                f()
            kern[name]["us"].append(1e3 * timed(torch, f, args.kernel_iters))
    a.unmerge_()
    med = lambda x: sorted(x)[len(x) // 2]
    for name, kk in kern.items():
        kk["us_median"] = med(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        kk["fraction_of_8TBps"] = kk["GB_per_s"] / 8000.0
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)
    spread = lambda x: max(x) - min(x)
    summary = {key + "_median": med(x) for key, x in rows.items()} | {key + "_spread": spread(x) for key, x in rows.items()}
    summary["lora_over_full"] = summary["lora_ms_median"] / summary["full_ms_median"]
    summary["lora_over_torch"] = summary["lora_ms_median"] / summary["torch_ms_median"]
    summary["merge_over_neuron_scale_rate"] = kern["lora_merge"]["GB_per_s"] / kern["neuron_scale"]["GB_per_s"]
    summary.update(agree)
    notes = []
    if summary["merge_over_neuron_scale_rate"] < 0.5:
        notes.append("vd_lora_merge runs below half of vd_neuron_scale's rate: beside the 8 B of w0 / w it issues r 16-byte loads of A per item "
                     "(one row of w re-reads the layer's whole A; they hit in cache but occupy the same load path), and r multiply-adds per float")
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": net.flat_numel, "batch": B, "rank": cfg.r, "target": cfg.target,
                      "jobs": tab.n_jobs, "adapted_weight_floats": tab.weight_floats, "adapter_floats": tab.adapter_floats,
                      "row_workgroups": tab.row_blocks, "column_workgroups": tab.col_blocks, "rounds": args.rounds, "steps": args.steps,
                      "warmup": args.warmup, "kernel_iters": args.kernel_iters, "conv_math": net.conv_math,
                      "device": torch.cuda.get_device_name(0)},
           "rounds": rows, "kernels": kern, "summary": summary, "parts": parts,
           "notes": notes}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
