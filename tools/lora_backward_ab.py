"""Interleaved timing on one box of one optimiser step of the fine-tune on config #2's network (CIFAR10 32x32 UNet) at batch 128, rank 4:
 * "finetune":        `Trainer(...)` -- every parameter trained;
 * "full_<target>":   `Trainer(..., lora=LoRAConfig(r, target), lora_backward="full")` -- the backward forms every weight gradient;
 * "adapted_<target>": the same with lora_backward="adapted" -- only the gradients the adapter needs (lora.BackwardRoute),
for target attn, conv and all -- ms per step, alternating inside every round, medians over the rounds; the spread of each over the rounds is
the same-box run-to-run spread the differences are to be read against.  The learning rate is 0 in every arm and all arms train ONE network (the
same buffers and addresses; the network's `lora_route` is switched per arm), so every step sees the same weights.
Then vd_lora_act_grad alone over the attn table of that network (synthetic activations of the real shapes), algorithmic bytes (x and dy once
per job) over time, beside vd_lora_grad over the same table's weight gradients in the same run.
   python tools/lora_backward_ab.py [--rounds 3] [--steps 10] [--out profiles/r14_lora_backward_ab.json]
Information only: no gate.  Boxes differ by a few per cent: quote ratios of one run only.  Run it under a time limit of its own
(`timeout -k 10 600 python tools/lora_backward_ab.py`)."""
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
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "r14_lora_backward_ab.json"))
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    from villandiffusion_amd import ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.lora import TARGETS, LoRAConfig
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.trainer import Trainer
    from villandiffusion_amd.unet import UNet2DModel

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).to(dev)
    R = torch.zeros_like(x0)
    eps = torch.randn(B, 3, 32, 32, generator=gen).to(dev)
    t = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    batch = {"target": x0, "pixel_values": R}
    net = UNet2DModel()
    net.reset_parameters(0)

    def trainer(kind):
        lf = LossFn(S.DDPMScheduler(), "SDE-VP", psi=1)
        if kind == "finetune":
            return Trainer(net, lf, lr=0.0, total_steps=10 ** 6, warmup_steps=0)
        mode, target = kind.split("_")
        tr = Trainer(net, lf, lr=0.0, total_steps=10 ** 6, warmup_steps=0, lora=LoRAConfig(r=args.rank, target=target), lora_backward=mode)
        net.lora_route = None                                # (every adapter is built on the untouched network; the route is set per step)
        return tr

    kinds = ["finetune"] + [f"{m}_{tg}" for tg in TARGETS for m in ("full", "adapted")]
    trs = {k: trainer(k) for k in kinds}
    for k, tr in trs.items():
        if tr.adapter is not None:
            gb = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for _, b in tr.adapter.table.slices.values():
                    tr.adapter.param[b] = 0.01 * torch.randn(b.stop - b.start, generator=gb).to(dev)

    def step(k):
        tr = trs[k]
        net.lora_route = tr.adapter.route if tr.adapter is not None else None
        tr.train_step(batch, t, noise=eps)

    rows = {k: [] for k in kinds}
    for rnd in range(args.rounds):
        for k in kinds:
            if trs[k].adapter is not None:
                trs[k].adapter.merge_()                      # this arm's weights (lr 0: they stay)
            for _ in range(args.warmup):
                step(k)
            rows[k].append(timed(torch, lambda k=k: step(k), args.steps))
        print(f"round {rnd}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in rows.items()), flush=True)
    net.lora_route = None
    med = lambda x: sorted(x)[len(x) // 2]
    spread = lambda x: max(x) - min(x)
    summary = {k + "_ms_median": med(v) for k, v in rows.items()} | {k + "_ms_spread": spread(v) for k, v in rows.items()}
    for tg in TARGETS:
        summary[f"adapted_over_full_{tg}"] = summary[f"adapted_{tg}_ms_median"] / summary[f"full_{tg}_ms_median"]
        summary[f"full_{tg}_over_finetune"] = summary[f"full_{tg}_ms_median"] / summary["finetune_ms_median"]
    agree = {}
    for tg in TARGETS:                                       # the two modes' adapter gradients after their last step's backward (lr 0: the same weights)
        a, f = trs[f"adapted_{tg}"], trs[f"full_{tg}"]
        for tr in (a, f):
            tr.adapter.merge_()
            net.lora_route = tr.adapter.route
            net.zero_grad()
            tr.adapter.zero_grad()
            loss = tr.loss_fn.p_loss_by_keys(batch, net, target_latent_key="target", poison_latent_key="pixel_values", timesteps=t, noise=eps)
            loss.backward()
            tr.adapter.backward_()
        net.lora_route = None
        agree[f"adapter_gradient_max_rel_diff_{tg}"] = float((a.adapter.grad - f.adapter.grad).abs().max() / f.adapter.grad.abs().max())
    net.zero_grad()
    summary.update(agree)

    # ---- the direct kernel alone over the attn table, on synthetic activations of the real shapes ----
    ad = trs["adapted_attn"].adapter
    tab = ad.table
    by_name = dict(zip(tab.slices, tab.jobs))
    levels = {}                                              # attention prefix -> pixels
    S0 = net.sample_size
    for i, blk in enumerate(net.down):
        for a in blk["attn"]:
            levels[a.prefix] = (S0 >> i) ** 2
    levels[net.mid_attn.prefix] = (S0 >> (len(net.down) - 1)) ** 2
    for i, blk in enumerate(net.up):
        for a in blk["attn"]:
            levels[a.prefix] = (S0 >> (len(net.down) - 1 - i)) ** 2
    jobs, keep = [], []
    for prefix, N in levels.items():
        ch = by_name[prefix + ".to_q.weight"][1]
        gx, dqkv, o, dout = (torch.randn(B, c, N, device=dev) for c in (ch, 3 * ch, ch, ch))
        keep += [gx, dqkv, o, dout]
        for i, n in enumerate(("to_q", "to_k", "to_v")):
            _, M, L, aoff, boff, _, _ = by_name[f"{prefix}.{n}.weight"]
            jobs.append((dqkv.data_ptr() + 4 * i * ch * N, 3 * ch * N, gx.data_ptr(), ch * N, B, M, L, N, aoff, boff))
        _, M, L, aoff, boff, _, _ = by_name[prefix + ".to_out.0.weight"]
        jobs.append((dout.data_ptr(), ch * N, o.data_ptr(), ch * N, B, M, L, N, aoff, boff))
    plan = ops.lora_act_plan(jobs, tab.r)
    ws = torch.empty(plan.ws_floats, device=dev)
    scratch = torch.zeros_like(ad.grad)
    kern = {"lora_act_grad": {"bytes": plan.nbytes, "us": [], "jobs": len(jobs), "table_rows": plan.n_rows, "workgroups": plan.workgroups},
            "lora_grad": {"bytes": 8.0 * tab.weight_floats, "us": [], "jobs": tab.n_jobs}}
    calls = {"lora_act_grad": lambda: ops.lora_act_grad(plan, ad.param, scratch, tab.s, ws),
             "lora_grad": lambda: ops.lora_grad(net.flat_grad, tab, ad.param, scratch)}
    for rnd in range(args.rounds):
        for name, f in calls.items():
            for _ in range(3):
                f()
            kern[name]["us"].append(1e3 * timed(torch, f, args.kernel_iters))
    for name, kk in kern.items():
        kk["us_median"] = med(kk["us"])
        kk["GB_per_s"] = kk["bytes"] / (kk["us_median"] * 1e-6) / 1e9
        kk["fraction_of_8TBps"] = kk["GB_per_s"] / 8000.0
        print(f"{name}: {kk['us_median']:.1f} us, {kk['bytes'] / 1e6:.1f} MB, {kk['GB_per_s']:.0f} GB/s", flush=True)
    for tr in trs.values():
        if tr.adapter is not None:
            tr.adapter.unmerge_()
    out = {"config": {"model": "UNet2DModel CIFAR10 32x32", "parameters": net.flat_numel, "batch": B, "rank": args.rank, "rounds": args.rounds,
                      "steps": args.steps, "warmup": args.warmup, "kernel_iters": args.kernel_iters, "conv_math": net.conv_math,
                      "device": torch.cuda.get_device_name(0),
                      "routes": {tg: {"direct": len(trs[f"adapted_{tg}"].adapter.route.direct), "full": len(trs[f"adapted_{tg}"].adapter.route.full_offs),
                                      "temb": trs[f"adapted_{tg}"].adapter.route.temb} for tg in TARGETS}},
           "rounds": rows, "kernels": kern, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
