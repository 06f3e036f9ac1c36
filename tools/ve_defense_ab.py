"""Interleaved timing on one box for the NCSN++ (SDE-VE) defences (villandiffusion_amd.defense_ve) on the default NCSN++ (61.9 M parameters, 32x32):
 * "dx": forward + the input-gradient pass of the frozen network, against "full": forward + the full backward (with the sample's gradient),
   ms per pass, alternating inside every alternation;
 * vd_pyramid_dgrad per level of the input-image pyramid against what it replaces -- one ops.gemm with M = 3 plus the ops.fir_resample2 launch
   that adds the coarser level's gradient -- in us, alternating, with the kernel's fraction of its HBM ceiling bytes(g) / 8 TB/s.  The kernel is
   kept only if it is not slower than the composed path in every alternation ("kernel_kept" per level and overall);
 * one VE inversion iteration and one VE removal step, ms (information only): the calls the library's own loops make per iteration
   (defense._noise_of, _objective_into and adam_update; mitigation._removal_step), not copies of them.
   python tools/ve_defense_ab.py [--alternations 3] [--batch 64] [--out profiles/r09_ve_defense_ab.json]
Run it under a time limit of its own (`timeout -k 10 900 python tools/ve_defense_ab.py`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alternations", type=int, default=3, help="A/B alternations (at least 3)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="timed passes per network measurement")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r09_ve_defense_ab.json"))
    args = ap.parse_args()
    assert args.alternations >= 3

    import torch
    from villandiffusion_amd import defense_ve, mitigation, ops
    from villandiffusion_amd import schedulers as S
    from villandiffusion_amd.defense import _frozen, _noise_of, _objective_into, adam_update
    from villandiffusion_amd.lib import A_COL, B_PLAIN
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.trainer import FusedAdam

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    torch.cuda.set_device(0)
    B = args.batch
    gen = torch.Generator(device="cuda").manual_seed(0)
    shape = (3, 32, 32)
    sched = S.ScoreSdeVeScheduler(sigma_max=380.0)
    _, sigma = defense_ve._sigma_at(sched, None, "ve_defense_ab")
    net = NCSNppModel()
    net.reset_parameters(0)
    x = torch.randn((B,) + shape, device="cuda", generator=gen) * sigma
    w = torch.randn((B,) + shape, device="cuda", generator=gen)
    sig = torch.full((B,), sigma, device="cuda")

    # ---- 1. forward + input-gradient pass of the frozen network against forward + full backward ----
    def full_pass():
        xc = x.clone().requires_grad_(True)
        with net.input_gradients():
            net(xc, sig)[0].backward(w)
        net.zero_grad()

    def dx_pass():
        xc = x.clone().requires_grad_(True)
        with _frozen(net), net.input_gradients():
            net(xc, sig)[0].backward(w)

    rows = {"dx_ms": [], "full_ms": []}
    for alt in range(args.alternations):
        for key, fn in (("dx_ms", dx_pass), ("full_ms", full_pass)):
            for _ in range(args.warmup):
                fn()
            rows[key].append(timed(fn, args.steps))
        print(f"alternation {alt}: fwd + dx pass {rows['dx_ms'][-1]:.2f} ms, fwd + full backward {rows['full_ms'][-1]:.2f} ms", flush=True)

    # ---- 2. vd_pyramid_dgrad per level against gemm (M = 3) + fir_resample2 ----
    levels = []
    for name, K, H, has_coarse in (("level 1: 128 ch, 16x16", 128, 16, True), ("level 2: 256 ch, 8x8", 256, 8, True), ("level 3: 256 ch, 4x4", 256, 4, False)):
        g = torch.randn((B, K, H, H), device="cuda", generator=gen)
        wk = torch.randn((K, 3), device="cuda", generator=gen) / K ** 0.5
        coarse = torch.randn((B, 3, H // 2, H // 2), device="cuda", generator=gen) if has_coarse else None
        out_k, out_c = torch.empty((B, 3, H, H), device="cuda"), torch.empty((B, 3, H, H), device="cuda")
        HW = H * H

        def kernel():
            ops.pyramid_dgrad(g, wk, out_k, coarse=coarse)

        def composed():
            ops.gemm(wk, g, out_c, M=3, N=B * HW, K=K, a_mode=A_COL, b_mode=B_PLAIN, NP=HW, lda=3, ldb=HW, b_bstride=K * HW, ldd=HW, d_bstride=3 * HW)
            if coarse is not None:
                ops.fir_resample2(coarse, out_c, up=True, scale=0.25, accumulate=True)

        kernel(), composed()
        torch.cuda.synchronize()
        err = float((out_k - out_c).abs().max() / out_c.abs().max())
        rec = {"level": name, "K": K, "H": H, "B": B, "bytes_g": 4.0 * g.numel(), "kernel_us": [], "composed_us": [], "max_rel_diff": err}
        for alt in range(args.alternations):
            for key, fn in (("kernel_us", kernel), ("composed_us", composed)):
                for _ in range(5):
                    fn()
                rec[key].append(1e3 * timed(fn, 50))
        med = sorted(rec["kernel_us"])[len(rec["kernel_us"]) // 2]
        rec["kernel_us_median"] = med
        rec["composed_us_median"] = sorted(rec["composed_us"])[len(rec["composed_us"]) // 2]
        rec["ceiling_us_at_8TBps"] = rec["bytes_g"] / 8e12 * 1e6
        rec["fraction_of_hbm_ceiling"] = rec["ceiling_us_at_8TBps"] / med
        rec["kernel_kept"] = all(k <= c for k, c in zip(rec["kernel_us"], rec["composed_us"]))
        levels.append(rec)
        print(f"{name}: kernel {rec['kernel_us']} us, gemm + fir {rec['composed_us']} us, {rec['fraction_of_hbm_ceiling']:.3f} of the HBM ceiling, "
              f"kept {rec['kernel_kept']}", flush=True)

    # ---- 3. one inversion iteration and one removal step (information only) ----
    Bi = min(B, 32)
    tau = torch.rand(shape, device="cuda", generator=gen)
    m, v, dtau = torch.zeros_like(tau), torch.zeros_like(tau), torch.empty_like(tau)
    loss, partial = torch.empty(1, device="cuda"), torch.empty(2048, device="cuda")
    eps = torch.empty((Bi,) + shape, device="cuda")
    sig_i = torch.full((Bi,), sigma, device="cuda")
    per_iter = (eps.numel() + 3) // 4
    it = [0]

    def inversion_iteration():                               # one iteration of defense._run_inversion; the caller's context is opened here
        it[0] += 1
        with _frozen(net), net.input_gradients():
            _objective_into(net, tau, _noise_of("ve_defense_ab", None, it[0] - 1, eps, 0, per_iter, "cuda"), sig_i, 0.5, loss, dtau, partial, sigma)
        adam_update(tau, dtau, m, v, it[0], 0.1)

    frozen = mitigation._frozen_copy(net)
    teacher = defense_ve._teacher(frozen)
    opt = FusedAdam(net, 1e-6, max_grad_norm=1.0)
    terms = torch.zeros(3, device="cuda")
    t2 = torch.full((2 * Bi,), sigma, device="cuda")
    tau_s = defense_ve._scaled(tau, sigma)

    def removal_step():                                      # one iteration of mitigation._run_removal as defense_ve.remove_backdoor calls it
        it[0] += 1
        eps_s = defense_ve._scaled(_noise_of("ve_defense_ab", None, it[0] - 1, eps, 0, per_iter, "cuda"), sigma)
        mitigation._removal_step(net, teacher, opt, tau_s, eps_s, t2, sigma * sigma, sigma * sigma, terms, partial)

    info = {}
    for key, fn in (("inversion_iteration_ms", inversion_iteration), ("removal_step_ms", removal_step)):
        for _ in range(args.warmup):
            fn()
        info[key] = [timed(fn, args.steps) for _ in range(args.alternations)]
        print(f"{key} (batch {Bi}): {info[key]}", flush=True)

    med = lambda vals: sorted(vals)[len(vals) // 2]
    summary = {"dx_ms_median": med(rows["dx_ms"]), "full_ms_median": med(rows["full_ms"]),
               "dx_over_full": med(rows["dx_ms"]) / med(rows["full_ms"]),
               "dx_not_slower_in_every_alternation": all(a <= b for a, b in zip(rows["dx_ms"], rows["full_ms"])),
               "pyramid_kernel_kept": all(r["kernel_kept"] for r in levels),
               "inversion_iteration_ms_median": med(info["inversion_iteration_ms"]), "removal_step_ms_median": med(info["removal_step_ms"])}
    out = {"config": {"model": "NCSNppModel default (61.9 M parameters, 32x32)", "batch": B, "defence_batch": Bi, "conv_math": net.conv_math,
                      "sigma": sigma, "alternations": args.alternations, "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0)},
           "passes": rows, "pyramid_levels": levels, "defence_steps": info, "summary": summary}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
