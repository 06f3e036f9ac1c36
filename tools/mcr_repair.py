"""Mode Connectivity Repair of a diffusers-format checkpoint (villandiffusion_amd.curve; Zhao et al. 2020):
   python tools/mcr_repair.py --ckpt-a A --ckpt-b B --dataset CIFAR10 --n-clean 512 --steps 200 --batch 64 --t 0.3 --out FIXED
                              [--kind bezier|polychain] [--lr 2e-4] [--seed 0] [--scan 11] [--trigger FILE --target NAME]
takes two checkpoints of one architecture (two backdoored models, or a backdoored model and its fine-tuned copy), trains the bend of a curve
between their weights on the first --n-clean clean images of --dataset (no poisoning, no flips; SYNTHETIC-CIFAR10 needs no files) for --steps
optimiser steps of --batch images, and writes
   FIXED/            the checkpoint of A with the weights of the curve's point at --t,
   FIXED/curve.pt    the bend (with the layout digest and the endpoints' fingerprints it belongs to),
   FIXED/mcr.json    family, kind, steps, t, the curve's geometry before and after training, the last losses and "scan".
--scan N evaluates the clean loss at N points spread evenly over [0, 1] (both ends included) on the same images, to choose --t by; with
--trigger FILE (a [C, H, W] tensor, a known trigger or the one tools/invert_trigger.py writes) and --target NAME (a backdoor target of
villandiffusion_amd.dataset) every point also gets the poisoned loss.
   python tools/mcr_repair.py --curve FIXED/curve.pt --ckpt-a A --ckpt-b B --t 0.4 --out FIXED2
cuts another point of a trained curve without training (the endpoints are not stored in curve.pt: the same two checkpoints are given again
and their fingerprints checked).

A directory with a vqvae/ folder is latent diffusion (family "ldm"): the dataset is loaded at the VQ-VAE's pixel size and encoded first, the curve
is the latent UNet's.  An NCSNppModel with a ScoreSdeVeScheduler (family "ve") uses the SDE-VE loss on images in [0, 1].  Both checkpoints must
be of one family and one parameter layout.  The networks use GroupNorm, so there are no BatchNorm statistics to re-estimate at the chosen t."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt-a", required=True, help="diffusers-format checkpoint directory of the endpoint t = 0 (unet/, scheduler/)")
    ap.add_argument("--ckpt-b", required=True, help="the endpoint t = 1: the same family and parameter layout")
    ap.add_argument("--curve", default=None, help="a curve.pt of these two endpoints: cut --t from it, train nothing")
    ap.add_argument("--dataset", default=None, help="where the clean images come from (villandiffusion_amd.dataset.DatasetLoader names)")
    ap.add_argument("--dataset-root", default="datasets", help="dataset root directory")
    ap.add_argument("--n-clean", type=int, default=512, help="clean images used (the first of the dataset)")
    ap.add_argument("--steps", type=int, default=200, help="optimiser steps")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--t", type=float, required=True, help="the point of the curve that is written out, in [0, 1]")
    ap.add_argument("--kind", choices=("bezier", "polychain"), default="bezier")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scan", type=int, default=0, metavar="N", help="evaluate the loss at N points of the curve (0: no scan)")
    ap.add_argument("--trigger", default=None, help="a [C, H, W] trigger tensor: the scan also gives the poisoned loss (needs --target)")
    ap.add_argument("--target", default=None, help="the backdoor target's name (with --trigger)")
    ap.add_argument("--out", required=True, help="the directory of the repaired checkpoint")
    args = ap.parse_args(argv)
    if not 0.0 <= args.t <= 1.0:
        ap.error("--t must lie in [0, 1]")
    if (args.trigger is None) != (args.target is None):
        ap.error("--trigger and --target go together (the poisoned loss needs both)")
    if args.trigger is not None and args.scan < 1:
        ap.error("--trigger / --target are read by --scan only")
    if args.scan < 0 or args.scan == 1:
        ap.error("--scan takes 0 (no scan) or at least 2 points (both ends are included)")
    train = args.curve is None
    if train and (args.n_clean < 1 or args.batch < 1 or args.steps < 1):
        ap.error("--n-clean, --batch and --steps must be positive")
    if (train or args.scan) and args.dataset is None:
        ap.error("--dataset is needed to train the curve and to scan it")

    import torch
    from villandiffusion_amd import anchor, curve
    from villandiffusion_amd.curve import CurveConfig
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.loss import SDE_LDM, SDE_VE, SDE_VP, LossFn
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline
    from villandiffusion_amd.schedulers import ScoreSdeVeScheduler, get_cosine_schedule_with_warmup_lambda

    def family_of(ckpt, pipe):
        if os.path.isdir(os.path.join(ckpt, "vqvae")):
            return "ldm"
        return "ve" if isinstance(pipe.unet, NCSNppModel) and isinstance(pipe.scheduler, ScoreSdeVeScheduler) else "vp"

    pipe, pipe_b = DiffusionPipeline.from_pretrained(args.ckpt_a), DiffusionPipeline.from_pretrained(args.ckpt_b)
    net, sched = pipe.unet, pipe.scheduler
    family, family_b = family_of(args.ckpt_a, pipe), family_of(args.ckpt_b, pipe_b)
    if family != family_b or type(net) is not type(pipe_b.unet):
        raise ValueError(f"tools/mcr_repair.py: --ckpt-a is a {family!r} checkpoint ({type(net).__name__}), --ckpt-b a {family_b!r} one "
                         f"({type(pipe_b.unet).__name__}); a curve joins two checkpoints of one family")
    if anchor.layout_digest(net) != anchor.layout_digest(pipe_b.unet) or net.flat_numel != pipe_b.unet.flat_numel:
        raise ValueError(f"tools/mcr_repair.py: the parameter layouts differ: --ckpt-a has {net.flat_numel} floats, digest "
                         f"{anchor.layout_digest(net)[:12]}...; --ckpt-b has {pipe_b.unet.flat_numel}, {anchor.layout_digest(pipe_b.unet)[:12]}...")
    end_a, end_b = net.flat_param.detach().clone(), pipe_b.unet.flat_param.detach().clone()
    del pipe_b

    value_range, encode = {}, None
    if family == "ldm":
        from villandiffusion_amd import anp_ldm
        lf = LossFn(sched, SDE_LDM, psi=1)
        anp_ldm._check_pipeline("tools/mcr_repair.py", pipe)
        _, (channels, S, _) = anp_ldm._shapes(pipe)                        # the dataset is loaded at the VQ-VAE's pixel size and encoded
        encode = anp_ldm._family("tools/mcr_repair.py", pipe, torch.empty((1, channels, S, S))).prepare
    elif family == "ve":
        lf = LossFn(type(sched)(**vars(sched.config)), SDE_VE, psi=0)      # (the training sigma table, as anp_ve rebuilds it)
        channels, S, value_range = int(net.in_channels), int(net.sample_size), dict(vmin=0, vmax=1)
    else:
        lf = LossFn(sched, SDE_VP, psi=1)
        channels, S = int(net.in_channels), int(net.sample_size)

    batches, n_clean, dsl = [], 0, None
    if train or args.scan:
        dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed, **value_range)
        dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
        n_clean = min(args.n_clean, len(dsl))
        clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]
        if encode is not None:
            clean = encode(clean, max(args.batch, 8))
        batches = [clean[i:i + args.batch] for i in range(0, n_clean, args.batch)]
    for p in net.parameters():                                             # (from_pretrained hands the network out frozen or not; the curve's
        p.requires_grad_(True)                                             # gradient is the whole network's)
    if family == "ve":
        net.time_proj.weight.requires_grad_(False)                         # the fixed Fourier features are no trained weight

    info = {"ckpt_a": os.path.abspath(args.ckpt_a), "ckpt_b": os.path.abspath(args.ckpt_b), "family": family, "t": args.t, "seed": args.seed,
            "numel": int(net.flat_numel), "layout_sha256": anchor.layout_digest(net)}
    if train:
        cv = curve.Curve(net, end_a, end_b, CurveConfig(kind=args.kind, seed=args.seed))
        opt = curve.CurveAdam(cv, args.lr)                                   # (the network holds phi(t0) from here on)
        before = cv.geometry()
        T = anchor._timesteps_of(lf)
        lr_at = get_cosine_schedule_with_warmup_lambda(0, args.steps)        # the trainer's schedule, no warm-up
        losses = []
        for k in range(args.steps):
            x0 = batches[k % len(batches)]
            steps_k, eps = anchor.fisher_draws(x0.shape, T, args.seed + 1, k)                # (the scan's draws use --seed: other ones)
            losses.append(curve.curve_step(net, opt, lf, x0, None, steps_k, noise=eps, lr=args.lr * lr_at(k)))
        if int(opt.skipped):
            raise FloatingPointError(f"{int(opt.skipped)} optimiser step(s) had a non-finite gradient norm and were skipped by the Adam kernel")
        losses = [float(v) for v in torch.stack(losses).reshape(-1).cpu()]
        info.update(kind=args.kind, steps=args.steps, batch=args.batch, lr=args.lr, dataset=args.dataset, n_clean=n_clean,
                    geometry_before=before, geometry_after=cv.geometry(), last_losses=losses[-10:], curve_from=None)
    else:
        cv = curve.load_curve(args.curve, net, end_a, end_b)
        geo = cv.geometry()
        info.update(kind=cv.kind, steps=0, geometry_before=geo, geometry_after=geo, last_losses=[], curve_from=os.path.abspath(args.curve))

    scan = None
    if args.scan:
        ts = [i / (args.scan - 1) for i in range(args.scan)]
        trigger, scan_batches = None, batches
        if args.trigger is not None:
            trigger = torch.load(args.trigger, map_location="cpu").float()
            if encode is not None and tuple(trigger.shape[-2:]) != tuple(batches[0].shape[-2:]):
                raise ValueError(f"tools/mcr_repair.py: --trigger is {tuple(trigger.shape)}; a latent-diffusion scan takes a latent-shaped trigger "
                                 f"{tuple(batches[0].shape[1:])}")
            pix = torch.zeros((channels, S, S))
            target = dsl._backdoor.get_target(args.target, pix, vmin=dsl._vmin, vmax=dsl._vmax)
            if encode is not None:
                target = encode(target.unsqueeze(0), 8)[0]
            scan_batches = [{"image": b, "target": target} for b in batches]
        scan = curve.curve_scan(net, cv, lf, scan_batches, ts, seed=args.seed, trigger=trigger)
    info["scan"] = scan

    cv.point(args.t)                                                       # the network of `pipe` holds phi(t): that is what is saved
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    cv.save(os.path.join(args.out, curve.CURVE_FILE))
    with open(os.path.join(args.out, "mcr.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("family", "kind", "steps", "t", "geometry_after", "last_losses", "scan")}))


if __name__ == "__main__":
    main()
