"""Merge diffusers-format checkpoints that were fine-tuned from one base (villandiffusion_amd.merge; task arithmetic, Ilharco et al. 2023, and
TIES-Merging, Yadav et al. 2023):
   python tools/merge_checkpoints.py --base BASE --ckpt A B C --method ties --density 0.2 --lam 1.0 --out MERGED
                                     [--weights "0.5,0.5,-1"] [--drop 0.9 [--seed 0] [--no-rescale]]
                                     [--scan "0.3,0.5,1.0" --dataset NAME --n-clean 64 --batch 64 [--trigger FILE --target NAME]]
   python tools/merge_checkpoints.py --base CLEAN --ckpt BACKDOORED --method mix --mix-keep 0.3 [--seed 0] --out MIXED
takes the base checkpoint and one to eight fine-tunes of it (one family, one parameter layout), forms the task vectors ckpt - base, and writes
   MERGED/             the checkpoint of BASE with the merged weights,
   MERGED/merge.json   family, method, density, lam, weights, k, the read-outs of merge() (per task: threshold, kept and won shares, norm;
                       support and sign-conflict shares; the cosines between the task vectors), the layout digest, the paths and "scan";
                       with --drop also drop, seed, rescale and per task drop_threshold, drawn, drawn_share.
--method linear is theta = base + sum_i lambda_i (ckpt_i - base) with lambda_i = lam * weights_i (--weights; default 1 / K each: the average;
a negative weight subtracts what that fine-tune added); --density below 1 trims every task vector to its largest entries first.
--method ties trims, elects one sign per parameter and averages the entries that agree with it, times --lam.
--drop P (or "p1,p2,...", one per checkpoint) is DARE (Yu et al. 2024): every entry of a task vector is dropped with probability P and the
survivors are multiplied by 1 / (1 - P) (--no-rescale: left as they are) before --method linear adds them (DARE-linear) or --method ties elects
signs over them (DARE-TIES; usually with --density 1).  The draw is a function of --seed, the checkpoint's position and the parameter's index.
--method mix is Fine-mixing (Zhang et al. 2022): exactly one --ckpt, the backdoored fine-tune of the clean --base; a random share --mix-keep of
its weights is kept and the rest is taken from the base.  MIXED/merge.json holds the record under "mix"; --scan takes keep shares then.  The
mixed checkpoint is then fine-tuned on a little clean data by the ordinary driver.
--scan "l1,l2,..." evaluates the clean loss of the merge at each lam on the first --n-clean images of --dataset (SYNTHETIC-CIFAR10 needs no
files); with --trigger FILE (a [C, H, W] tensor) and --target NAME every lam also gets the poisoned loss.  No data is needed otherwise.

A directory with a vqvae/ folder is latent diffusion (family "ldm"): the dataset is loaded at the VQ-VAE's pixel size and encoded first, and only
the latent UNet is merged.  An NCSNppModel with a ScoreSdeVeScheduler is family "ve"."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def floats_of(text, what, ap):
    try:
        out = [float(v) for v in text.split(",") if v.strip() != ""]
    except ValueError:
        out = []
    if not out or any(v != v or v in (float("inf"), float("-inf")) for v in out):
        ap.error(f"{what} takes a comma-separated list of finite numbers, got {text!r}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", required=True, help="diffusers-format checkpoint directory of the base every --ckpt was fine-tuned from")
    ap.add_argument("--ckpt", required=True, nargs="+", help="one to eight fine-tuned checkpoints of the base's family and parameter layout")
    ap.add_argument("--method", choices=("ties", "linear", "mix"), default="ties")
    ap.add_argument("--density", type=float, default=0.2, help="share of each task vector that is kept (largest magnitudes), in [0, 1]")
    ap.add_argument("--lam", type=float, default=1.0, help="scale of the merged task vector")
    ap.add_argument("--weights", default=None, help='per-checkpoint weights of --method linear, e.g. "0.5,0.5,-1" (default: 1 / K each)')
    ap.add_argument("--drop", default=None, help='DARE: drop each entry of a task vector with this probability in [0, 1), e.g. 0.9, or one per '
                                                 'checkpoint, e.g. "0.9,0.9,0.5"')
    ap.add_argument("--no-rescale", action="store_true", help="with --drop: do not multiply the surviving entries by 1 / (1 - P)")
    ap.add_argument("--mix-keep", type=float, default=None, help="--method mix: the share of the backdoored weights that is kept, in [0, 1]")
    ap.add_argument("--scan", default=None, help='evaluate the loss of the merge at these lam, e.g. "0.3,0.5,1.0" (--method mix: at these keep '
                                                 'shares; needs --dataset)')
    ap.add_argument("--dataset", default=None, help="where the clean images of --scan come from (villandiffusion_amd.dataset.DatasetLoader names)")
    ap.add_argument("--dataset-root", default="datasets", help="dataset root directory")
    ap.add_argument("--n-clean", type=int, default=64, help="clean images used by --scan (the first of the dataset)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0, help="seed of the scan's timesteps and noise, and of the draw of --drop and --method mix")
    ap.add_argument("--trigger", default=None, help="a [C, H, W] trigger tensor: the scan also gives the poisoned loss (needs --target)")
    ap.add_argument("--target", default=None, help="the backdoor target's name (with --trigger)")
    ap.add_argument("--out", required=True, help="the directory of the merged checkpoint")
    args = ap.parse_args(argv)
    K = len(args.ckpt)
    if K > 8:
        ap.error(f"--ckpt names {K} checkpoints; one merge takes 1 to 8")
    if not 0.0 <= args.density <= 1.0:
        ap.error("--density must lie in [0, 1]")
    if args.lam != args.lam or args.lam in (float("inf"), float("-inf")):
        ap.error("--lam must be finite")
    weights = None
    if args.weights is not None:
        if args.method != "linear":
            ap.error("--weights are the per-checkpoint weights of --method linear")
        weights = floats_of(args.weights, "--weights", ap)
        if len(weights) != K:
            ap.error(f"--weights holds {len(weights)} numbers, --ckpt names {K} checkpoints")
    mix = args.method == "mix"
    if mix:
        if K != 1:
            ap.error(f"--method mix takes exactly one --ckpt (the backdoored fine-tune of --base), --ckpt names {K}")
        if args.mix_keep is None:
            ap.error("--method mix needs --mix-keep")
        if not 0.0 <= args.mix_keep <= 1.0:
            ap.error("--mix-keep must lie in [0, 1]")
        if args.drop is not None:
            ap.error("--drop is read by --method ties and --method linear only")
    elif args.mix_keep is not None:
        ap.error("--mix-keep is read by --method mix only")
    drop = None
    if args.drop is not None:
        drop = floats_of(args.drop, "--drop", ap)
        if not all(0.0 <= v < 1.0 for v in drop):
            ap.error("--drop must lie in [0, 1)")
        if len(drop) == 1:
            drop = drop[0]
        elif len(drop) != K:
            ap.error(f"--drop holds {len(drop)} numbers, --ckpt names {K} checkpoints")
    elif args.no_rescale:
        ap.error("--no-rescale is read with --drop only")
    if (drop is not None or mix) and not 0 <= args.seed < 1 << 64:
        ap.error("--seed must lie in [0, 2^64) with --drop and --method mix")
    lams = None
    if args.scan is not None:
        lams = floats_of(args.scan, "--scan", ap)
        if mix and not all(0.0 <= v <= 1.0 for v in lams):
            ap.error("--scan takes keep shares in [0, 1] with --method mix")
        if args.dataset is None:
            ap.error("--dataset is needed to scan the merge")
        if args.n_clean < 1 or args.batch < 1:
            ap.error("--n-clean and --batch must be positive")
    if (args.trigger is None) != (args.target is None):
        ap.error("--trigger and --target go together (the poisoned loss needs both)")
    if args.trigger is not None and lams is None:
        ap.error("--trigger / --target are read by --scan only")

    import torch
    from villandiffusion_amd import anchor, merge
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.loss import SDE_LDM, SDE_VE, SDE_VP, LossFn
    from villandiffusion_amd.merge import MergeConfig
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline
    from villandiffusion_amd.schedulers import ScoreSdeVeScheduler

    def family_of(ckpt, pipe):
        if os.path.isdir(os.path.join(ckpt, "vqvae")):
            return "ldm"
        return "ve" if isinstance(pipe.unet, NCSNppModel) and isinstance(pipe.scheduler, ScoreSdeVeScheduler) else "vp"

    pipe = DiffusionPipeline.from_pretrained(args.base)
    net, sched = pipe.unet, pipe.scheduler
    family, digest = family_of(args.base, pipe), anchor.layout_digest(net)
    tasks = []
    for path in args.ckpt:
        other = DiffusionPipeline.from_pretrained(path)
        fam = family_of(path, other)
        if fam != family or type(other.unet) is not type(net):
            raise ValueError(f"tools/merge_checkpoints.py: --base {args.base} is a {family!r} checkpoint ({type(net).__name__}), --ckpt {path} a "
                             f"{fam!r} one ({type(other.unet).__name__}); a merge takes checkpoints of one family")
        if anchor.layout_digest(other.unet) != digest or other.unet.flat_numel != net.flat_numel:
            raise ValueError(f"tools/merge_checkpoints.py: the parameter layouts differ: --base {args.base} has {net.flat_numel} floats, digest "
                             f"{digest}; --ckpt {path} has {other.unet.flat_numel}, digest {anchor.layout_digest(other.unet)}")
        tasks.append(other.unet.flat_param.detach().clone())
        del other
    base = net.flat_param.detach().clone()
    cfg = None if mix else MergeConfig(method=args.method, density=args.density, lam=args.lam, weights=weights,
                                       **({} if drop is None else dict(drop=drop, seed=args.seed, rescale=not args.no_rescale)))

    scan = None
    if lams is not None:
        value_range, encode = {}, None
        if family == "ldm":
            from villandiffusion_amd import anp_ldm
            lf = LossFn(sched, SDE_LDM, psi=1)
            anp_ldm._check_pipeline("tools/merge_checkpoints.py", pipe)
            _, (channels, S, _) = anp_ldm._shapes(pipe)                    # the dataset is loaded at the VQ-VAE's pixel size and encoded
            encode = anp_ldm._family("tools/merge_checkpoints.py", pipe, torch.empty((1, channels, S, S))).prepare
        elif family == "ve":
            lf = LossFn(type(sched)(**vars(sched.config)), SDE_VE, psi=0)  # (the training sigma table, as anp_ve rebuilds it)
            channels, S, value_range = int(net.in_channels), int(net.sample_size), dict(vmin=0, vmax=1)
        else:
            lf = LossFn(sched, SDE_VP, psi=1)
            channels, S = int(net.in_channels), int(net.sample_size)
        dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed, **value_range)
        dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
        n_clean = min(args.n_clean, len(dsl))
        clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]
        if encode is not None:
            clean = encode(clean, max(args.batch, 8))
        batches = [clean[i:i + args.batch] for i in range(0, n_clean, args.batch)]
        trigger, scan_batches = None, batches
        if args.trigger is not None:
            trigger = torch.load(args.trigger, map_location="cpu").float()
            if encode is not None and tuple(trigger.shape[-2:]) != tuple(batches[0].shape[-2:]):
                raise ValueError(f"tools/merge_checkpoints.py: --trigger is {tuple(trigger.shape)}; a latent-diffusion scan takes a latent-shaped "
                                 f"trigger {tuple(batches[0].shape[1:])}")
            pix = torch.zeros((channels, S, S))
            target = dsl._backdoor.get_target(args.target, pix, vmin=dsl._vmin, vmax=dsl._vmax)
            if encode is not None:
                target = encode(target.unsqueeze(0), 8)[0]
            scan_batches = [{"image": b, "target": target} for b in batches]
        if mix:
            scan = merge.fine_mix_scan(net, base, tasks[0], lf, scan_batches, lams, seed=args.seed, data_seed=args.seed, trigger=trigger)
        else:
            scan = merge.merge_scan(net, base, tasks, cfg, lf, scan_batches, lams, seed=args.seed, trigger=trigger)

    if mix:
        report = merge.fine_mix(net, base, tasks[0], args.mix_keep, seed=args.seed)     # the network of `pipe` holds the mix: that is what is saved
        info = {"base": os.path.abspath(args.base), "ckpt": [os.path.abspath(p) for p in args.ckpt], "out": os.path.abspath(args.out),
                "family": family, "method": "mix", "numel": int(net.flat_numel), "layout_sha256": digest, "mix": report, "scan": scan}
    else:
        report = merge.merge(net, base, tasks, cfg)                        # the network of `pipe` holds the merge: that is what is saved
        info = {"base": os.path.abspath(args.base), "ckpt": [os.path.abspath(p) for p in args.ckpt], "out": os.path.abspath(args.out),
                "family": family, "method": args.method, "density": args.density, "lam": args.lam, "weights": weights, "k": report["k"],
                "numel": int(net.flat_numel), "layout_sha256": digest, "merge": report, "scan": scan}
        if drop is not None:
            info.update(drop=report.get("drop", drop), seed=args.seed, rescale=not args.no_rescale)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    with open(os.path.join(args.out, "merge.json"), "w") as f:
        json.dump(info, f, indent=1)
    if mix:
        print(json.dumps({"family": family, "method": "mix", "scan": scan} | {k: report[k] for k in ("keep", "seed", "drawn_share", "differing")}))
        return
    print(json.dumps({k: info[k] for k in ("family", "method", "density", "lam", "weights", "k", "scan")} |
                     {"support_share": report["support_share"], "conflict_share": report["conflict_share"]}))


if __name__ == "__main__":
    main()
