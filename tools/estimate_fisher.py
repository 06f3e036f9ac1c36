"""Estimate the diagonal Fisher information of a diffusers-format checkpoint on clean data (villandiffusion_amd.anchor.estimate_fisher):
   python tools/estimate_fisher.py --ckpt DIR --dataset CIFAR10 --n-clean 512 --batch 8 [--normalize mean|max|none] [--seed 0] --out DIR/fisher.pt
takes the first --n-clean clean images of --dataset (no poisoning, no flips; SYNTHETIC-CIFAR10 needs no files) in batches of --batch and, per
batch, the gradient of the clean training loss at seeded timesteps and noise; F is the mean over the batches of the squared gradient, one launch
per batch over the flat gradient buffer.  --batch 1 gives the empirical Fisher; a larger batch the mean square of the batch-mean gradient, the
usual cheap approximation.  F is divided once by its mean (the default), its maximum, or not at all, and written as fisher.pt (the tensor, what
it was estimated on, and a digest of the parameter layout it belongs to): what `--anchor_fisher` of the training drivers and of
tools/remove_backdoor.py read.  A line with the Fisher's mean, its maximum and the share of entries below 1e-12 * max (before the division) is
printed and kept in fisher.json beside the file.

A directory with a vqvae/ folder is latent diffusion (family "ldm"): the dataset is loaded at the VQ-VAE's pixel size and encoded, the Fisher is
the latent UNet's.  An NCSNppModel with a ScoreSdeVeScheduler (family "ve") uses the SDE-VE loss on images in [0, 1]."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--dataset", required=True, help="where the clean images come from (villandiffusion_amd.dataset.DatasetLoader names)")
    ap.add_argument("--dataset-root", default="datasets", help="dataset root directory")
    ap.add_argument("--n-clean", type=int, default=512, help="clean images used (the first of the dataset)")
    ap.add_argument("--batch", type=int, default=8, help="images per gradient (1: the empirical Fisher)")
    ap.add_argument("--normalize", choices=("none", "mean", "max"), default="mean")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="the fisher.pt to write (or a directory to write it into)")
    args = ap.parse_args(argv)
    if args.n_clean < 1 or args.batch < 1:
        ap.error("--n-clean and --batch must be positive")

    import torch
    from villandiffusion_amd import anchor
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.loss import SDE_LDM, SDE_VE, SDE_VP, LossFn
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline
    from villandiffusion_amd.schedulers import ScoreSdeVeScheduler

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    net, sched = pipe.unet, pipe.scheduler
    value_range, encode = {}, None
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        from villandiffusion_amd import anp_ldm
        family, lf = "ldm", LossFn(sched, SDE_LDM, psi=1)
        anp_ldm._check_pipeline("tools/estimate_fisher.py", pipe)
        _, (channels, S, _) = anp_ldm._shapes(pipe)                        # the dataset is loaded at the VQ-VAE's pixel size and encoded
        encode = anp_ldm._family("tools/estimate_fisher.py", pipe, torch.empty((1, channels, S, S))).prepare
    elif isinstance(net, NCSNppModel) and isinstance(sched, ScoreSdeVeScheduler):
        family, lf = "ve", LossFn(type(sched)(**vars(sched.config)), SDE_VE, psi=0)      # (the training sigma table, as anp_ve rebuilds it)
        channels, S, value_range = int(net.in_channels), int(net.sample_size), dict(vmin=0, vmax=1)
    else:
        family, lf = "vp", LossFn(sched, SDE_VP, psi=1)
        channels, S = int(net.in_channels), int(net.sample_size)
    dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed, **value_range)
    dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
    n_clean = min(args.n_clean, len(dsl))
    clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]
    if encode is not None:
        clean = encode(clean, max(args.batch, 8))
    batches = [clean[i:i + args.batch] for i in range(0, n_clean, args.batch)]
    for p in net.parameters():                                             # (from_pretrained hands the network out frozen or not; the estimate
        p.requires_grad_(True)                                             # needs every gradient)
    if family == "ve":
        net.time_proj.weight.requires_grad_(False)                         # the fixed Fourier features are no trained weight: their F stays 0
    raw = anchor.estimate_fisher(net, lf, batches, seed=args.seed, normalize="none")
    stats = anchor.fisher_stats(raw)
    F = anchor.normalize_fisher(raw, args.normalize)
    path = anchor.save_fisher(args.out if not os.path.isdir(args.out) else os.path.join(args.out, anchor.FISHER_FILE), F, net,
                              n_batches=len(batches), batch=args.batch, normalize=args.normalize)
    info = {"ckpt": os.path.abspath(args.ckpt), "dataset": args.dataset, "n_clean": n_clean, "batch": args.batch, "n_batches": len(batches),
            "family": family, "normalize": args.normalize, "seed": args.seed, "numel": int(net.flat_numel),
            "layout_sha256": anchor.layout_digest(net), "out": os.path.abspath(path)} | stats
    with open(os.path.splitext(path)[0] + ".json", "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("family", "n_clean", "batch", "n_batches", "normalize", "numel", "mean", "max", "share_below_1e-12_max")}))


if __name__ == "__main__":
    main()
