"""Prune a diffusers-format checkpoint by Adversarial Neuron Pruning on a small clean set, without a trigger:
   python tools/anp_defense.py --ckpt DIR --dataset NAME --n-clean 512 --steps 200 --batch 64 [--anp-eps 0.4 --anp-steps 1 --anp-alpha 0.2
                               --lr 0.2 --layers conv --threshold 0.2 | --fraction F --sweep "f1,f2,..." --seed 0] --out DIR
learns a mask over the network's neurons (output rows of its weight tensors) under adversarial neuron perturbation on the first --n-clean clean
images of --dataset (no poisoning, no flips; SYNTHETIC-CIFAR10 needs no files), zeroes the weight rows whose mask is below --threshold (ANP's 0.2;
the default) or the --fraction of the network's neurons with the smallest masks, and writes into --out the pruned checkpoint (save_pretrained
layout), anp_mask.pt (weight name -> mask) and anp.json (family, settings, the natural and robust loss curves, per-layer pruned counts).
--sweep "f1,f2,..." adds anp.json["curve"]: the clean loss of the unpruned model and of the model pruned at each of these fractions, on the last
--batch clean images (`pruning_curve`), which is what a threshold is chosen with.

The module is picked from the checkpoint, as tools/invert_trigger.py, detect_backdoor.py and remove_backdoor.py pick theirs: a directory with
a vqvae/ folder (latent diffusion, family "ldm") goes to villandiffusion_amd.anp_ldm -- the dataset is loaded at the VQ-VAE's pixel size and
encoded, the latent UNet alone is pruned, the record gains "space"; an NCSNppModel with a ScoreSdeVeScheduler (family "ve") goes to
villandiffusion_amd.anp_ve -- the images are loaded in [0, 1]; anything else (family "vp") goes to villandiffusion_amd.anp."""
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
    ap.add_argument("--steps", type=int, default=200, help="mask-learning steps")
    ap.add_argument("--batch", type=int, default=64, help="clean images per step")
    ap.add_argument("--anp-eps", type=float, default=0.4, help="bound of the neuron perturbation (0: no perturbation, the natural loss alone)")
    ap.add_argument("--anp-steps", type=int, default=1, help="ascent iterations per step")
    ap.add_argument("--anp-alpha", type=float, default=0.2, help="weight of the natural loss; 1 - alpha weighs the robust one")
    ap.add_argument("--lr", type=float, default=0.2, help="step of the mask (SGD with momentum 0.9)")
    ap.add_argument("--layers", choices=("conv", "all"), default="conv", help="conv: the convolutions; all: attention projections and linears too")
    sel = ap.add_mutually_exclusive_group()
    sel.add_argument("--threshold", type=float, default=None, help="prune masks below this (default 0.2 when --fraction is not given)")
    sel.add_argument("--fraction", type=float, default=None, help="prune this fraction of all neurons, smallest masks first")
    ap.add_argument("--sweep", default=None, metavar="F1,F2,...",
                    help="fractions whose clean loss goes into anp.json[\"curve\"] (pruning_curve on the last --batch clean images)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory of the pruned checkpoint")
    args = ap.parse_args(argv)
    if args.n_clean < 1:
        ap.error("--n-clean must be positive")
    sweep = None
    if args.sweep is not None:
        try:
            sweep = [float(v) for v in args.sweep.split(",") if v.strip()]
        except ValueError:
            ap.error(f"--sweep takes comma-separated fractions, got {args.sweep!r}")
        if not sweep or not all(0.0 <= v < 1.0 for v in sweep):
            ap.error(f"--sweep takes fractions in [0, 1), got {args.sweep!r}")

    import torch
    from villandiffusion_amd import anp, anp_ldm, anp_ve
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline
    from villandiffusion_amd.schedulers import ScoreSdeVeScheduler

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    extra, value_range = {}, {}
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        family, mod, target = "ldm", anp_ldm, (pipe,)
        anp_ldm._check_pipeline("tools/anp_defense.py", pipe)
        _, (channels, S, _) = anp_ldm._shapes(pipe)                        # the dataset is loaded at the VQ-VAE's pixel size and encoded
        extra = {"space": "pixel"}
    elif isinstance(pipe.unet, NCSNppModel) and isinstance(pipe.scheduler, ScoreSdeVeScheduler):
        family, mod, target = "ve", anp_ve, (pipe.unet, pipe.scheduler)
        anp_ve._check_model("tools/anp_defense.py", pipe.unet, pipe.scheduler)
        channels, S, value_range = int(pipe.unet.in_channels), int(pipe.unet.sample_size), dict(vmin=0, vmax=1)
    else:
        family, mod, target = "vp", anp, (pipe.unet, pipe.scheduler)
        anp._check_model("tools/anp_defense.py", pipe.unet, pipe.scheduler)      # NotImplementedError for what no module here is built for
        channels, S = int(pipe.unet.in_channels), int(pipe.unet.sample_size)
    dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed, **value_range)
    dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
    n_clean = min(args.n_clean, len(dsl))
    clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]

    res = mod.learn_neuron_mask(*target, clean, steps=args.steps, batch=args.batch, anp_eps=args.anp_eps, anp_steps=args.anp_steps,
                                anp_alpha=args.anp_alpha, lr=args.lr, layers=args.layers, seed=args.seed)
    if sweep is not None:                                  # before the pruning: the curve is the unpruned model's
        extra["curve"] = mod.pruning_curve(*target, clean[-args.batch:], res, fractions=sweep, seed=args.seed)
    select = {"fraction": args.fraction} if args.fraction is not None else {"threshold": 0.2 if args.threshold is None else args.threshold}
    counts = mod.prune_neurons(target[0], res, **select)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    torch.save(res.masks, os.path.join(args.out, "anp_mask.pt"))
    flat = res.flat()
    info = {"ckpt": os.path.abspath(args.ckpt), "dataset": args.dataset, "n_clean": n_clean, "family": family} | res.settings() | select | \
        {"natural": res.natural, "robust": res.robust, "pruned": counts, "pruned_total": sum(counts.values()),
         "mask_min": float(flat.min()), "mask_mean": float(flat.mean())} | extra
    with open(os.path.join(args.out, "anp.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("steps", "batch", "layers", "n_neurons", "pruned_total", "mask_min", "mask_mean")} |
                     {"natural_first": res.natural[0], "natural_last": res.natural[-1]} |
                     ({"robust_last": res.robust[-1]} if res.robust else {})))


if __name__ == "__main__":
    main()
