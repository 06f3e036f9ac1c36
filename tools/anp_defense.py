"""Prune a diffusers-format checkpoint by Adversarial Neuron Pruning on a small clean set, without a trigger (villandiffusion_amd.anp):
   python tools/anp_defense.py --ckpt DIR --dataset NAME --n-clean 512 --steps 200 --batch 64 [--anp-eps 0.4 --anp-steps 1 --anp-alpha 0.2
                               --lr 0.2 --layers conv --threshold 0.2 | --fraction F --seed 0] --out DIR
learns a mask over the UNet's neurons (output rows of its weight tensors) under adversarial neuron perturbation on the first --n-clean clean
images of --dataset (no poisoning, no flips; SYNTHETIC-CIFAR10 needs no files), zeroes the weight rows whose mask is below --threshold (ANP's 0.2;
the default) or the --fraction of the network's neurons with the smallest masks, and writes into --out the pruned checkpoint (save_pretrained
layout), anp_mask.pt (weight name -> mask) and anp.json (settings, the natural and robust loss curves, per-layer pruned counts).  Pixel-space
VP-type UNet2DModel checkpoints only: SDE-VE (NCSN++) and latent-diffusion checkpoints are refused."""
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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory of the pruned checkpoint")
    args = ap.parse_args(argv)
    if args.n_clean < 1:
        ap.error("--n-clean must be positive")

    import torch
    from villandiffusion_amd import anp
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")) or getattr(pipe, "vqvae", None) is not None:
        raise NotImplementedError("tools/anp_defense.py: latent-diffusion checkpoints are out of scope; pixel-space VP-type UNet2DModel only")
    anp._check_model("tools/anp_defense.py", pipe.unet, pipe.scheduler)              # NotImplementedError for NCSN++ / VE schedulers
    S = int(pipe.unet.sample_size)
    dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=int(pipe.unet.in_channels), image_size=S, shuffle=False, seed=args.seed)
    dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
    n_clean = min(args.n_clean, len(dsl))
    clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]

    res = anp.learn_neuron_mask(pipe.unet, pipe.scheduler, clean, steps=args.steps, batch=args.batch, anp_eps=args.anp_eps, anp_steps=args.anp_steps,
                                anp_alpha=args.anp_alpha, lr=args.lr, layers=args.layers, seed=args.seed)
    select = {"fraction": args.fraction} if args.fraction is not None else {"threshold": 0.2 if args.threshold is None else args.threshold}
    counts = anp.prune_neurons(pipe.unet, res, **select)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    torch.save(res.masks, os.path.join(args.out, "anp_mask.pt"))
    flat = res.flat()
    info = {"ckpt": os.path.abspath(args.ckpt), "dataset": args.dataset, "n_clean": n_clean} | res.settings() | select | \
        {"natural": res.natural, "robust": res.robust, "pruned": counts, "pruned_total": sum(counts.values()),
         "mask_min": float(flat.min()), "mask_mean": float(flat.mean())}
    with open(os.path.join(args.out, "anp.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("steps", "batch", "layers", "n_neurons", "pruned_total", "mask_min", "mask_mean")} |
                     {"natural_first": res.natural[0], "natural_last": res.natural[-1]} |
                     ({"robust_last": res.robust[-1]} if res.robust else {})))


if __name__ == "__main__":
    main()
