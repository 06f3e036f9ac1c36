"""Prune a diffusers-format checkpoint by what its channels do on data (villandiffusion_amd.actprune):
   python tools/fine_prune.py --ckpt DIR --dataset NAME --n-clean 512 --batch 64 [--score dormancy|sensitivity] [--trigger trigger_inv.pt]
                              (--fraction F | --threshold T) [--sweep "0.01,0.02,0.05"] [--seed 0] --out PRUNED
takes the per-channel statistics of silu(norm2(.)) in every ResnetBlock on the first --n-clean clean images of --dataset (no poisoning, no flips;
SYNTHETIC-CIFAR10 needs no files) and scores the `conv1` output channels:
  --score dormancy (Fine-Pruning; the default): the root mean square of the activation, the most dormant channel first;
  --score sensitivity: -|mean with the trigger - clean mean| / clean standard deviation, the most trigger-sensitive channel first; needs
  --trigger, the [C, H, W] tensor tools/invert_trigger.py writes (latent-shaped for a latent-diffusion checkpoint).
The --fraction of the scored channels with the smallest scores, or every channel whose score is below --threshold, is pruned: its `conv1`
weight row is zeroed (the bias and the time-embedding row stay).  Written into --out: the pruned checkpoint (save_pretrained layout),
prune_mask.pt (what `--keep_pruned` of the training drivers and Trainer(keep_pruned=...) read) and fine_prune.json (settings, "family",
per-layer pruned counts).  --sweep "f1,f2,..." adds fine_prune.json["curve"]: the clean loss of the unpruned model and of the model pruned at
each of these fractions, on the last --batch clean images (`pruning_curve`).

A directory with a vqvae/ folder is latent diffusion (family "ldm"): the dataset is loaded at the VQ-VAE's pixel size and encoded, the latent
UNet alone is pruned.  An NCSNppModel is refused: not built."""
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
    ap.add_argument("--batch", type=int, default=64, help="images per forward")
    ap.add_argument("--score", choices=("dormancy", "sensitivity"), default="dormancy")
    ap.add_argument("--trigger", default=None, help="the inverted trigger, a [C, H, W] tensor (tools/invert_trigger.py writes trigger_inv.pt)")
    sel = ap.add_mutually_exclusive_group(required=True)
    sel.add_argument("--fraction", type=float, default=None, help="prune this fraction of the scored channels, smallest scores first")
    sel.add_argument("--threshold", type=float, default=None, help="prune the channels whose score is below this")
    ap.add_argument("--sweep", default=None, metavar="F1,F2,...",
                    help="fractions whose clean loss goes into fine_prune.json[\"curve\"] (pruning_curve on the last --batch clean images)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory of the pruned checkpoint")
    args = ap.parse_args(argv)
    if args.n_clean < 1 or args.batch < 1:
        ap.error("--n-clean and --batch must be positive")
    if args.score == "sensitivity" and args.trigger is None:
        ap.error("--score sensitivity needs --trigger: the score is how far a channel's mean activation moves when the trigger is added to the "
                 "input, so there must be a trigger to add (tools/invert_trigger.py writes trigger_inv.pt)")
    if args.score == "dormancy" and args.trigger is not None:
        ap.error("--trigger is read by --score sensitivity only")
    if args.fraction is not None and not 0.0 <= args.fraction < 1.0:
        ap.error(f"--fraction must lie in [0, 1), got {args.fraction}")
    sweep = None
    if args.sweep is not None:
        try:
            sweep = [float(v) for v in args.sweep.split(",") if v.strip()]
        except ValueError:
            ap.error(f"--sweep takes comma-separated fractions, got {args.sweep!r}")
        if not sweep or not all(0.0 <= v < 1.0 for v in sweep):
            ap.error(f"--sweep takes fractions in [0, 1), got {args.sweep!r}")

    import torch
    from villandiffusion_amd import actprune, anp, anp_ldm
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    what = "tools/fine_prune.py"
    actprune._unet_of(what, pipe)                                          # NotImplementedError for NCSN++, saying what is missing
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        family, target, curve = "ldm", pipe, lambda *a, **k: anp_ldm.pruning_curve(pipe, *a, **k)
        anp_ldm._check_pipeline(what, pipe)
        _, (channels, S, _) = anp_ldm._shapes(pipe)                        # the dataset is loaded at the VQ-VAE's pixel size and encoded
    else:
        family, target, curve = "vp", pipe.unet, lambda *a, **k: anp.pruning_curve(pipe.unet, pipe.scheduler, *a, **k)
        anp._check_model(what, pipe.unet, pipe.scheduler)
        channels, S = int(pipe.unet.in_channels), int(pipe.unet.sample_size)
    trigger = None
    if args.trigger is not None:
        trigger = torch.load(args.trigger, map_location="cpu")
    dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed)
    dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
    n_clean = min(args.n_clean, len(dsl))
    clean = dsl.make_batch(torch.arange(n_clean), flip_bits=torch.zeros(n_clean, dtype=torch.bool), full=False)[DatasetLoader.IMAGE]

    kw = dict(batch=args.batch, seed=args.seed)
    stats = actprune.channel_stats(target, pipe.scheduler, clean, **kw)
    if args.score == "sensitivity":
        scores = actprune.sensitivity_scores(stats, actprune.channel_stats(target, pipe.scheduler, clean, trigger=trigger, **kw))
    else:
        scores = actprune.dormancy_scores(stats)
    extra = {}
    select = {"fraction": args.fraction} if args.fraction is not None else {"threshold": args.threshold}
    anp._selection(what, pipe.unet, scores, **select)                      # ValueError for an emptied layer before the sweep runs
    if sweep is not None:                                                  # before the pruning: the curve is the unpruned model's
        extra["curve"] = curve(clean[-args.batch:], scores, fractions=sweep, seed=args.seed)
    mask = actprune.fine_prune(pipe.unet, scores, **select)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    mask.save(os.path.join(args.out, actprune.MASK_FILE))
    flat = torch.cat([scores[n] for n in stats.table.names])
    info = {"ckpt": os.path.abspath(args.ckpt), "dataset": args.dataset, "n_clean": n_clean, "family": family, "score": args.score,
            "trigger": None if args.trigger is None else os.path.abspath(args.trigger)} | stats.settings() | select | \
        {"pruned": mask.pruned, "pruned_total": mask.n_pruned, "score_min": float(flat.min()), "score_median": float(flat.median())} | extra
    with open(os.path.join(args.out, "fine_prune.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("family", "score", "layers", "n_channels", "pruned_total", "score_min", "score_median")}))


if __name__ == "__main__":
    main()
