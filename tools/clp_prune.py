"""Prune a diffusers-format checkpoint by Channel Lipschitzness-based Pruning (villandiffusion_amd.clp), the data-free defence:
   python tools/clp_prune.py --ckpt DIR [--u 3] [--layers resnet|conv|all] [--scale gamma|none] [--sweep "2,3,4,5"]
                             [--dataset NAME --n-clean N --batch B] --out PRUNED
scores every output channel of the selected layers by UCLC = |gamma| * sigma_max(filter as [Cin, kh * kw]) in ONE launch over the network's
weights, and zeroes, per layer, the weight rows with UCLC > mean + u * std (the bias stays).  It needs no data, no trigger and no pass of the
network.  Written into --out: the pruned checkpoint (save_pretrained layout), prune_mask.pt (what `--keep_pruned` of the training drivers and
Trainer(keep_pruned=...) read) and clp.json: the family and settings, per layer the rows, mean, std, largest z, rows pruned and scale source,
and the totals.  --sweep "u1,u2,..." adds clp.json["sweep"]: the rows each u would prune; with --dataset also the clean loss of the unpruned
model and of the model pruned at each u, on the first --batch of --n-clean clean images (`pruning_curve`; UNet2DModel and latent diffusion:
NCSN++ goes through anp_ve).

A directory with a vqvae/ folder is latent diffusion (family "ldm"): the latent UNet alone is scored and pruned."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--u", type=float, default=3.0, help="prune the rows whose UCLC lies more than u standard deviations above its layer's mean")
    ap.add_argument("--layers", choices=("resnet", "conv", "all"), default="resnet")
    ap.add_argument("--scale", choices=("gamma", "none"), default="gamma")
    ap.add_argument("--sweep", default=None, metavar="U1,U2,...", help="values of u whose pruned counts (and clean loss, with --dataset) go into clp.json")
    ap.add_argument("--dataset", default=None, help="clean images for the sweep's loss (villandiffusion_amd.dataset.DatasetLoader names)")
    ap.add_argument("--dataset-root", default="datasets", help="dataset root directory")
    ap.add_argument("--n-clean", type=int, default=None, help="clean images loaded (the first of the dataset; default 64)")
    ap.add_argument("--batch", type=int, default=None, help="images of the sweep's one batch (default 64)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory of the pruned checkpoint")
    args = ap.parse_args(argv)
    if not math.isfinite(args.u):
        ap.error(f"--u must be finite, got {args.u}")
    sweep = None
    if args.sweep is not None:
        try:
            sweep = [float(v) for v in args.sweep.split(",") if v.strip()]
        except ValueError:
            ap.error(f"--sweep takes comma-separated values of u, got {args.sweep!r}")
        if not sweep or not all(math.isfinite(v) for v in sweep):
            ap.error(f"--sweep takes comma-separated values of u, got {args.sweep!r}")
    if args.dataset is None and (args.n_clean is not None or args.batch is not None):
        ap.error("--n-clean and --batch are read with --dataset")
    if args.dataset is not None and sweep is None:
        ap.error("--dataset is read with --sweep only: the defence itself needs no data")
    n_clean, batch = args.n_clean or 64, args.batch or 64
    if n_clean < 1 or batch < 1:
        ap.error("--n-clean and --batch must be positive")

    import torch
    from villandiffusion_amd import actprune, anp, anp_ldm, anp_ve, clp
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    what = "tools/clp_prune.py"
    net = pipe.unet
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        family = "ldm"
    elif isinstance(net, NCSNppModel):
        family = "ve"
    else:
        family = "vp"
    uclc, settings = clp.channel_lipschitz(net, layers=args.layers, scale=args.scale)      # the one launch
    z = clp.clp_z(uclc)
    keep_of = lambda u: {name: (~(v > u)).to(torch.float32) for name, v in z.items()}
    anp._selection(what, net, keep_of(args.u), threshold=0.5)                              # ValueError for an emptied layer before anything runs
    extra = {}
    if sweep is not None:
        recs = [{"u": u, "pruned": int(sum(int((v > u).sum()) for v in z.values()))} for u in sweep]
        if args.dataset is not None:                                                       # before the pruning: the curve is the unpruned model's
            from villandiffusion_amd.dataset import DatasetLoader
            if family == "ldm":
                anp_ldm._check_pipeline(what, pipe)
                _, (channels, S, _) = anp_ldm._shapes(pipe)
                curve = lambda *a, **k: anp_ldm.pruning_curve(pipe, *a, **k)
            elif family == "ve":
                channels, S = int(net.in_channels), int(net.sample_size)
                curve = lambda *a, **k: anp_ve.pruning_curve(net, pipe.scheduler, *a, **k)
            else:
                anp._check_model(what, net, pipe.scheduler)
                channels, S = int(net.in_channels), int(net.sample_size)
                curve = lambda *a, **k: anp.pruning_curve(net, pipe.scheduler, *a, **k)
            dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=channels, image_size=S, shuffle=False, seed=args.seed)
            dsl.set_poison("NONE", "CORNER", clean_rate=1.0, poison_rate=0.0).prepare_dataset(mode=DatasetLoader.MODE_NONE)     # nothing is poisoned
            n = min(n_clean, len(dsl))
            clean = dsl.make_batch(torch.arange(n), flip_bits=torch.zeros(n, dtype=torch.bool), full=False)[DatasetLoader.IMAGE][:batch]
            losses = [curve(clean, keep_of(u), thresholds=[0.5], seed=args.seed) for u in sweep]
            extra["loss_unpruned"] = losses[0][0]["loss"]
            for rec, cv in zip(recs, losses):
                assert cv[1]["pruned"] == rec["pruned"], (cv, rec)
                rec["loss"] = cv[1]["loss"]
            extra |= {"dataset": args.dataset, "n_clean": int(clean.shape[0])}
        extra["sweep"] = recs
    stats = clp.layer_statistics(uclc, args.u)
    mask = clp.clp_prune(net, u=args.u, uclc=uclc)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    mask.save(os.path.join(args.out, actprune.MASK_FILE))
    per_layer = {name: rec | {"scale_source": settings["scale_source"][name], "taps": settings["taps"][name]} for name, rec in stats.items()}
    info = {"ckpt": os.path.abspath(args.ckpt), "family": family, "u": args.u} | \
        {k: settings[k] for k in ("layers", "scale", "n_layers", "n_channels", "weight_floats", "sweeps")} | \
        {"per_layer": per_layer, "pruned": mask.pruned, "pruned_total": mask.n_pruned,
         "z_max": max(rec["z_max"] for rec in stats.values() if rec["z_max"] is not None)} | extra
    with open(os.path.join(args.out, "clp.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("family", "layers", "scale", "u", "n_layers", "n_channels", "pruned_total", "z_max")}))


if __name__ == "__main__":
    main()
