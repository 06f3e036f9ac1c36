"""Repair a backdoored diffusers-format checkpoint from an inverted trigger, without data (villandiffusion_amd.mitigation.remove_backdoor):
   python tools/remove_backdoor.py --ckpt DIR --trigger trigger_inv.pt --steps 200 --batch 64 [--lr --w-clean 1 --w-shift 1 --seed 0] --out DIR
fine-tunes the UNet on pure noise so that eps + trigger gives what a frozen copy of the same model gives on eps, and writes the repaired
checkpoint (save_pretrained layout) and removal.json (settings and the three loss curves) into --out.  --lr defaults to the driver's fine-tune
rate for the model's size (2e-4 up to 64 x 64, 6e-5 above).  VP-type UNet2DModel checkpoints go to villandiffusion_amd.mitigation; a checkpoint
whose network is an NCSNppModel (SDE-VE, ScoreSdeVeScheduler) goes to villandiffusion_amd.defense_ve: the trigger is in noise units, the loss
terms are in noise-prediction units at sigma_T, the record gains "sigma".  A checkpoint directory with a vqvae/ folder (latent diffusion) goes to
villandiffusion_amd.defense_ldm: --trigger is latent-shaped or pixel-shaped (encoded once; the record gains "space"), the latent UNet alone is
fine-tuned and the VQ-VAE is written back as it was.  --anchor_lambda L [--anchor_fisher fisher.pt] holds the weights to the checkpoint's with
the L2-SP (or, with a Fisher of tools/estimate_fisher.py, the EWC) penalty of villandiffusion_amd.anchor; the record gains "anchor_lambda" and
"anchor_penalty", the penalty at the start of every step."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--trigger", required=True, help="the inverted trigger, a [C, H, W] tensor (tools/invert_trigger.py writes trigger_inv.pt)")
    ap.add_argument("--steps", type=int, required=True, help="Adam iterations")
    ap.add_argument("--batch", type=int, required=True, help="noise images per iteration (the training pass runs at twice this)")
    ap.add_argument("--lr", type=float, default=None, help="default: the driver's fine-tune rate for the model's size")
    ap.add_argument("--w-clean", type=float, default=1.0, help="weight of mse(model(eps), frozen(eps))")
    ap.add_argument("--w-shift", type=float, default=1.0, help="weight of mse(model(eps + trigger), frozen(eps))")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory of the repaired checkpoint")
    ap.add_argument("--anchor_lambda", type=float, default=None, help="weight of the penalty toward the checkpoint's weights (default: none)")
    ap.add_argument("--anchor_fisher", default=None, help="a fisher.pt of tools/estimate_fisher.py: EWC instead of L2-SP")
    args = ap.parse_args(argv)
    if args.anchor_fisher is not None and args.anchor_lambda is None:
        ap.error("--anchor_fisher needs --anchor_lambda")

    import torch
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    tau = torch.load(args.trigger, map_location="cpu")
    lr = args.lr if args.lr is not None else (2e-4 if int(pipe.unet.sample_size) <= 64 else 6e-5)
    kw = dict(steps=args.steps, batch=args.batch, lr=lr, w_clean=args.w_clean, w_shift=args.w_shift, seed=args.seed)
    if args.anchor_lambda is not None:
        from villandiffusion_amd.anchor import load_fisher
        kw.update(anchor_lambda=args.anchor_lambda, fisher=None if args.anchor_fisher is None else load_fisher(args.anchor_fisher, pipe.unet))
    space = None
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        from villandiffusion_amd import defense_ldm
        space = defense_ldm.trigger_space(pipe, tau)
        res = defense_ldm.remove_backdoor(pipe, tau, **kw)
    elif isinstance(pipe.unet, NCSNppModel):
        from villandiffusion_amd.defense_ve import remove_backdoor
        res = remove_backdoor(pipe.unet, pipe.scheduler, tau, **kw)
    else:
        from villandiffusion_amd.mitigation import remove_backdoor
        res = remove_backdoor(pipe.unet, pipe.scheduler, tau, **kw)
    os.makedirs(args.out, exist_ok=True)
    pipe.save_pretrained(args.out)
    info = {"ckpt": os.path.abspath(args.ckpt), "trigger": os.path.abspath(args.trigger), "steps": res.steps, "batch": res.batch, "lr": res.lr,
            "w_clean": res.w_clean, "w_shift": res.w_shift, "max_grad_norm": res.max_grad_norm, "seed": res.seed, "timestep": res.timestep,
            "total": res.total, "clean": res.clean, "shift": res.shift} | ({"sigma": res.sigma} if res.sigma is not None else {}) | \
        ({"space": space} if space is not None else {}) | \
        ({"anchor_lambda": res.anchor_lambda, "anchor_fisher": None if args.anchor_fisher is None else os.path.abspath(args.anchor_fisher),
          "anchor_penalty": res.anchor_penalty} if res.anchor_penalty is not None else {})
    with open(os.path.join(args.out, "removal.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("steps", "batch", "lr", "timestep")} | {"shift_first": res.shift[0], "shift_last": res.shift[-1],
                                                                                    "clean_last": res.clean[-1]}))


if __name__ == "__main__":
    main()
