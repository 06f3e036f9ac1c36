"""Invert the backdoor trigger of a diffusers-format checkpoint (distribution-shift objective of Elijah, villandiffusion_amd.defense):
   python tools/invert_trigger.py --ckpt DIR [--steps 100 --batch 100 --lam 0.5 --lr 0.1 --seed 0 --out DIR]
writes trigger_inv.pt (the trigger, [C, H, W]) and trigger_inv.json (settings, loss curve, ||tau||_2) into --out (default: the checkpoint
directory).  VP-type UNet2DModel checkpoints (DDPM / DDIM / LDM latent UNet) go to villandiffusion_amd.defense; a checkpoint whose network is
an NCSNppModel (SDE-VE, ScoreSdeVeScheduler) goes to villandiffusion_amd.defense_ve: the trigger is then in noise units, --timestep indexes the
ascending training sigma table, the record gains "sigma", and --lam 1 suits a backdoor trained with the ode solver.  A checkpoint directory
with a vqvae/ folder (latent diffusion) goes to villandiffusion_amd.defense_ldm: --space latent (the default) inverts the latent UNet as before
and trigger_inv.pt is the latent trigger; --space pixel searches over a pixel image through the VQ-VAE encoder and trigger_inv.pt is that image.
Either way trigger_inv.png shows it (a latent trigger decoded by the VQ-VAE) and the record gains "space"."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--steps", type=int, default=100, help="Adam iterations")
    ap.add_argument("--batch", type=int, default=100, help="noise images per iteration")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timestep", type=int, default=None, help="default: the scheduler's last training timestep")
    ap.add_argument("--space", choices=("latent", "pixel"), default="latent",
                    help="latent-diffusion checkpoints (vqvae/) only: the space the trigger is searched in (default: latent)")
    ap.add_argument("--out", default=None, help="output directory (default: --ckpt)")
    args = ap.parse_args(argv)
    ldm = os.path.isdir(os.path.join(args.ckpt, "vqvae"))
    if args.space != "latent" and not ldm:
        ap.error("--space pixel needs a latent-diffusion checkpoint (one with a vqvae/ folder)")

    import torch
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    kw = dict(steps=args.steps, batch=args.batch, lam=args.lam, lr=args.lr, seed=args.seed, timestep=args.timestep)
    if ldm:
        from villandiffusion_amd import defense_ldm
        res = defense_ldm.invert_trigger(pipe, space=args.space, **kw)
    elif isinstance(pipe.unet, NCSNppModel):
        from villandiffusion_amd.defense_ve import invert_trigger
        res = invert_trigger(pipe.unet, pipe.scheduler, **kw)
    else:
        from villandiffusion_amd.defense import invert_trigger
        res = invert_trigger(pipe.unet, pipe.scheduler, **kw)
    out = args.out or args.ckpt
    os.makedirs(out, exist_ok=True)
    torch.save(res.trigger.detach().cpu(), os.path.join(out, "trigger_inv.pt"))
    if ldm:
        from PIL import Image
        from villandiffusion_amd.pipelines import _post
        pix = res.trigger if args.space == "pixel" else defense_ldm.render_trigger(pipe, res.trigger)
        Image.fromarray((_post(pix.unsqueeze(0))[0] * 255).round().astype("uint8").squeeze()).save(os.path.join(out, "trigger_inv.png"))
    info = {"ckpt": os.path.abspath(args.ckpt), "steps": res.steps, "batch": res.batch, "lam": res.lam, "lr": res.lr, "seed": res.seed,
            "timestep": res.timestep, "losses": res.losses, "trigger_l2": res.trigger_norm} | {k: res.extra[k] for k in ("sigma", "space") if k in res.extra}
    with open(os.path.join(out, "trigger_inv.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("steps", "batch", "timestep", "trigger_l2")} | {"loss_first": res.losses[0], "loss_last": res.losses[-1]}))


if __name__ == "__main__":
    main()
