"""Invert the backdoor trigger of a diffusers-format checkpoint (distribution-shift objective of Elijah, villandiffusion_amd.defense):
   python tools/invert_trigger.py --ckpt DIR [--steps 100 --batch 100 --lam 0.5 --lr 0.1 --seed 0 --out DIR]
writes trigger_inv.pt (the trigger, [C, H, W]) and trigger_inv.json (settings, loss curve, ||tau||_2) into --out (default: the checkpoint
directory).  VP-type UNet2DModel checkpoints (DDPM / DDIM / LDM latent UNet) go to villandiffusion_amd.defense; a checkpoint whose network is
an NCSNppModel (SDE-VE, ScoreSdeVeScheduler) goes to villandiffusion_amd.defense_ve: the trigger is then in noise units, --timestep indexes the
ascending training sigma table, the record gains "sigma", and --lam 1 suits a backdoor trained with the ode solver."""
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
    ap.add_argument("--out", default=None, help="output directory (default: --ckpt)")
    args = ap.parse_args(argv)

    import torch
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    if isinstance(pipe.unet, NCSNppModel):
        from villandiffusion_amd.defense_ve import invert_trigger
    else:
        from villandiffusion_amd.defense import invert_trigger
    res = invert_trigger(pipe.unet, pipe.scheduler, steps=args.steps, batch=args.batch, lam=args.lam, lr=args.lr, seed=args.seed,
                         timestep=args.timestep)
    out = args.out or args.ckpt
    os.makedirs(out, exist_ok=True)
    torch.save(res.trigger.detach().cpu(), os.path.join(out, "trigger_inv.pt"))
    info = {"ckpt": os.path.abspath(args.ckpt), "steps": res.steps, "batch": res.batch, "lam": res.lam, "lr": res.lr, "seed": res.seed,
            "timestep": res.timestep, "losses": res.losses, "trigger_l2": res.trigger_norm} | ({"sigma": res.extra["sigma"]} if "sigma" in res.extra else {})
    with open(os.path.join(out, "trigger_inv.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("steps", "batch", "timestep", "trigger_l2")} | {"loss_first": res.losses[0], "loss_last": res.losses[-1]}))


if __name__ == "__main__":
    main()
