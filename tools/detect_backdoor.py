"""Backdoor detection features of a diffusers-format checkpoint from an inverted trigger (Elijah's uniformity / total-variation features,
villandiffusion_amd.mitigation):
   python tools/detect_backdoor.py --ckpt DIR --trigger trigger_inv.pt --n 256 --batch 64 [--steps 50 --seed 0 --threshold X --out DIR]
samples --n images from eps and --n from eps + trigger (the same eps) and writes detection.json (both feature sets, their ratios, the settings;
a verdict only when --threshold is given: nothing here has been calibrated) and mean_shifted.pt (the mean shifted image, [C, H, W] in [0, 1]:
for a collapsed set, the recovered target) into --out (default: the checkpoint directory).  Pixel-space UNet2DModel checkpoints (DDPM / DDIM /
...) go to villandiffusion_amd.mitigation; a checkpoint whose network is an NCSNppModel (ScoreSdeVePipeline) goes to
villandiffusion_amd.defense_ve: the sets start from sigma_T * eps and sigma_T * (eps + trigger), the record gains "sigma".  A checkpoint
directory with a vqvae/ folder (latent diffusion) goes to villandiffusion_amd.defense_ldm: --trigger is latent-shaped or pixel-shaped (the record
gains "space"), the top-level features are those of the decoded images, the record gains a "latent" block with those of the final latents, and
mean_shifted.pt is the mean decoded image.  Karras-VE checkpoints are refused."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--trigger", required=True, help="the inverted trigger, a [C, H, W] tensor (tools/invert_trigger.py writes trigger_inv.pt)")
    ap.add_argument("--n", type=int, required=True, help="images per set")
    ap.add_argument("--batch", type=int, required=True, help="images per sampler chunk")
    ap.add_argument("--steps", type=int, default=None, help="sampler steps (default: the pipeline's own)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=None, help="report verdict = uniformity_ratio < THRESHOLD (no default: uncalibrated)")
    ap.add_argument("--out", default=None, help="output directory (default: --ckpt)")
    args = ap.parse_args(argv)

    import torch
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        from villandiffusion_amd.defense_ldm import backdoor_features
    elif isinstance(pipe.unet, NCSNppModel):
        from villandiffusion_amd.defense_ve import backdoor_features
        from villandiffusion_amd.pipelines import ScoreSdeVePipeline
        pipe = ScoreSdeVePipeline(pipe.unet, pipe.scheduler)      # (from_pretrained hands back the base class: the predictor-corrector loop is this one's)
    else:
        from villandiffusion_amd.mitigation import backdoor_features
    tau = torch.load(args.trigger, map_location="cpu")
    res = backdoor_features(pipe, tau, n=args.n, batch=args.batch, num_inference_steps=args.steps, seed=args.seed)
    out = args.out or args.ckpt
    os.makedirs(out, exist_ok=True)
    torch.save(res.shifted.mean_image.detach().cpu(), os.path.join(out, "mean_shifted.pt"))
    info = {"ckpt": os.path.abspath(args.ckpt), "trigger": os.path.abspath(args.trigger), "pipeline": type(pipe).__name__} | res.as_dict()
    if res.sigma is not None:
        info["sigma"] = res.sigma
    if args.threshold is not None:
        info["threshold"] = args.threshold
        info["verdict"] = bool(res.verdict(args.threshold))
    with open(os.path.join(out, "detection.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("n", "batch", "num_inference_steps", "uniformity_ratio", "tv_ratio")} |
                     ({"verdict": info["verdict"]} if "verdict" in info else {})))


if __name__ == "__main__":
    main()
