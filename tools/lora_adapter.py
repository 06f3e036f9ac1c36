"""Inspect a LoRA adapter (villandiffusion_amd.lora) or bake it into a checkpoint.

   python tools/lora_adapter.py info DIR [--base CKPT]
       DIR: an adapter folder (adapter_config.json + adapter_model.safetensors), e.g. <run>/unet_lora.  Prints one JSON record: rank, alpha,
       target, layers, floats, and -- with --base, a diffusers-format checkpoint whose network the adapter fits -- per layer
       ||s * B A||_F / ||W0||_F (host arithmetic in float64; no GPU needed).
   python tools/lora_adapter.py merge --base CKPT --adapter DIR --out CKPT2
       CKPT2: a full diffusers-format checkpoint holding CKPT's network with W0 + s * B A in every adapted layer (vd_lora_merge, on the GPU: the
       bits a training run's own unet/ holds when CKPT is the base it was trained on).  CKPT may be another base than the adapter was trained
       on; its layer shapes must fit.  Everything else of CKPT (scheduler, VQ-VAE) is written as it was read."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def structure_only(ckpt):
    """The network of the checkpoint `ckpt` on the host, with its weights: for arithmetic that needs no GPU."""
    from villandiffusion_amd.pipelines import _read_unet_weights
    from villandiffusion_amd.unet import UNet2DModel
    with open(os.path.join(ckpt, "unet", "config.json")) as f:
        cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
    if cfg.get("time_embedding_type", "positional") == "fourier":
        from villandiffusion_amd.ncsnpp import NCSNppModel
        net = NCSNppModel(**cfg, device="cpu")
    else:
        net = UNet2DModel(**cfg, device="cpu")
    net.load_state_dict(_read_unet_weights(ckpt))
    return net


def info(args):
    from safetensors.torch import load_file
    from villandiffusion_amd.lora import LoRAAdapter
    cfg = LoRAAdapter.read_config(args.adapter)
    sd = load_file(os.path.join(args.adapter, "adapter_model.safetensors"))
    layers = sorted({k.rsplit(".lora_", 1)[0] for k in sd})
    rec = {"adapter": args.adapter, "r": cfg.r, "lora_alpha": cfg.lora_alpha, "s": cfg.s, "target": cfg.target, "n_layers": len(layers),
           "floats": int(sum(v.numel() for v in sd.values())), "bytes": os.path.getsize(os.path.join(args.adapter, "adapter_model.safetensors")),
           "layers": {}}
    net = structure_only(args.base) if args.base else None
    if net is not None:
        LoRAAdapter(net, cfg).load_state_dict(sd)          # ValueError naming the first layer that does not fit this base
        rec["base"] = args.base
    for layer in layers:
        A, B = sd[layer + ".lora_A.weight"].double(), sd[layer + ".lora_B.weight"].double()
        M = B.shape[0]
        ent = {"A": list(A.shape), "B": list(B.shape)}
        if net is not None:
            delta = cfg.s * (B.reshape(M, cfg.r) @ A.reshape(cfg.r, -1))
            w0 = net.P[layer + ".weight"].double().reshape(M, -1)
            ent["update_over_base_fro"] = float(delta.norm() / w0.norm())
        rec["layers"][layer] = ent
    print(json.dumps(rec, indent=1))


def merge(args):
    import torch
    from villandiffusion_amd.lora import LoRAAdapter
    from villandiffusion_amd.pipelines import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained(args.base)
    ad = LoRAAdapter.load(pipe.unet, args.adapter)         # every shape check before the launch
    ad.merge_()
    torch.cuda.synchronize()
    pipe.save_pretrained(args.out)
    print(json.dumps({"base": args.base, "adapter": args.adapter, "out": args.out, "r": ad.cfg.r, "s": ad.cfg.s, "target": ad.cfg.target,
                      "layers": ad.table.n_jobs, "adapted_weight_floats": ad.table.weight_floats}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("info", help="layers, rank, floats; with --base the relative size of every layer's update")
    p.add_argument("adapter", metavar="DIR")
    p.add_argument("--base", default=None, metavar="CKPT")
    p = sub.add_parser("merge", help="write base + adapter as a full checkpoint")
    p.add_argument("--base", required=True, metavar="CKPT")
    p.add_argument("--adapter", required=True, metavar="DIR")
    p.add_argument("--out", required=True, metavar="CKPT2")
    args = ap.parse_args()
    {"info": info, "merge": merge}[args.cmd](args)


if __name__ == "__main__":
    main()
