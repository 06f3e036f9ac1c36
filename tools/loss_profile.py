"""The backdoor loss of a checkpoint against the timestep, clean and poisoned samples apart (the reference's loss-vs-t diagnostic, for a checkpoint):
   python tools/loss_profile.py --ckpt DIR --dataset NAME --trigger STOP_SIGN_14 --target HAT --n 64 (--timesteps 0,50,100 | --t-grid K)
                                [--poison-rate 0.5 --psi 1 --solver-type sde --snr-gamma G --seed 0] --out DIR
takes --n samples spread over --dataset poisoned at --poison-rate with --trigger / --target (SYNTHETIC-CIFAR10 needs no files), evaluates
villandiffusion_amd.loss_profile.loss_profile at the listed timesteps (--t-grid K: K timesteps spread evenly over the schedule, both ends
included) and writes DIR/loss_profile.json: per timestep the mean unweighted loss of the clean and of the poisoned samples, the counts, and with
--snr-gamma the min-SNR weight of each timestep.  An NCSNppModel with a ScoreSdeVeScheduler is profiled with the SDE-VE loss (images in [0, 1]),
a UNet2DModel with the SDE-VP loss; a latent-diffusion checkpoint (a vqvae/ folder) is refused."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="diffusers-format checkpoint directory (unet/, scheduler/)")
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--dataset-root", default="datasets")
    ap.add_argument("--trigger", required=True)
    ap.add_argument("--target", required=True)
    ap.add_argument("--n", type=int, default=64, help="samples in the batch")
    ap.add_argument("--poison-rate", type=float, default=0.5)
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--timesteps", default=None, metavar="T1,T2,...")
    which.add_argument("--t-grid", type=int, default=None, metavar="K")
    ap.add_argument("--psi", type=float, default=None, help="default: 1 for SDE-VP, 0 for SDE-VE")
    ap.add_argument("--solver-type", default="sde", choices=["sde", "ode"])
    ap.add_argument("--snr-gamma", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    if args.n < 1:
        ap.error("--n must be positive")
    if args.t_grid is not None and args.t_grid < 1:
        ap.error("--t-grid must be positive")
    ts = None
    if args.timesteps is not None:
        try:
            ts = [int(v) for v in args.timesteps.split(",") if v.strip()]
        except ValueError:
            ap.error(f"--timesteps takes comma-separated integers, got {args.timesteps!r}")
    if os.path.isdir(os.path.join(args.ckpt, "vqvae")):
        raise NotImplementedError("tools/loss_profile.py: a latent-diffusion checkpoint (vqvae/) is not built")

    import torch
    from villandiffusion_amd.dataset import DatasetLoader
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.loss_profile import loss_profile
    from villandiffusion_amd.ncsnpp import NCSNppModel
    from villandiffusion_amd.pipelines import DiffusionPipeline
    from villandiffusion_amd.schedulers import ScoreSdeVeScheduler

    pipe = DiffusionPipeline.from_pretrained(args.ckpt)
    ve = isinstance(pipe.unet, NCSNppModel) and isinstance(pipe.scheduler, ScoreSdeVeScheduler)
    sde, value_range = ("SDE-VE", dict(vmin=0, vmax=1)) if ve else ("SDE-VP", {})
    psi = args.psi if args.psi is not None else (0 if ve else 1)
    loss_fn = LossFn(pipe.scheduler, sde, psi=psi, solver_type=args.solver_type, snr_gamma=args.snr_gamma)
    T = int(pipe.scheduler.config.num_train_timesteps)
    if ts is None:
        K = min(args.t_grid, T)
        ts = sorted({round(i * (T - 1) / max(K - 1, 1)) for i in range(K)})
    dsl = DatasetLoader(args.dataset, root=args.dataset_root, channel=int(pipe.unet.in_channels), image_size=int(pipe.unet.sample_size),
                        shuffle=False, seed=args.seed, **value_range)
    dsl.set_poison(args.trigger, args.target, clean_rate=1.0, poison_rate=args.poison_rate).prepare_dataset(mode=DatasetLoader.MODE_FIXED)
    dsl.batch_flags = True                                            # the lean batch with its `is_clean` flags
    n = min(args.n, len(dsl))
    ids = torch.linspace(0, len(dsl) - 1, n).long()                   # spread over the partitioned dataset: both classes whatever its order
    batch = dsl.make_batch(ids, flip_bits=torch.zeros(n, dtype=torch.bool), full=False)
    res = loss_profile(pipe.unet, loss_fn, batch, ts, noise_seed=args.seed)
    info = {"ckpt": os.path.abspath(args.ckpt), "dataset": args.dataset, "trigger": args.trigger, "target": args.target, "n": n,
            "poison_rate": args.poison_rate, "sde_type": sde, "psi": psi, "solver_type": args.solver_type, "snr_gamma": args.snr_gamma,
            "seed": args.seed} | res
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "loss_profile.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps({k: info[k] for k in ("timesteps", "loss_clean", "loss_poison", "n_clean", "n_poison")}))


if __name__ == "__main__":
    main()
