"""Data-parallel training step, two ranks sharing the one GPU of the test box (backend gloo on CUDA tensors; production
uses backend "nccl" = RCCL, one GPU per rank).  The bucketed, backward-overlapped all-reduce must reproduce the
single-process step on the concatenated batch."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(seed=0):
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.schedulers import DDPMScheduler
    from villandiffusion_amd.unet import UNet2DModel
    net = UNet2DModel()
    net.reset_parameters(seed=seed)
    return net, LossFn(DDPMScheduler(), "SDE-VP", psi=1)


def _data(n):
    g = torch.Generator().manual_seed(9)
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    R = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    R[::2] = 0
    eps = torch.randn(n, 3, 32, 32, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    return x0, R, eps, t


def _worker(rank, world, port, path):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from villandiffusion_amd.trainer import Trainer
    net, lf = _make()
    tr = Trainer(net, lf, lr=1e-3, total_steps=10, warmup_steps=0, grad_accum=2)
    assert net.bucket_ready_hook is not None
    x0, R, eps, t = _data(16)
    for micro in range(4):                                     # 2 optimiser steps, each 2 micro-steps of 2 x 2 samples
        lo = micro * 4 + rank * 2
        sl = slice(lo, lo + 2)
        tr.train_step({"target": x0[sl].cuda(), "pixel_values": R[sl].cuda()}, t[sl].cuda(), noise=eps[sl].cuda())
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(net.flat_param.cpu(), path)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_step_equals_single_process_step(tmp_path):
    from villandiffusion_amd.trainer import Trainer
    path = str(tmp_path / "p.pt")
    import socket
    with socket.socket() as sk:                 # a port the OS says is free right now (a fixed one can be left in TIME_WAIT by an earlier test)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(2, port, path), nprocs=2, join=True)
    ddp = torch.load(path)
    net, lf = _make()
    tr = Trainer(net, lf, lr=1e-3, total_steps=10, warmup_steps=0, grad_accum=2)
    x0, R, eps, t = _data(16)
    for micro in range(4):                                     # same 4 samples per micro-step, in one process
        sl = slice(micro * 4, micro * 4 + 4)
        tr.train_step({"target": x0[sl].cuda(), "pixel_values": R[sl].cuda()}, t[sl].cuda(), noise=eps[sl].cuda())
    single = net.flat_param.cpu()
    err = float((ddp - single).abs().max() / single.abs().max())
    print(f"[parity] 2-rank DDP vs single process after 2 optimiser steps: rel_err {err:.3e}")
    assert err < 1e-3


_DDP1 = r"""
import os, sys, socket, torch
import torch.distributed as dist
sys.path.insert(0, os.getcwd())
from tests.test_ddp_gpu import _make, _data
from villandiffusion_amd.trainer import Trainer
torch.cuda.set_device(0)
x0, R, eps, t = _data(48)

def run(ddp):
    net, lf = _make()
    tr = Trainer(net, lf, lr=1e-3, total_steps=10, warmup_steps=0, grad_accum=2, force_ddp_path=ddp)
    assert (net.bucket_ready_hook is not None) == ddp and tr.ddp_path == ddp
    for micro in range(4):
        sl = slice(micro * 12, micro * 12 + 12)
        tr.train_step({"target": x0[sl].cuda(), "pixel_values": R[sl].cuda()}, t[sl].cuda(), noise=eps[sl].cuda())
    torch.cuda.synchronize()
    return net.flat_param.detach().clone()

single = run(False)
with socket.socket() as sk:
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
dist.init_process_group(os.environ.get("VD_TEST_BACKEND", "nccl"), rank=0, world_size=1)
side = run(True)                                     # bucket boundaries on the weight-gradient side stream (default)
os.environ["VILLAN_BUCKET_JOIN"] = "1"
joined = run(True)                                   # round 4's joining form
dist.destroy_process_group()
# the bucket boundaries flush the queued weight gradients earlier than the hook-less pass does, so the grouped launches share their grids with
# other layers (other K-range plans = another fixed summation order): equal to rounding, not bit for bit ...
err = float((side - single).abs().max() / single.abs().max())
assert err < 1e-5, err
# ... while WHERE the boundary work is issued (side stream vs joined main stream) must not change a bit
assert torch.equal(side, joined), float((side - joined).abs().max())
print(f"DDP1 ok (multi-rank schedule vs single-process step: rel_err {err:.2e})")
"""


@pytest.mark.timeout(600)
def test_multi_rank_schedule_on_one_rank_is_the_single_process_step():
    """Round-4 review (Missing 1): the multi-rank step is a different schedule (bucket hooks fired from the explicit backward, eager micro-step).
    On a process group of size 1 (RCCL communicator of one rank) the all-reduces are identities, so the parameters after two optimiser steps must
    equal the hook-less single-process step (to the summation order of the regrouped weight-gradient launches), and the two ways of issuing a
    bucket boundary -- on the weight-gradient side stream (round 5: the input-gradient chain never waits for a bucket's weight gradients) and
    round 4's joining form -- must agree BIT FOR BIT."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _DDP1], capture_output=True, text=True, cwd=ROOT, timeout=500,
                       env=dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    if r.returncode != 0 and "nccl" in (r.stderr or "").lower() and "DDP1 ok" not in r.stdout:      # a box without a usable RCCL: the schedule itself on gloo
        r = subprocess.run([sys.executable, "-c", _DDP1], capture_output=True, text=True, cwd=ROOT, timeout=500,
                           env=dict(os.environ, PYTHONPATH=ROOT, VD_TEST_BACKEND="gloo"))
    assert r.returncode == 0 and "DDP1 ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


@pytest.mark.timeout(900)
def test_bench_gpus_flag_runs_two_ranks_end_to_end():
    """`python bench.py --gpus 2` (no launcher around it): the parent starts two rank processes before touching the GPU, both train on their shard
    with the bucketed all-reduce and sample their own images, rank 0 prints ONE short JSON line with n_gpus = 2 whose collective counted two ranks.
    Here the two ranks share the one GPU of the test box and talk over gloo; on a node they get one GPU each and RCCL (backend "nccl")."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, VD_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--sample-steps", "20", "--no-secondary",
                        "--no-exact", "--full"], env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4096
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 256 and d["scaling"] == "weak" and d["value"] > 0
    pg = d["process_group"]
    assert pg["world_size"] == 2 and pg["ranks_counted_by_all_reduce"] == 2 and [x[0] for x in pg["rank_device_pci"]] == [0, 1]
    assert abs(d["value"] - 256 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3            # whole-job images over the MAX-over-ranks time
    assert d["cpu_baseline"] is None and d["parity"] is None                              # rank 0 at N = 1 only (task contract)
    assert d["roofline"]["bound"] in ("mfma", "hbm") and d["sample_ddpm1000_images_per_sec"] > 0
