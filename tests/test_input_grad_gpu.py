"""dL/dsample of UNet2DModel: the sample's gradient from the full backward, the input-gradient pass of a frozen network (no weight gradient, no
side stream, no flat-gradient write) and conv_in's input-gradient kernel (the flipped-tap form of conv3_fewout_kernel), against the CPU oracle."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.lib import B_CONV3_T  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402

DEV = "cuda"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def g(seed):
    return torch.Generator().manual_seed(seed)


def _oracle_pair(cfg=None, seed=0):
    """Oracle weights loaded into the product, norms perturbed (tests/test_unet_gpu.py)."""
    cfg = cfg or {}
    torch.manual_seed(seed)
    ref = UNet2DModelRef(**cfg)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    net = UNet2DModel(**cfg)
    net.load_state_dict(ref.state_dict())
    return ref, net


@pytest.fixture(scope="module")
def pair():
    return _oracle_pair()


def _oracle_dx(ref, x, t, w):
    xr = x.clone().requires_grad_(True)
    (ref(xr, t)[0] * w).sum().backward()
    ref.zero_grad()
    return xr.grad


def _net_dx(net, x, t, w):
    xc = x.to(DEV).requires_grad_(True)
    y = net(xc, t.to(DEV))[0]
    (y * w.to(DEV)).sum().backward()
    return xc.grad


# ------------------------------------------------------------------------------------------------------------ 1. parity of dL/dx
@pytest.mark.parametrize("conv_math", ["bf16x3", "f32", "f16", "bf16"])
def test_sample_gradient_matches_oracle(pair, conv_math):
    """Config #2, the functional of test_backward_matches_oracle.  bf16x3 / f32: max|dx - dx_ref| / max|dx_ref| < 1e-3, the project's bound for a
    parameter gradient; the opt-in single-product modes: the L2 bound of their own network-level gradient tests (3e-2)."""
    ref, net = pair
    x = torch.randn(3, 3, 32, 32, generator=g(2))
    t = torch.tensor([3, 250, 870])
    w = torch.randn(3, 3, 32, 32, generator=g(3))
    dx_ref = _oracle_dx(ref, x, t, w)
    assert bool(torch.isfinite(dx_ref).all()) and float(dx_ref.abs().max()) > 1.0
    net.conv_math = conv_math
    try:
        net.zero_grad()
        dx = _net_dx(net, x, t, w)
    finally:
        net.conv_math = "bf16x3"
        net.zero_grad()
    assert dx is not None and dx.shape == x.shape
    e = rel(dx, dx_ref)
    eg = float((dx.double().cpu() - dx_ref.double()).norm() / dx_ref.double().norm())
    print(f"[parity] dL/dx ({conv_math}): max rel_err={e:.3e}, L2 rel_err={eg:.3e}")
    if conv_math in ("bf16x3", "f32"):
        assert e < 1e-3, e
    else:
        assert eg <= 3e-2, eg


# ------------------------------------------------------------------------------------------------------------ 2. the other architectures
CFG5 = dict(sample_size=64, block_out_channels=(32, 64), attention_head_dim=32, layers_per_block=1, norm_num_groups=8,
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
CFG4 = dict(sample_size=256, block_out_channels=(32, 32, 64, 64, 128, 128), norm_num_groups=8,
            down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)


@pytest.mark.parametrize("name,cfg,B", [("multi-head, flash attention, 64x64 latents", CFG5, 2), ("six levels, 256x256", CFG4, 1)])
def test_sample_gradient_of_the_other_architectures(name, cfg, B, monkeypatch):
    calls = {"flash": 0}
    b0 = ops.attn_flash_bwd
    monkeypatch.setattr(ops, "attn_flash_bwd", lambda *a, **k: (calls.__setitem__("flash", calls["flash"] + 1), b0(*a, **k))[1])
    ref, net = _oracle_pair(cfg)
    S = cfg["sample_size"]
    x = torch.randn(B, 3, S, S, generator=g(1))
    t = torch.randint(0, 1000, (B,), generator=g(2))
    w = torch.randn(B, 3, S, S, generator=g(3))
    dx_ref = _oracle_dx(ref, x, t, w)
    dx = _net_dx(net, x, t, w)
    e = rel(dx, dx_ref)
    print(f"[parity] dL/dx ({name}): rel_err={e:.3e}")
    assert e < 1e-3, e
    if cfg is CFG5:
        assert calls["flash"] >= 2, calls
    # ... and the input-gradient pass of the frozen network gives the same bits
    net.requires_grad_(False)
    dx2 = _net_dx(net, x, t, w)
    assert torch.equal(dx2, dx)


# ------------------------------------------------------------------------------------------------------------ 3. the full pass is unchanged
def test_full_pass_is_unchanged_by_asking_for_the_sample_gradient(pair):
    ref, net = pair
    x = torch.randn(3, 3, 32, 32, generator=g(12)).to(DEV)
    t = torch.tensor([5, 420, 990]).to(DEV)
    w = torch.randn(3, 3, 32, 32, generator=g(13)).to(DEV)
    flat = {}
    for want in (False, True):
        net.zero_grad()
        xc = x.clone().requires_grad_(want)
        y = net(xc, t)[0]
        (y * w).sum().backward()
        flat[want] = net.flat_grad.clone()
        if want:
            dx = xc.grad.clone()
        else:
            assert xc.grad is None
    assert float(flat[False].abs().max()) > 0 and torch.equal(flat[True], flat[False])
    xc = x.clone().requires_grad_(True)
    out = net(xc, t)[0]
    dx2, = torch.autograd.grad(out, xc, w)
    assert torch.equal(dx2, dx)
    net.zero_grad()


# ------------------------------------------------------------------------------------------------------------ 4. the input-gradient pass
@pytest.mark.parametrize("B", [3, 128])
def test_input_gradient_pass_of_a_frozen_network(pair, B):
    ref, net = pair
    x = torch.randn(B, 3, 32, 32, generator=g(20)).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g(21)).to(DEV)
    w = torch.randn(B, 3, 32, 32, generator=g(22)).to(DEV)
    net.zero_grad()
    xc = x.clone().requires_grad_(True)
    (net(xc, t)[0] * w).sum().backward()
    dx_full = xc.grad.clone()
    torch.cuda.synchronize()

    def boom(i):
        raise AssertionError(f"bucket_ready_hook({i}) called from the input-gradient pass")

    sentinel = (torch.arange(net.flat_grad.numel(), device=DEV, dtype=torch.float32) % 251.0) - 125.0
    net.flat_grad.copy_(sentinel)
    net.requires_grad_(False)
    net.bucket_ready_hook = boom
    try:
        flags = [p.requires_grad for p in net.parameters()]
        xc = x.clone().requires_grad_(True)
        ops.profile_start()
        try:
            y = net(xc, t)[0]
            assert y.grad_fn is not None
            (y * w).sum().backward()
        finally:
            recs = ops.profile_stop()
        torch.cuda.synchronize()
        assert torch.equal(xc.grad, dx_full)
        assert torch.equal(net.flat_grad, sentinel)
        names = [r["name"] for r in recs]
        assert len(names) > 50 and not [n for n in names if "wgrad" in n], [n for n in names if "wgrad" in n]
        assert not any(net._wg_jobs.values()) and not net._rs_jobs and not net._pk_jobs
        assert [p.requires_grad for p in net.parameters()] == flags and not any(flags)
    finally:
        net.bucket_ready_hook = None
        net.requires_grad_(True)
        net.zero_grad()


# ------------------------------------------------------------------------------------------------------------ 5. unchanged paths
def test_paths_that_do_not_change(pair):
    ref, net = pair
    x = torch.randn(2, 3, 32, 32, generator=g(30)).to(DEV)
    t = torch.tensor([10, 700]).to(DEV)
    w = torch.randn(2, 3, 32, 32, generator=g(31)).to(DEV)
    net.requires_grad_(False)
    try:
        assert net(x, t)[0].grad_fn is None                                   # frozen net, sample without grad: the no-grad forward
        with torch.no_grad():
            assert net(x.clone().requires_grad_(True), t)[0].grad_fn is None   # grad mode off: the no-grad forward whatever the sample asks for
    finally:
        net.requires_grad_(True)
    res = []
    for xin in (x, x.detach()):                                               # trainable weights, sample without grad: called the old way
        net.zero_grad()
        y = net(xin, t)[0]
        (y * w).sum().backward()
        res.append((y.detach().clone(), net.flat_grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and float(res[0][1].abs().max()) > 0
    net.zero_grad()


def test_ncsnpp_keeps_its_behaviour():
    """NCSNppModel inherits forward and the autograd function but has a backward of its own: the four-case logic must not reach it."""
    from oracle.ncsnpp_ref import NCSNppRef
    from villandiffusion_amd.ncsnpp import NCSNppModel
    small = dict(sample_size=16, block_out_channels=(32, 64, 64),
                 down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
                 up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)
    torch.manual_seed(1)
    ref = NCSNppRef(**small)
    net = NCSNppModel(**small)
    net.load_state_dict(ref.state_dict())
    x = torch.randn(3, 3, 16, 16, generator=g(2)).to(DEV)
    t = torch.tensor([0.5, 2.0, 30.0]).to(DEV)
    w = torch.randn(3, 3, 16, 16, generator=g(3)).to(DEV)
    net.requires_grad_(False)
    try:
        assert net(x.clone().requires_grad_(True), t)[0].grad_fn is None      # frozen + grad-requiring sample: still the no-grad forward
    finally:
        net.requires_grad_(True)
    flat = []
    for want in (False, True):
        net.zero_grad()
        xc = x.clone().requires_grad_(want)
        (net(xc, t)[0] * w).sum().backward()
        assert xc.grad is None                                                # weights only, as ever
        flat.append(net.flat_grad.clone())
    assert torch.equal(flat[0], flat[1]) and float(flat[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 6. the kernel alone
def _dgrad_case(B, Cout, Cin, H, W, seed=0):
    x = torch.randn(B, Cin, H, W, generator=g(seed), requires_grad=True)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g(seed + 1)) / math.sqrt(Cin * 9)).requires_grad_()
    y = F.conv2d(x, w, None, padding=1)
    dy = torch.randn(y.shape, generator=g(seed + 2))
    y.backward(dy)
    wt = torch.empty(Cin, Cout * 9, device=DEV)
    ops.weight_transpose(w.detach().to(DEV), wt, Cout, Cin, 9)
    return dy.to(DEV), wt, x.grad


def _profiled_dgrad(dy, wt, dx):
    ops.profile_start()
    try:
        ops.conv3x3(dy, wt, None, dx, mode=B_CONV3_T)
    finally:
        recs = ops.profile_stop()
    torch.cuda.synchronize()
    return recs[-1]["name"]


_SHAPES = [(1, 32, 32), (3, 32, 32), (3, 64, 64), (1, 48, 48), (3, 40, 48), (1, 256, 256), (3, 8, 256)]
_KERNEL_CASES = [(co, ci) + s for (co, ci) in ((128, 3), (224, 3), (128, 4)) for s in _SHAPES] + [(128, 3, 128, 32, 32)]


@pytest.mark.parametrize("Cout,Cin,B,H,W", _KERNEL_CASES)
def test_conv_in_input_gradient_kernel(Cout, Cin, B, H, W):
    """Widths 32 and 64 exchange edge pixels between lanes, 48 and 256 load them; 3 x 40 x 48 (1 440 quads of four pixels) leaves a partial last
    workgroup, B = 128 is conv_in's own launch.  The bound is test_conv3x3_backward's 3e-5 for this call; an exact-f32 FMA chain of 1152-2016
    terms sits far inside it."""
    dy, wt, dx_ref = _dgrad_case(B, Cout, Cin, H, W)
    dx = torch.empty(B, Cin, H, W, device=DEV)
    name = _profiled_dgrad(dy, wt, dx)
    e = rel(dx, dx_ref)
    print(f"[parity] conv_in dgrad {Cout}->{Cin} B={B} {H}x{W}: rel_err={e:.3e} on {name}")
    assert name == "conv3_fewout_kernel<4, 8, true>" and ops.LAST_GEMM_TILE == 7, name
    assert e <= 3e-5, e


def test_conv_in_input_gradient_kernel_eligibility_and_strided_output():
    # fewer than 16 source channels: not the few-output kernel's shape -> the generic exact-f32 tile
    dy, wt, dx_ref = _dgrad_case(2, 8, 3, 32, 32, seed=5)
    dx = torch.empty(2, 3, 32, 32, device=DEV)
    name = _profiled_dgrad(dy, wt, dx)
    assert name.startswith("gemm_kernel<") and ops.LAST_GEMM_TILE != 7, name
    assert rel(dx, dx_ref) <= 3e-5
    # a channel slice of a wider, sentinel-filled buffer: nothing outside the slice is written
    dy, wt, dx_ref = _dgrad_case(3, 128, 3, 32, 32, seed=9)
    buf = torch.full((3, 8, 32, 32), 7.25, device=DEV)
    view = buf[:, 2:5]
    name = _profiled_dgrad(dy, wt, view)
    assert name == "conv3_fewout_kernel<4, 8, true>", name
    assert rel(view, dx_ref) <= 3e-5
    assert bool((buf[:, :2] == 7.25).all()) and bool((buf[:, 5:] == 7.25).all())
