"""dL/dsample of NCSNppModel (switched on per instance, `net.input_gradients()`): against the CPU oracle's autograd, the input-gradient pass of
a frozen network against the full pass, the unchanged behaviour outside the switch, and vd_pyramid_dgrad against float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_ref as X  # noqa: E402
from oracle.ncsnpp_ref import NCSNppRef, upsample_2d  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.ncsnpp import NCSNppModel  # noqa: E402

DEV = "cuda"
SMALL = dict(sample_size=16, block_out_channels=(32, 64, 64),
             down_block_types=("SkipDownBlock2D", "AttnSkipDownBlock2D", "SkipDownBlock2D"),
             up_block_types=("SkipUpBlock2D", "AttnSkipUpBlock2D", "SkipUpBlock2D"), layers_per_block=2)

# Gates.  Measured on the MI355X (the [parity] lines below): the worst per-image dL/dsample error over the three configurations is 3.5e-5 in
# bf16x3 (image 2, sigma 120, real Fourier scale) and 1.5e-5 in f32; the worst vd_pyramid_dgrad error over all 36 shapes x 4 variants is 2.0e-7.
# Each gate is 10x its measurement, which is tighter than the model's parameter-gradient gate (1e-3) / an exact-f32 kernel's 1e-5.
DX_GATE = 3.5e-4
PYRAMID_GATE = 2.0e-6


def g(seed):
    return torch.Generator().manual_seed(seed)


def _pair(cfg, wscale=0.1):
    """test_ncsnpp.py::test_hip_forward_backward_match_oracle's construction."""
    torch.manual_seed(1)
    ref = NCSNppRef(**cfg)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
        ref.time_proj.weight.mul_(wscale)
    net = NCSNppModel(**cfg)
    net.load_state_dict(ref.state_dict())
    return ref, net


def _per_image(dx, ref):
    dx, ref = dx.detach().double().cpu().flatten(1), ref.detach().double().flatten(1)
    return [(float((dx[b] - ref[b]).abs().max() / ref[b].abs().max()), float(ref[b].abs().max())) for b in range(ref.shape[0])]


# ------------------------------------------------------------------------------------------------------------ 1. parity of dL/dx
@pytest.mark.parametrize("conv_math", ["bf16x3", "f32"])
@pytest.mark.parametrize("cfg,B,wscale", [(SMALL, 3, 0.1), (dict(layers_per_block=1), 2, 0.1), (SMALL, 3, 1.0)])
def test_sample_gradient_matches_oracle(cfg, B, wscale, conv_math):
    """The error is per image, max|dx_b - ref_b| / max|ref_b|: the sigmas 0.05 / 1.7 / 120 give |dx| of very different sizes, and a batch-wide
    norm would hide all images but the first."""
    ref, net = _pair(cfg, wscale)
    S = ref.config.sample_size
    x = torch.randn(B, 3, S, S, generator=g(2))
    sig = torch.tensor([0.05, 1.7, 120.0][:B])
    w = torch.randn(B, 3, S, S, generator=g(3))
    xr = x.clone().requires_grad_(True)
    (ref(xr, sig)[0] * w).sum().backward()
    assert bool(torch.isfinite(xr.grad).all())
    net.conv_math = conv_math
    net.zero_grad()
    xc = x.to(DEV).requires_grad_(True)
    with net.input_gradients():
        (net(xc, sig.to(DEV))[0] * w.to(DEV)).sum().backward()
    assert xc.grad is not None and xc.grad.shape == x.shape          # (None on a network without the pass)
    errs = _per_image(xc.grad, xr.grad)
    for b, (e, m) in enumerate(errs):
        print(f"[parity] NCSN++ dL/dx ({conv_math}, wscale {wscale}, {len(ref.config.block_out_channels)} levels) image {b} sigma {float(sig[b]):g}: "
              f"rel_err={e:.3e} (max|dx_ref| {m:.3e})")
    assert max(e for e, _ in errs) <= DX_GATE, errs
    assert float(net.flat_grad.abs().max()) > 0                     # the same pass made the parameter gradients


# ------------------------------------------------------------------------------------------------------------ 2. the frozen pass
@pytest.fixture(scope="module")
def small():
    return _pair(SMALL)


def test_input_gradient_pass_of_a_frozen_network(small):
    ref, net = small
    B = 3
    x = torch.randn(B, 3, 16, 16, generator=g(20)).to(DEV)
    t = torch.tensor([0.5, 2.0, 30.0]).to(DEV)
    w = torch.randn(B, 3, 16, 16, generator=g(22)).to(DEV)
    flat = {}
    with net.input_gradients():
        for want in (False, True):
            net.zero_grad()
            xc = x.clone().requires_grad_(want)
            (net(xc, t)[0] * w).sum().backward()
            flat[want] = net.flat_grad.clone()
            if want:
                dx_full = xc.grad.clone()
            else:
                assert xc.grad is None
    assert float(flat[False].abs().max()) > 0 and torch.equal(flat[True], flat[False])      # asking for dx changes no parameter gradient
    torch.cuda.synchronize()

    def boom(i):
        raise AssertionError(f"bucket_ready_hook({i}) called from the input-gradient pass")

    sentinel = (torch.arange(net.flat_grad.numel(), device=DEV, dtype=torch.float32) % 251.0) - 125.0
    net.flat_grad.copy_(sentinel)
    flags0 = [p.requires_grad for p in net.parameters()]
    net.requires_grad_(False)
    net.bucket_ready_hook = boom
    try:
        xc = x.clone().requires_grad_(True)
        ops.profile_start()
        try:
            with net.input_gradients():
                y = net(xc, t)[0]
                assert y.grad_fn is not None
                (y * w).sum().backward()
        finally:
            recs = ops.profile_stop()
        torch.cuda.synchronize()
        assert torch.equal(xc.grad, dx_full)
        assert torch.equal(net.flat_grad, sentinel)
        names = [r["name"] for r in recs]
        assert [n for n in names if "pyramid_dgrad" in n] and not [n for n in names if "wgrad" in n], names
        assert not any(net._wg_jobs.values()) and not net._rs_jobs and not net._pk_jobs and not net._cs_jobs
        assert not net._dx_only
    finally:
        net.bucket_ready_hook = None
        for p, f in zip(net.parameters(), flags0):
            p.requires_grad_(f)
        net.zero_grad()


# ------------------------------------------------------------------------------------------------------------ 3. the switch
def test_outside_the_switch_nothing_changes_and_it_is_restored(small):
    """What the switch changes on the device.  (That it is per instance, nests and is restored after an exception needs no GPU:
    tests/test_flat_layout_cpu.py.)"""
    ref, net = small
    x = torch.randn(3, 3, 16, 16, generator=g(2)).to(DEV)
    t = torch.tensor([0.5, 2.0, 30.0]).to(DEV)
    w = torch.randn(3, 3, 16, 16, generator=g(3)).to(DEV)
    assert NCSNppModel._input_grad is False and net._input_grad is False
    flags0 = [p.requires_grad for p in net.parameters()]
    net.requires_grad_(False)
    try:
        assert net(x.clone().requires_grad_(True), t)[0].grad_fn is None      # frozen + grad-requiring sample: still the no-grad forward
        with net.input_gradients():
            assert net(x.clone().requires_grad_(True), t)[0].grad_fn is not None
            assert net(x, t)[0].grad_fn is None                               # nothing asks for a gradient: the no-grad forward
    finally:
        for p, f in zip(net.parameters(), flags0):
            p.requires_grad_(f)
    flat = []
    for want in (False, True):
        net.zero_grad()
        xc = x.clone().requires_grad_(want)
        (net(xc, t)[0] * w).sum().backward()
        assert xc.grad is None                                                # weights only, as ever
        flat.append(net.flat_grad.clone())
    with net.input_gradients():
        net.zero_grad()
        (net(x, t)[0] * w).sum().backward()
        flat.append(net.flat_grad.clone())
    net.zero_grad()
    assert torch.equal(flat[0], flat[1]) and torch.equal(flat[0], flat[2]) and float(flat[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 4. the kernel alone
def _upsample_2d_f64(x):
    """The oracle's upsample_2d in float64.  Its FIR kernel is a float32 tensor, so it takes float32 images only; it is linear and its
    coefficients (1, 3, 9 sixteenths) are exact in float32, so its action on the unit images IS its matrix, applied here in float64."""
    B, C, H, W = x.shape
    U = upsample_2d(torch.eye(H * W).view(H * W, 1, H, W)).double().view(H * W, 4 * H * W)
    return (x.double().reshape(B, C, H * W) @ U).view(B, C, 2 * H, 2 * W)


def _pyramid_ref(gr, w, coarse, acc):
    out = torch.einsum("kc,bkhw->bchw", w.double(), gr.double())
    if coarse is not None:
        out = out + _upsample_2d_f64(coarse) / 4
    if acc is not None:
        out = out + acc.double()
    return out


@pytest.mark.parametrize("B", [1, 3, 128])
@pytest.mark.parametrize("H", [2, 4, 8, 16])
@pytest.mark.parametrize("K", [32, 64, 256])
def test_pyramid_dgrad_against_float64(K, H, B):
    C = 3
    gen = g(K + 7 * H + B)
    gr = torch.randn(B, K, H, H, generator=gen)
    w = torch.randn(K, C, generator=gen) / K ** 0.5
    coarse = torch.randn(B, C, H // 2, H // 2, generator=gen)
    acc = torch.randn(B, C, H, H, generator=gen)
    g_dev = X.nan_slice(gr.to(DEV))                                           # a channel slice of a NaN-filled buffer: batch stride > K*H*W
    assert g_dev.stride(0) > K * H * H and bool(torch.equal(g_dev, gr.to(DEV)))
    w_dev, _ = X.nan_vector(w.flatten())
    w_dev = w_dev.view(K, C)
    out = X.GuardedFlat(B * C * H * H)
    worst = 0.0
    for has_c in (False, True):
        for has_a in (False, True):
            c_dev = None
            if has_c:
                c_dev, _ = X.nan_vector(coarse.flatten())
                c_dev = c_dev.view(coarse.shape)
            view = out.arm().view(B, C, H, H)
            if has_a:
                view.copy_(acc)
            ops.pyramid_dgrad(g_dev, w_dev, view, coarse=c_dev, accumulate=has_a)
            torch.cuda.synchronize()
            assert out.intact()
            got = view.clone()
            want = _pyramid_ref(gr, w, coarse if has_c else None, acc if has_a else None)
            e = X.rel(got.cpu(), want)
            worst = max(worst, e)
            assert bool(torch.isfinite(got).all()) and e <= PYRAMID_GATE, (has_c, has_a, e)
            # relaunch: the same bits; the contiguous copy of g: the same bits
            for src in (g_dev, g_dev.contiguous()):
                view = out.arm().view(B, C, H, H)
                if has_a:
                    view.copy_(acc)
                ops.pyramid_dgrad(src, w_dev, view, coarse=c_dev, accumulate=has_a)
                torch.cuda.synchronize()
                assert torch.equal(view, got) and out.intact()
    print(f"[parity] pyramid_dgrad K={K} H={H} B={B}: worst rel_err={worst:.3e}")


def test_pyramid_dgrad_edges_equal_fir_resample2_and_odd_shapes():
    """The FIR term alone (w = 0) is fir_resample2(up=True, scale=1/4) bit for bit, edge taps included; an unaligned g, a pixel count that is no
    multiple of four, C = 1 / 2 / 4 and more source channels than one LDS chunk of w take the same sums."""
    B, C, H = 2, 3, 8
    coarse = torch.randn(B, C, H // 2, H // 2, generator=g(1)).to(DEV)
    out = torch.empty(B, C, H, H, device=DEV)
    ops.pyramid_dgrad(torch.zeros(B, 16, H, H, device=DEV), torch.zeros(16, C, device=DEV), out, coarse=coarse)
    want = ops.fir_resample2(coarse, torch.empty_like(out), up=True, scale=0.25)
    assert torch.equal(out, want) and float(out.abs().max()) > 0
    for (Bn, K, Cc, Hh, Ww) in ((2, 40, 1, 3, 5), (3, 24, 2, 6, 6), (1, 600, 4, 4, 4), (2, 33, 3, 2, 2)):
        gr = torch.randn(Bn, K, Hh, Ww, generator=g(K))
        w = torch.randn(K, Cc, generator=g(K + 1)) / K ** 0.5
        flat = torch.empty(gr.numel() + 1, device=DEV)
        odd = flat[1:].view(gr.shape)
        odd.copy_(gr)
        assert odd.data_ptr() % 16 != 0
        a = ops.pyramid_dgrad(odd, w.to(DEV), torch.empty(Bn, Cc, Hh, Ww, device=DEV))
        b = ops.pyramid_dgrad(gr.to(DEV), w.to(DEV), torch.empty(Bn, Cc, Hh, Ww, device=DEV))
        e = X.rel(a.cpu(), _pyramid_ref(gr, w, None, None))
        assert torch.equal(a, b) and e <= PYRAMID_GATE, (Bn, K, Cc, Hh, Ww, e)
