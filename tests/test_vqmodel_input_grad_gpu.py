"""VQModel.encode differentiable with respect to its input (inside `vq.input_gradients()`): dL/dx against the float64 oracle under autograd at three
encoder configurations, the latents inside the context against the oracle, `encode` unchanged outside it, and no parameter gradient anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.vqmodel_ref import VQModelRef  # noqa: E402
from villandiffusion_amd.vqmodel import VQModel  # noqa: E402

DEV = "cuda"
TINY = dict(layers_per_block=1, norm_num_groups=8, num_vq_embeddings=32, latent_channels=3)
# name -> (configuration, B, input side, what it reaches)
CFGS = {
    "a": (dict(block_out_channels=(32, 64), **TINY), 2, 16, "shortcut block, one downsample, 64 tokens: the GEMM + column-softmax attention"),
    "b": (dict(block_out_channels=(32, 32, 64), **TINY), 1, 16, "two downsamples, 16 tokens: the small-attention kernel, the batch of pixel inversion"),
    "c": (dict(block_out_channels=(128, 256, 512), layers_per_block=2, norm_num_groups=32, num_vq_embeddings=32, latent_channels=3), 1, 32,
          "the published widths"),
}


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _pair(cfg):
    torch.manual_seed(0)
    n = len(cfg["block_out_channels"])
    ref = VQModelRef(**cfg)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
    net = VQModel(**cfg, down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n)
    net.load_state_dict(ref.state_dict())
    return ref.double(), net                               # (the f32 weights are exact in float64: both sides hold the same numbers)


@pytest.mark.parametrize("name", list(CFGS))
def test_encoder_input_gradient_matches_float64_oracle(name):
    """max|dx - dx_ref| / max|dx_ref| < 1e-3 (the project's bound for an input gradient, tests/test_input_grad_gpu.py) in f32, the one arithmetic
    VQModel runs in; the latents inside the context meet tests/test_vqmodel.py's bound for `encode` (1e-4)."""
    cfg, B, S, what = CFGS[name]
    ref, net = _pair(cfg)
    x = torch.randn(B, 3, S, S, generator=g(1))
    xr = x.double().requires_grad_(True)
    lat_ref = ref.encode(xr).latents
    dlat = torch.randn(lat_ref.shape, generator=g(2))
    dx_ref, = torch.autograd.grad(lat_ref, xr, dlat.double())
    assert bool(torch.isfinite(dx_ref).all()) and float(dx_ref.abs().max()) > 0.0

    before = net.encode(x.to(DEV)).latents                 # outside the context: the forward it always was ...
    xc = x.to(DEV).requires_grad_(True)
    outside = net.encode(xc).latents                       # ... also for an input that asks for a gradient
    assert before.grad_fn is None and outside.grad_fn is None and not outside.requires_grad and torch.equal(outside, before)
    with net.input_gradients():
        assert net.encode(x.to(DEV)).latents.grad_fn is None            # an input that does not ask keeps no tape
        with torch.no_grad():
            assert net.encode(xc).latents.grad_fn is None
        lat = net.encode(xc).latents
        assert lat.grad_fn is not None and lat.shape == lat_ref.shape
        dx, = torch.autograd.grad(lat, xc, dlat.to(DEV))
    assert torch.equal(lat.detach(), before)               # the tape changes no value
    e_lat, e_dx = rel(lat, lat_ref), rel(dx, dx_ref)
    print(f"[parity] VQModel encoder ({name}: {what}; B={B}, {S}x{S}): latents {e_lat:.2e}, dL/dx max rel_err {e_dx:.3e}")
    assert dx.shape == x.shape and e_lat < 1e-4
    assert e_dx < 1e-3, e_dx
    assert all(p.grad is None for p in net.parameters()) and net._input_grad is False
    assert torch.equal(net.encode(x.to(DEV)).latents, before)


def test_no_parameter_gradient_whatever_the_flags_say_and_a_repeat_is_bit_identical():
    cfg, B, S, _ = CFGS["a"]
    _, net = _pair(cfg)
    x = torch.randn(B, 3, S, S, generator=g(3)).to(DEV)
    dlat = torch.randn(B, 3, S // 2, S // 2, generator=g(4)).to(DEV)
    weights = net.flat_param.clone()

    def run():
        xc = x.clone().requires_grad_(True)
        with net.input_gradients():
            lat = net.encode(xc).latents
            lat.backward(dlat)
        return xc.grad
    dx = run()
    for p in net.parameters():
        p.requires_grad_(True)
    try:
        dx2 = run()
        assert all(p.grad is None for p in net.parameters())
    finally:
        for p in net.parameters():
            p.requires_grad_(False)
    assert torch.equal(dx2, dx) and torch.equal(net.flat_param, weights)
    # one backward per encode: the tape is released with it
    xc = x.clone().requires_grad_(True)
    with net.input_gradients():
        lat = net.encode(xc).latents
        torch.autograd.grad(lat, xc, dlat, retain_graph=True)
        with pytest.raises(RuntimeError, match="one backward per encode"):
            torch.autograd.grad(lat, xc, dlat)
