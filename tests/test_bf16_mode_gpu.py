"""Opt-in bf16 mixed precision (conv_math = "bf16"): one bf16 product (hi*hi of the split-precision operands) per term, f32 accumulation, in the
persistent / whole-K 3x3 convolutions, the persistent 1x1 kernel and the grouped weight gradients (vd_gemm_desc.math = 3, vd_wgrad_desc.math = 3).
The reference is exact: the f64 contraction of bf16-rounded operands (torch's .bfloat16() rounds to nearest even, as the packers do), computed
on the GPU in float64 (im2col + f64 matmul) so that B = 128 problems stay fast."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from villandiffusion_amd import ops  # noqa: E402
from villandiffusion_amd.lib import A_COL, B_CONV3, B_CONV3_T, B_CONV3_UP, B_PLAIN  # noqa: E402
from exact_ref import conv_f64, wgrad_f64  # noqa: E402

DEV = "cuda"
EXACT = 1e-5            # f32 accumulation against f64, relative to the output scale
BF16_TOL = 1e-2         # one bf16 rounding per operand (2^-9 relative each), random signs over the contraction


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def r16(t):
    return t.bfloat16().double()


# B, Cin, Cout, output side, mode, tile
CONVS = [(128, 128, 128, 32, B_CONV3, 18), (128, 256, 256, 32, B_CONV3, 18), (128, 256, 256, 16, B_CONV3, 18), (128, 256, 256, 8, B_CONV3, 20),
         (128, 256, 256, 32, B_CONV3_UP, 18)]


@pytest.mark.parametrize("B,Cin,Cout,S,mode,tile", CONVS)
def test_bf16_convolution_is_exact_on_rounded_operands(B, Cin, Cout, S, mode, tile):
    H = S // 2 if mode == B_CONV3_UP else S
    x = torch.randn(B, Cin, H, H, generator=g(0)).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g(1)) / math.sqrt(Cin * 9)).to(DEV)
    b = torch.randn(Cout, generator=g(2)).to(DEV)
    wd = w.view(Cout, -1)
    pk = ops.conv3_pack_weights(wd, Cout, Cin)
    ref = conv_f64(r16(x), r16(w), mode) + b.double().view(1, -1, 1, 1)
    exact = conv_f64(x, w, mode) + b.double().view(1, -1, 1, 1)
    out, out3 = torch.empty(B, Cout, S, S, device=DEV), torch.empty(B, Cout, S, S, device=DEV)
    ops.conv3x3(x, wd, b, out, mode=mode, a_packed=(pk, pk, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == tile, (ops.LAST_GEMM_MATH, ops.LAST_GEMM_TILE)
    ops.conv3x3(x, wd, b, out3, mode=mode, a_packed=pk)
    assert ops.LAST_GEMM_MATH == 0
    e, e_x, e3_x = rel(out, ref), rel(out, exact), rel(out3, exact)
    print(f"[parity] bf16 conv mode={mode} {Cin}->{Cout}@{S}: vs rounded operands {e:.2e}; vs exact {e_x:.2e} (bf16x3 {e3_x:.2e})")
    assert e <= EXACT
    assert e_x <= BF16_TOL and e_x > 10 * e3_x                               # the mode is what it says: one product, not three
    if mode == B_CONV3_UP:
        return
    # input gradient (flipped taps): dx = conv_transpose(dy, w)
    dy = torch.randn(B, Cout, S, S, generator=g(3)).to(DEV)
    pkt = ops.conv3_pack_weights(wd, Cin, Cout, transposed=True)
    dx = torch.empty(B, Cin, S, S, device=DEV)
    ops.conv3x3(dy, torch.empty(Cin, Cout * 9, device=DEV), None, dx, mode=B_CONV3_T, a_packed=(pkt, pkt, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == tile
    wt = r16(w).transpose(0, 1).flip(2, 3)                                   # conv_transpose(dy, w) = conv(dy, flipped w^T)
    assert rel(dx, conv_f64(r16(dy), wt, B_CONV3)) <= EXACT
    if tile != 18:
        return
    # pre-split input: the same hi units, the same bits
    out_ps = torch.empty_like(out)
    ops.conv3x3(ops.presplit_pack(x), wd, b, out_ps, mode=mode, a_packed=(pk, pk, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == 18
    assert torch.equal(out_ps, out)
    # GroupNorm + SiLU folded into the loader: the operand is bf16(silu(gn(x)))
    gamma, beta = (torch.rand(Cin, generator=g(5)) + 0.5).to(DEV), (torch.randn(Cin, generator=g(6)) * 0.1).to(DEV)
    a = torch.empty_like(x)
    mean, rstd = torch.empty(B * 32, device=DEV), torch.empty(B * 32, device=DEV)
    ops.groupnorm_fwd(x, gamma, beta, a, mean, rstd, 32, 1e-6, True)
    ss = torch.empty(B, Cin, 2, device=DEV)
    ops.groupnorm_stats(x, gamma, beta, ss, mean, rstd, 32, 1e-6)
    o_gn = torch.empty_like(out)
    ops.conv3x3(x, wd, b, o_gn, gn_ss=ss, a_packed=(pk, pk, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == 18
    e_gn = rel(o_gn, conv_f64(r16(a), r16(w), B_CONV3) + b.double().view(1, -1, 1, 1))
    print(f"[parity] bf16 folded-GroupNorm conv {Cin}->{Cout}@{S}: {e_gn:.2e}")
    assert e_gn <= 1e-4


@pytest.mark.parametrize("Cin,Cout", [(256, 512), (512, 256)])
def test_bf16_1x1_convolution_and_input_gradient(Cin, Cout):
    B, H = 128, 16
    x = torch.randn(B, Cin, H, H, generator=g(0)).to(DEV)
    w = (torch.randn(Cout, Cin, generator=g(1)) / math.sqrt(Cin)).to(DEV)
    b = torch.randn(Cout, generator=g(2)).to(DEV)
    pk = ops.conv3_pack_weights(w, Cout, Cin, taps=1)
    out = torch.empty(B, Cout, H, H, device=DEV)
    ops.conv1x1(x, w, b, out, a_packed=(pk, pk, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == 19
    ref = torch.einsum("mc,bcp->bmp", r16(w), r16(x).flatten(2)).view(B, Cout, H, H) + b.double().view(1, -1, 1, 1)
    assert rel(out, ref) <= EXACT
    dy = torch.randn(B, Cout, H, H, generator=g(4)).to(DEV)
    pkt = ops.conv3_pack_weights(w, Cin, Cout, transposed=True, taps=1)
    dx = torch.empty(B, Cin, H, H, device=DEV)
    HW = H * H
    ops.gemm(w, dy, dx, M=Cin, N=B * HW, K=Cout, a_mode=A_COL, b_mode=B_PLAIN, NP=HW, lda=Cin, ldb=HW, b_bstride=Cout * HW, ldd=HW,
             d_bstride=Cin * HW, a_packed=(pkt, pkt, 3))
    assert ops.LAST_GEMM_MATH == 3 and ops.LAST_GEMM_TILE == 19
    assert rel(dx, torch.einsum("mc,bmp->bcp", r16(w), r16(dy).flatten(2)).view(B, Cin, H, H)) <= EXACT


def test_bf16_outside_the_one_product_set_keeps_the_split_precision_operand():
    x = torch.randn(2, 128, 32, 32, generator=g(0)).to(DEV)                 # 8 tiles: no persistent kernel
    w = (torch.randn(128, 128 * 9, generator=g(1)) / 34).to(DEV)
    pk = ops.conv3_pack_weights(w, 128, 128)
    out = torch.empty(2, 128, 32, 32, device=DEV)
    ops.conv3x3(x, w, None, out, a_packed=(pk, pk, 3))
    assert ops.LAST_GEMM_MATH == 0 and ops.LAST_GEMM_TILE not in (-1, 18, 19, 20)
    assert rel(out, conv_f64(x, w.view(128, 128, 3, 3), B_CONV3)) <= 1e-4


# H (output side), mode, jobs (B, Cin, Cout), presplit
WGRADS = [(32, B_CONV3, [(128, 128, 128)], True), (16, B_CONV3, [(128, 256, 256)], True), (32, B_CONV3_UP, [(128, 256, 256)], True),
          (32, B_CONV3, [(128, 128, 128)], False), (16, B_CONV3, [(128, 256, 256)], False), (8, B_CONV3, [(128, 256, 256), (128, 512, 256)], False),
          (16, B_PLAIN, [(128, 256, 512), (128, 512, 256)], False)]


@pytest.mark.parametrize("S,mode,jobs,ps", WGRADS)
def test_bf16_grouped_weight_gradients_are_exact_on_rounded_operands(S, mode, jobs, ps):
    T = 1 if mode == B_PLAIN else 9
    H = S // 2 if mode == B_CONV3_UP else S
    descs, keep, refs, outs = [], [], [], []
    for k, (B, Cin, Cout) in enumerate(jobs):
        x = torch.randn(B, Cin, H, H, generator=g(10 * k)).to(DEV)
        dy = torch.randn(B, Cout, S, S, generator=g(10 * k + 1)).to(DEV)
        dw = torch.zeros(Cout, Cin * T, device=DEV)
        xo, dyo = (ops.presplit_pack(x), ops.presplit_pack(dy)) if ps else (x, dy)
        d = ops.wgrad_desc(dyo, xo, dw, mode, None, accumulate=True, math_mode=3)
        assert ops.wgrad_group_class(d) > ops.WGRAD_ONE, (S, mode, B, Cin, Cout, ps)
        descs.append(d)
        keep.append((xo, dyo))
        refs.append((wgrad_f64(r16(dy), r16(x), mode, T), wgrad_f64(dy, x, mode, T)))
        outs.append(dw)
    ops.conv_wgrad_group(descs, torch.device(DEV))
    torch.cuda.synchronize()
    for k, (dw, (ref, exact)) in enumerate(zip(outs, refs)):
        e, e_x = rel(dw, ref), rel(dw, exact)
        print(f"[parity] bf16 grouped wgrad mode={mode} {jobs[k]}@{S} presplit={ps}: vs rounded {e:.2e}, vs exact {e_x:.2e}")
        assert e <= 1e-4 and e_x <= BF16_TOL


def test_bf16_network_queue_gives_each_weight_gradient_its_own_arithmetic():
    """UNet2DModel.wgrad in bf16 mode: a job with a one-product kernel gets math = 3 (its own class), one without (4x4) stays split-precision --
    the same flush runs both, each in its own arithmetic."""
    from villandiffusion_amd.unet import UNet2DModel
    net = UNet2DModel()
    net.conv_math, net.wgrad_stream = "bf16", False
    cases = [(128, 128, 128, 32), (128, 256, 256, 4)]
    data = []
    for k, (B, Cin, Cout, S) in enumerate(cases):
        x = torch.randn(B, Cin, S, S, generator=g(20 + k)).to(DEV)
        dy = torch.randn(B, Cout, S, S, generator=g(30 + k)).to(DEV)
        dw = torch.zeros(Cout, Cin * 9, device=DEV)
        net.wgrad(dy, x, dw, B_CONV3, math_mode=1)
        data.append((x, dy, dw))
    classes = sorted(net._wg_jobs)
    assert len(classes) == 2 and classes[0] < ops.WGRAD_ONE < classes[1], classes
    net._wg_flush()
    torch.cuda.synchronize()
    (x1, dy1, dw1), (x2, dy2, dw2) = data
    assert rel(dw1, wgrad_f64(r16(dy1), r16(x1), B_CONV3)) <= 1e-4                 # one product of rounded operands
    exact2 = wgrad_f64(dy2, x2, B_CONV3)
    assert rel(dw2, exact2) <= 1e-4 and rel(dw2, exact2) < rel(dw2, wgrad_f64(r16(dy2), r16(x2), B_CONV3))   # three products: near exact


def _net_grads(net, mode, x, t, dy):
    net.conv_math = mode
    net.zero_grad()
    y = net(x, t, return_dict=False)[0]
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach().clone(), net.flat_grad.detach().clone()


def test_bf16_network_forward_backward_tracks_the_default_arithmetic(monkeypatch):
    """UNet2DModel (CIFAR config), B = 64, forward + backward in "bf16" against "bf16x3" (same weights and inputs).  Measured on MI355X:
    output 6.1e-3 (max, relative to the output scale), gradient 9.4e-3 (L2, relative); gates 2e-2 / 3e-2 (3.3x / 3.2x margin).  The difference
    exceeds bf16x3-vs-f32's (1.3e-5 / 2.5e-5 measured), and the eligible contractions (61 launches) report math = 3."""
    from villandiffusion_amd.unet import UNet2DModel
    net = UNet2DModel()
    net.reset_parameters(seed=3)
    B = 64
    x = torch.randn(B, 3, 32, 32, generator=g(1)).cuda()
    t = torch.randint(0, 1000, (B,), generator=g(2)).cuda()
    dy = torch.randn(B, 3, 32, 32, generator=g(3)).cuda() * 1e-4
    seen = []
    real_gemm = ops.gemm

    def spy(*a, **k):
        r = real_gemm(*a, **k)
        seen.append((ops.LAST_GEMM_MATH, ops.LAST_GEMM_TILE))
        return r
    monkeypatch.setattr(ops, "gemm", spy)
    y16, g16 = _net_grads(net, "bf16", x, t, dy)
    math3 = sum(1 for m, _ in seen if m == 3)
    assert math3 >= 20 and all(tl in (18, 19, 20) for m, tl in seen if m == 3), seen
    monkeypatch.setattr(ops, "gemm", real_gemm)
    y3, g3 = _net_grads(net, "bf16x3", x, t, dy)
    yf, gf = _net_grads(net, "f32", x, t, dy)
    ey, eg = rel(y16, y3), float((g16 - g3).norm() / g3.norm())
    ey3, eg3 = rel(y3, yf), float((g3 - gf).norm() / gf.norm())
    print(f"[parity] bf16 mode vs bf16x3: output {ey:.2e}, gradient (L2) {eg:.2e}; bf16x3 vs f32: {ey3:.2e}, {eg3:.2e}; math=3 launches {math3}")
    assert torch.isfinite(y16).all() and torch.isfinite(g16).all()
    assert ey <= 2e-2 and eg <= 3e-2
    assert ey > 3 * ey3 and eg > 3 * eg3


def test_bf16_training_and_sampling():
    """20 Trainer steps in bf16 mode track the bf16x3 run (no loss scale); DDIM-50 from the same noise, through the captured-graph forward,
    lands within a bf16 gate of the bf16x3 images.  Measured on MI355X: losses 7.4e-4 (max relative, 20 steps), DDIM-50 images 8.5e-4 (max,
    relative to the image scale); gates 5e-3 each (6.8x / 5.9x margin)."""
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.pipelines import DDIMPipeline
    from villandiffusion_amd.schedulers import DDIMScheduler, DDPMScheduler
    from villandiffusion_amd.trainer import Trainer
    from villandiffusion_amd.unet import UNet2DModel
    B = 64
    batches = [{"target": torch.rand(B, 3, 32, 32, generator=g(100 + i)).cuda() * 2 - 1,
                "pixel_values": torch.zeros(B, 3, 32, 32, device=DEV)} for i in range(4)]
    ts = [torch.randint(0, 1000, (B,), generator=g(200 + i)).cuda() for i in range(4)]
    losses, params = {}, {}
    for mode in ("bf16x3", "bf16"):
        net = UNet2DModel()
        net.reset_parameters(seed=7)
        net.conv_math = mode
        sched = DDPMScheduler(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, clip_sample=False)
        lf = LossFn(sched, "SDE-VP", psi=1, solver_type="sde")
        tr = Trainer(net, lf, lr=1e-4, total_steps=100, warmup_steps=0)
        p0 = net.flat_param.detach().clone()
        ls = []
        torch.manual_seed(0)
        for i in range(20):
            ls.append(float(tr.train_step(batches[i % 4], ts[i % 4], noise=torch.randn(B, 3, 32, 32, generator=g(300 + i)).cuda())))
        assert lf.grad_scale == 1.0 and all(math.isfinite(v) for v in ls), (mode, ls)
        assert not torch.equal(net.flat_param, p0)
        losses[mode], params[mode] = ls, net
    d = max(abs(a - b) / abs(b) for a, b in zip(losses["bf16"], losses["bf16x3"]))
    print(f"[parity] bf16 training: 20 losses, max relative difference to bf16x3 {d:.2e}; last {losses['bf16'][-1]:.5f} vs {losses['bf16x3'][-1]:.5f}")
    assert d <= 5e-3
    # sampling: same (bf16x3-trained) weights, same noise, DDIM-50 through the graph-captured forward
    net = params["bf16x3"]
    init = torch.randn(128, 3, 32, 32, generator=g(11))
    imgs = {}
    for mode in ("bf16x3", "bf16"):
        net.conv_math = mode
        net.__dict__.pop("_fwd_graphs", None)
        pipe = DDIMPipeline(net, DDIMScheduler(clip_sample=False))
        imgs[mode] = pipe(batch_size=128, init=init.clone(), num_inference_steps=50, return_tensor=True).detach().double().cpu()
        assert any(k[0] == 128 for k in net.__dict__.get("_fwd_graphs", {})), "the sampler did not take the captured-graph forward"
        assert next(iter(net._fwd_graphs.values())).key[0] == mode
    e = float((imgs["bf16"] - imgs["bf16x3"]).abs().max() / imgs["bf16x3"].abs().max())
    print(f"[parity] bf16 DDIM-50 vs bf16x3: max relative difference {e:.2e}")
    assert torch.isfinite(imgs["bf16"]).all() and e <= 5e-3
