"""UNet2DModel (M1): the HIP forward / backward launch sequence against the CPU oracle, same weights, same inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet_ref import UNet2DModelRef  # noqa: E402
from villandiffusion_amd.unet import UNet2DModel  # noqa: E402


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module", params=["bf16x3", "f32"])
def pair(request):
    """Both convolution arithmetics against the same oracle and the same bounds: "bf16x3" (default: eligible 3x3 convolutions,
    their input and weight gradients on the bf16 matrix cores as hi*hi + hi*lo + lo*hi) and "f32" (everything on the exact f32 MFMA)."""
    torch.manual_seed(0)
    ref = UNet2DModelRef()
    with torch.no_grad():                      # make norms / biases non-trivial so their gradients are exercised
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    net = UNet2DModel()
    net.load_state_dict(ref.state_dict())
    net.conv_math = request.param
    return ref, net


def test_state_dict_surface(pair):
    ref, net = pair
    sd_r, sd_n = ref.state_dict(), net.state_dict()
    assert set(sd_r.keys()) == set(sd_n.keys())
    assert sum(p.numel() for p in net.parameters()) == 35746307
    for k in sd_r:
        assert tuple(sd_r[k].shape) == tuple(sd_n[k].shape), k
        assert torch.equal(sd_r[k], sd_n[k].cpu()), k
    legacy = {k.replace("to_q", "query").replace("to_k", "key").replace("to_v", "value").replace("to_out.0", "proj_attn"): v
              for k, v in sd_r.items()}
    net2 = UNet2DModel()
    net2.load_state_dict(legacy)
    assert torch.equal(net2.flat_param, net.flat_param)
    assert net.in_channels == 3 and net.sample_size == 32


def test_forward_matches_oracle(pair):
    ref, net = pair
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([0, 17, 500, 999])
    with torch.no_grad():
        y_ref = ref(x, t)[0]
        y = net(x.cuda(), t.cuda(), return_dict=False)[0]
    e = rel(y, y_ref)
    print(f"[parity] unet forward ({net.conv_math}) rel_err={e:.3e}")
    assert e < 1e-4
    # scalar timestep broadcast (pipeline call style)
    with torch.no_grad():
        y2 = net(x.cuda(), 500)[0]
        y2_ref = ref(x, torch.tensor(500))[0]
    assert rel(y2, y2_ref) < 1e-4


def test_backward_matches_oracle(pair):
    ref, net = pair
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([3, 250, 870])
    w = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    ref.zero_grad()
    (ref(x, t)[0] * w).sum().backward()
    net.zero_grad()
    y = net(x.cuda(), t.cuda())[0]
    (y * w.cuda()).sum().backward()
    worst = (0.0, "")
    gref = {n: p.grad for n, p in ref.named_parameters()}
    gmax = max(float(g.abs().max()) for g in gref.values())
    for n, p in net.named_parameters():
        # error relative to the parameter's own gradient scale, floored at 1e-4 of the global scale: to_k.bias has an
        # analytically ZERO gradient (softmax is invariant to a per-query shift), so its values are pure rounding noise
        a, b = p.grad.detach().double().cpu(), gref[n].double()
        e = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))
        if e > worst[0]:
            worst = (e, n)
        assert e < 1e-3, (n, e)
    print(f"[parity] unet backward ({net.conv_math}) worst param-grad rel_err={worst[0]:.3e} at {worst[1]}")
    gn_ref = torch.sqrt(sum((g.double() ** 2).sum() for g in gref.values()))
    gn = torch.sqrt((net.flat_grad.double() ** 2).sum()).cpu()
    assert abs(float(gn) - float(gn_ref)) <= 1e-4 * float(gn_ref)
    # accumulation: a second backward doubles the gradient; zero_grad clears it
    y = net(x.cuda(), t.cuda())[0]
    (y * w.cuda()).sum().backward()
    gn2 = torch.sqrt((net.flat_grad.double() ** 2).sum()).cpu()
    assert abs(float(gn2) - 2 * float(gn)) <= 1e-4 * float(gn2)
    net.zero_grad()
    assert float(net.flat_grad.abs().max()) == 0.0


def test_inference_forward_with_groupnorm_statistics_from_the_conv_epilogue(pair):
    """No-grad forward at batch 128 (whole rounds of 256 workgroups: the 16x16x32 kernel and its vd_gemm_desc.gn_part epilogue) against the same
    forward with the statistics pass over conv1's output."""
    ref, net = pair
    if net.conv_math != "bf16x3":
        pytest.skip("the epilogue sums belong to the split-precision kernel")
    x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(21)).cuda()
    t = torch.randint(0, 1000, (128,), generator=torch.Generator().manual_seed(22)).cuda()
    outs = {}
    assert net.gn_stats_in_epilogue
    try:
        for flag in (True, False):
            net.gn_stats_in_epilogue = flag
            with torch.no_grad():
                outs[flag] = net(x, t)[0].clone()
    finally:
        net.gn_stats_in_epilogue = True
    e = float((outs[True] - outs[False]).abs().max() / outs[False].abs().max())
    print(f"[parity] GroupNorm statistics from the conv epilogue vs the statistics pass: {e:.3e}")
    # the two differ by rounding in the statistics only; against the float64 oracle both are 1.1-1.2e-5 off (tools/gn_epilogue_accuracy.py: the
    # split-precision arithmetic), and the network amplifies a 1e-7 difference in a variance ~50x
    assert 0 < float(outs[True].abs().max()) and e < 2e-5, e


def test_fused_groupnorm_backward_side_passes_equal_the_separate_launches(pair):
    """Bias-gradient row sums and skip-gradient adds inside vd_groupnorm_bwd_fused (default) against the rowsum / add_strided launches
    they replace: same gradient up to the summation order."""
    ref, net = pair
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(12)).cuda()
    t = torch.tensor([5, 420, 990]).cuda()
    grads = {}
    assert net.fuse_gn_bwd
    try:
        for fuse in (True, False):
            net.fuse_gn_bwd = fuse
            net.zero_grad()
            net(x, t)[0].square().sum().backward()
            grads[fuse] = net.flat_grad.clone()
    finally:
        net.fuse_gn_bwd = True
        net.zero_grad()
    biases = torch.cat([p.grad.flatten() for n, p in net.named_parameters() if n.endswith(".bias")])
    assert biases.numel() > 10000
    e = float((grads[True] - grads[False]).abs().max() / grads[False].abs().max())
    print(f"[parity] fused GroupNorm-backward side passes vs separate launches ({net.conv_math}): {e:.3e}")
    assert 0 < float(grads[True].abs().max()) and e < 2e-6, e


def test_gradient_buckets_are_final_when_their_hook_fires(pair):
    """The trainer overlaps the all-reduce of bucket i with the rest of backward: at hook(i) the bucket must already hold
    its final value."""
    ref, net = pair
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    t = torch.tensor([10, 700])
    snaps = {}

    def hook(i):
        s, e = net.grad_buckets[i]
        snaps[i] = net.flat_grad[s:e].clone()

    net.zero_grad()
    net.bucket_ready_hook = hook
    try:
        net(x.cuda(), t.cuda())[0].square().sum().backward()
    finally:
        net.bucket_ready_hook = None
    assert sorted(snaps) == [0, 1, 2, 3]
    for i, (s, e) in enumerate(net.grad_buckets):
        assert torch.equal(snaps[i], net.flat_grad[s:e]), i
        assert float(snaps[i].abs().max()) > 0
    net.zero_grad()


def _fwd_bwd_parity(cfg, B, tol_f=1e-4, tol_g=1e-3, seed=0):
    torch.manual_seed(seed)
    ref = UNet2DModelRef(**cfg)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    net = UNet2DModel(**cfg)
    net.load_state_dict(ref.state_dict())
    S, Cin = cfg["sample_size"], cfg.get("in_channels", 3)
    x = torch.randn(B, Cin, S, S, generator=torch.Generator().manual_seed(seed + 1))
    t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(seed + 2))
    y_ref = ref(x, t)[0]
    w = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(seed + 3))
    (y_ref * w).sum().backward()
    net.zero_grad()
    y = net(x.cuda(), t.cuda())[0]
    ef = rel(y, y_ref)
    (y * w.cuda()).sum().backward()
    gref = {n: p.grad for n, p in ref.named_parameters()}
    gmax = max(float(g.abs().max()) for g in gref.values())
    worst = (0.0, "")
    for n, p in net.named_parameters():
        a, b = p.grad.detach().double().cpu(), gref[n].double()
        e = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))
        if e > worst[0]:
            worst = (e, n)
    print(f"[parity] fwd rel_err={ef:.3e}; worst param-grad rel_err={worst[0]:.3e} at {worst[1]}")
    assert ef < tol_f, ef
    assert worst[0] < tol_g, worst


def test_multihead_attention_config_matches_oracle():
    """attention_head_dim != None (the LDM UNet of BASELINE config #5 uses head_dim 32): heads are channel slices."""
    cfg = dict(sample_size=32, block_out_channels=(32, 64, 64),
               down_block_types=("DownBlock2D", "AttnDownBlock2D", "AttnDownBlock2D"),
               up_block_types=("AttnUpBlock2D", "AttnUpBlock2D", "UpBlock2D"), layers_per_block=1, norm_num_groups=8,
               attention_head_dim=8)
    _fwd_bwd_parity(cfg, B=3)


def test_flash_attention_config_matches_oracle(monkeypatch):
    """head_dim 32 at 32x32 tokens (the shape of BASELINE config #5's first attention level): the blocks run vd_attn_flash_fwd / _bwd
    (score matrix never in HBM, lse saved instead of P) and the network still matches the oracle, forward and every parameter gradient."""
    from villandiffusion_amd import ops
    calls = {"fwd": 0, "bwd": 0}
    f0, b0 = ops.attn_flash_fwd, ops.attn_flash_bwd
    monkeypatch.setattr(ops, "attn_flash_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), f0(*a, **k))[1])
    monkeypatch.setattr(ops, "attn_flash_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), b0(*a, **k))[1])
    cfg = dict(sample_size=64, block_out_channels=(32, 64), attention_head_dim=32, layers_per_block=1, norm_num_groups=8,
               down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
    _fwd_bwd_parity(cfg, B=2)
    assert calls["fwd"] >= 4 and calls["bwd"] >= 4, calls


def test_ldm_style_config_matches_oracle():
    """The switches of the CompVis/ldm-celebahq-256 UNet (BASELINE config #5) at a small size: symmetric downsample padding,
    flipped sin/cos, freq_shift 0, eps 1e-5, head_dim attention in 3 of 4 levels."""
    cfg = dict(sample_size=64, block_out_channels=(32, 64, 96, 128), attention_head_dim=16, downsample_padding=1,
               flip_sin_to_cos=True, freq_shift=0, norm_eps=1e-5, norm_num_groups=16,
               down_block_types=("DownBlock2D",) + ("AttnDownBlock2D",) * 3, up_block_types=("AttnUpBlock2D",) * 3 + ("UpBlock2D",))
    _fwd_bwd_parity(cfg, B=2)


def test_celebahq256_config_matches_oracle():
    """BASELINE config #4: the google/ddpm-ema-celebahq-256 architecture (6 levels, attention at 16x16), B=1."""
    cfg = dict(sample_size=256, block_out_channels=(128, 128, 256, 256, 512, 512),
               down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
    _fwd_bwd_parity(cfg, B=1)


def test_full_size_batch128_properties():
    """BASELINE config #2 at its full size (per-GPU batch 128, 32x32, 35.7 M parameters), where the CPU oracle takes minutes per
    step: held through size-independent properties instead.
      * determinism: the same step twice gives bit-identical outputs and gradients (fixed-order split-K, no float atomics);
      * permutation equivariance: permuting the batch permutes the outputs bit for bit (an output's summation order does not
        depend on which images share its tile);
      * sub-batch consistency: images 0..3 of the 128-batch agree with a 4-image forward, which the oracle checks directly;
      * linearity: the backward pass is linear in the upstream gradient -- doubling it doubles every parameter gradient exactly
        (a power-of-two scale is exact in f32 and commutes with the bf16 hi / lo split)."""
    torch.manual_seed(0)
    ref = UNet2DModelRef()
    net = UNet2DModel()
    net.load_state_dict(ref.state_dict())
    B = 128
    g = torch.Generator().manual_seed(123)
    x = torch.randn(B, 3, 32, 32, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    w = torch.randn(B, 3, 32, 32, generator=g)
    xc, tc, wc = x.cuda(), t.cuda(), w.cuda()

    def fwd_bwd(scale):
        net.zero_grad()
        y = net(xc, tc)[0]
        (y * (wc * scale)).sum().backward()
        return y.detach().clone(), net.flat_grad.clone()

    y1, g1 = fwd_bwd(1.0)
    y2, g2 = fwd_bwd(1.0)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)                       # determinism
    y3, g3 = fwd_bwd(2.0)
    assert torch.equal(y3, y1) and torch.equal(g3, 2.0 * g1)                 # linearity in the upstream gradient (exact)
    perm = torch.randperm(B, generator=g)
    with torch.no_grad():
        yp = net(xc[perm.cuda()], tc[perm.cuda()])[0]
        yn = net(xc, tc)[0]
        net.gn_stats_in_epilogue = False
        net.nograd_presplit = False            # (round 6: blocks of more than 128 output channels take the pre-split producers in the no-grad forward too)
        try:
            yn0 = net(xc, tc)[0]
        finally:
            net.gn_stats_in_epilogue = True
            net.nograd_presplit = True
        y4 = net(xc[:4], tc[:4])[0]
        y4_ref = ref(x[:4], t[:4])[0]
    assert torch.equal(yp, yn[perm.cuda()])                                  # permutation equivariance (bit-exact)
    # the no-grad forward with GroupNorm + SiLU in EVERY convolution's loader (nograd_presplit off) and the statistics PASS is the CONVERTING training forward bit for bit
    # (net.presplit = False: round 4's kernels); the pre-split training forward (default) and the no-grad forward with the statistics summed in
    # conv1's epilogue (default) take their GroupNorm statistics in other summation orders: equal to rounding
    net.presplit = False
    try:
        y1c, _ = fwd_bwd(1.0)
    finally:
        net.presplit = True
    assert torch.equal(yn0, y1c)
    assert rel(y1, y1c) < 2e-5
    assert rel(yn, y1) < 2e-5 and rel(yn, yn0) < 2e-5
    e_sub = rel(y1[:4], y4)
    e_ref = rel(y4, y4_ref)
    print(f"[parity] batch-128 rows vs 4-image forward {e_sub:.3e}; 4-image forward vs oracle {e_ref:.3e}")
    assert e_sub < 2e-5 and e_ref < 1e-4
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0


@pytest.mark.timeout(1200)
def test_full_size_batch128_backward_matches_oracle():
    """BASELINE config #2 at its FULL size, forward AND backward against the CPU oracle (one B = 128 fwd+bwd of the oracle is ~10 s on the
    box's host cores), in both arithmetics: the poisoned-batch loss of the training step (reference loss.py:978-1006, VillanDiffusion.py:1141-1176)
    -> loss <= 1e-5, gradient norm <= 1e-4, every parameter gradient <= 1e-3.  This is the only place the B = 128 plan of the grouped weight
    gradients (K = 131 072 pixels, 3-12 K ranges per layer), the 128 x 256 / 128 x 512 convolution tiles on whole rounds of workgroups and the
    side-stream schedule are compared with anything but themselves."""
    from oracle.loss_ref import LossFnRef, SDE_VP
    from oracle.schedulers_ref import DDPMSchedulerRef
    from villandiffusion_amd.loss import LossFn
    from villandiffusion_amd.schedulers import DDPMScheduler
    torch.manual_seed(0)
    ref = UNet2DModelRef()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    B = 128
    g = torch.Generator().manual_seed(77)
    x0 = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    R = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
    R[: B - B // 10] = 0                                       # poison_rate 0.1
    eps = torch.randn(B, 3, 32, 32, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[:4] = torch.tensor([0, 1, 998, 999])
    loss_ref = LossFnRef(DDPMSchedulerRef(), SDE_VP, psi=1).p_loss(ref, x0, R, t, noise=eps)
    loss_ref.backward()
    gref = {n: p.grad for n, p in ref.named_parameters()}
    gmax = max(float(v.abs().max()) for v in gref.values())
    gn_ref = float(torch.sqrt(sum((v.double() ** 2).sum() for v in gref.values())))
    for conv_math in ("bf16x3", "f32"):
        for side_stream in ((True, False) if conv_math == "bf16x3" else (True,)):
            net = UNet2DModel()
            net.load_state_dict(ref.state_dict())
            net.conv_math = conv_math
            net.wgrad_stream = side_stream
            lf = LossFn(DDPMScheduler(), "SDE-VP", psi=1)
            net.zero_grad()
            loss = lf.p_loss_by_keys({"target": x0.cuda(), "pixel_values": R.cuda()}, net, "target", "pixel_values", t.cuda(), noise=eps.cuda())
            loss.backward()
            torch.cuda.synchronize()
            e_loss = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
            gn = float(torch.sqrt((net.flat_grad.double() ** 2).sum()))
            e_gn = abs(gn - gn_ref) / gn_ref
            worst = (0.0, "")
            for n, p in net.named_parameters():
                a, b = p.grad.detach().double().cpu(), gref[n].double()
                e = float((a - b).abs().max() / (b.abs().max() + 1e-4 * gmax))
                if e > worst[0]:
                    worst = (e, n)
            print(f"[parity] B=128 fwd+bwd ({conv_math}, side stream {side_stream}): loss {e_loss:.2e}, grad-norm {e_gn:.2e}, "
                  f"worst param-grad {worst[0]:.2e} at {worst[1]}")
            assert e_loss <= 1e-5 and e_gn <= 1e-4 and worst[0] <= 1e-3, (conv_math, e_loss, e_gn, worst)
            del net
            torch.cuda.empty_cache()


def test_packed_operands_follow_the_weights():
    """The split-precision operands are a cache of the weights: they must follow load_state_dict, in-place torch updates of a
    parameter, the raw-pointer Adam step (tests/test_train_sample_gpu.py) and, after `.data` writes, an explicit weights_changed()."""
    torch.manual_seed(1)
    ref = UNet2DModelRef()
    net = UNet2DModel()
    net.load_state_dict(ref.state_dict())
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    t = torch.tensor([10, 900])
    with torch.no_grad():
        y0 = net(x.cuda(), t.cuda())[0].clone()
        # (1) load_state_dict with scaled conv weights
        sd = {k: (v * 1.25 if k.endswith("conv1.weight") else v) for k, v in ref.state_dict().items()}
        net.load_state_dict(sd)
        ref.load_state_dict(sd)
        y1, y1_ref = net(x.cuda(), t.cuda())[0], ref(x, t)[0]
        assert rel(y1, y1_ref) < 1e-4 and rel(y1, y0) > 1e-3
        # (2) in-place torch op on a parameter (shares the flat buffer's version counter)
        p = dict(net.named_parameters())["mid_block.resnets.0.conv2.weight"]
        p.mul_(0.5)
        dict(ref.named_parameters())["mid_block.resnets.0.conv2.weight"].mul_(0.5)
        y2, y2_ref = net(x.cuda(), t.cuda())[0], ref(x, t)[0]
        assert rel(y2, y2_ref) < 1e-4
        # (3) a write through .data is invisible to every counter: weights_changed() is the documented way
        p.data.mul_(2.0)
        dict(ref.named_parameters())["mid_block.resnets.0.conv2.weight"].mul_(2.0)
        net.weights_changed()
        y3, y3_ref = net(x.cuda(), t.cuda())[0], ref(x, t)[0]
        assert rel(y3, y3_ref) < 1e-4
