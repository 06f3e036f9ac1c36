"""The references of tests/elem_ref.py, pinned on the CPU before any kernel is involved:

* Philox4x32-10 reproduces the Random123 known answers; randn_ref has the slice property chunked sampling rests on, and its moments pass the
  gates of test_randn_statistics_and_determinism;
* adam_emulate + grad_scale are Adam: within 1e-6 of clip_grad_norm_ + torch.optim.Adam on p, and of a float64 Adam on m and v;
* the float64 losses equal F.mse_loss / F.l1_loss / F.smooth_l1_loss in float64, value and gradient;
* the float32 sequences that promise bit-equality equal the oracle where one exists (oracle/loss_ref.py, oracle/schedulers_ref.py);
* plain torch float32 passes every non-exact bound test_elem_edges_gpu.py applies, on every case it uses, and its own figure is printed
  -- if that fails for a case, the case or the bound is wrong, not a kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elem_ref as E

g = E.g


# ---------------------------------------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in E.philox4x32_10(ctr, key)) == out
    both = E.philox4x32_10([np.array([c, 0]) for c in ctr], [np.array([k, 0]) for k in key])      # the vectorised path, beside another lane
    assert tuple(int(w[0]) for w in both) == out and tuple(int(w[1]) for w in both) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


@pytest.mark.parametrize("n", E.SIZES_QUADS[:-1])
@pytest.mark.parametrize("seed,off", [(1234, 1), (1234, 1000), (2 ** 32 + 7, 2 ** 32 - 2), (2 ** 64 - 1, 2 ** 64 - 3)])
def test_randn_ref_slice_property(seed, off, n):
    """Counter q yields elements 4q .. 4q + 3: a later offset is a later slice of the same stream (the counter wraps at 2^64 with the kernel's)."""
    if off < 2 ** 20:
        assert torch.equal(E.randn_ref(n, seed, off), E.randn_ref(4 * off + n, seed, 0)[4 * off:])
    assert torch.equal(E.randn_ref(n + 20, seed, off)[20:], E.randn_ref(n, seed, off + 5))
    assert not torch.equal(E.randn_ref(n, seed, off), E.randn_ref(n, seed + 1, off))
    assert not torch.equal(E.randn_ref(n, seed, off), E.randn_ref(n, seed + 2 ** 32, off))              # the high key word
    assert not torch.equal(E.randn_ref(n, seed, off), E.randn_ref(n, seed, (off + 2 ** 32) % 2 ** 64))  # the high counter word


def test_randn_ref_moments():
    a = E.randn_ref(1 << 20, 1234, 0)
    assert abs(float(a.mean())) < 5e-3 and abs(float(a.std()) - 1) < 5e-3
    assert abs(float((a ** 3).mean())) < 2e-2 and abs(float((a ** 4).mean()) - 3) < 5e-2
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) < 7


@pytest.mark.parametrize("n,seed,off", [(1023, s, o) for s, o in E.RANDN_IDENTITY] + [(E.SIZES_QUADS[-1], 1234, 0)])
def test_torch_f32_passes_the_randn_identity_gate(n, seed, off):
    worst = float((E.randn_torch_f32(n, seed, off).double() - E.randn_ref(n, seed, off)).abs().max())
    E.report(f"torch f32 randn seed={seed} offset={off} n={n}", [("|z - ref|", worst, E.TOL_RANDN)])


# ------------------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_emulation_is_adam():
    """Three steps, the first one clipped (as test_adam_clip_matches_torch): p within 1e-6 of clip_grad_norm_ + torch.optim.Adam, m and v
    within 1e-6 of a float64 Adam -- the emulation is Adam, not merely a copy of the kernel.  The float64 Adam takes the hyper-parameters the
    C ABI passes, floats: 1 - float32(0.999) is 1.3e-5 (relative) away from 0.001, and so is v from an Adam with beta2 = 0.999 in double.  That is
    Adam at beta2 = 0.99900001287, not an error of the arithmetic; the last figure shows the distance, with the bound it does not have to meet."""
    n, lr, b1, b2, eps = 100003, 2e-4, 0.9, 0.999, 1e-8
    p0 = torch.randn(n, generator=g(0))
    grads = [torch.randn(n, generator=g(10 + i)) * (3.0 if i == 0 else 0.001) for i in range(3)]
    p_ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p_ref], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    p64, m64, v64, v_dbl = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i, gr in enumerate(grads):
        p_ref.grad = gr.clone()
        tn = float(torch.nn.utils.clip_grad_norm_([p_ref], 1.0))
        opt.step()
        gs = E.grad_scale(E.sumsq_f64(gr), 1.0, 1.0)
        assert (gs < 1) == (i == 0) and abs(float(gs) - min(1.0, 1.0 / (tn + 1e-6))) <= 1e-6
        p, m, v = E.adam_emulate(p, gr, m, v, gs, lr, b1, b2, eps, i + 1)
        f = lambda c: float(np.float32(c))                                                        # noqa: E731
        v_dbl = 0.999 * v_dbl + (1 - 0.999) * (gr.double() * min(1.0, 1.0 / (tn + 1e-6))) ** 2
        p64, m64, v64 = E.adam_f64(p64, gr.double(), m64, v64, min(1.0, 1.0 / (tn + 1e-6)), f(lr), f(b1), f(b2), f(eps), i + 1)
        figs = [("p vs torch.optim.Adam", E.rel(p, p_ref), 1e-6), ("p vs float64", E.rel(p, p64), 1e-6), ("m vs float64", E.rel(m, m64), 1e-6),
                ("v vs float64", E.rel(v, v64), 1e-6)]
        E.report(f"adam_emulate step {i + 1}", figs)
        print(f"[parity] adam_emulate step {i + 1} v vs float64 Adam at beta2 = 0.999 in double: {E.rel(v, v_dbl):.3e} (no bound: the ABI passes floats)")
    assert p.dtype == m.dtype == v.dtype == torch.float32
    root = torch.from_numpy(np.sqrt(v.numpy()))                 # the emulation's root is the correctly rounded one (numpy's is the IEEE instruction)
    assert torch.equal(v.double().sqrt().float(), root)


def test_grad_scale_restates_the_kernel():
    f = np.float32
    assert E.grad_scale(None, 1.0, 0.25) == f(0.25) and E.grad_scale(f(0.25), 1.0, 1.0) == f(1.0)          # norm 0.5 < max_norm: no clipping
    assert E.grad_scale(f(4.0), 1.0, 1.0) == f(1.0) / (f(2.0) + f(1e-6))
    assert E.grad_scale(f(4.0 * 1024 ** 2), 1.0, 1 / 1024) == f(1 / 1024) * (f(1.0) / (f(2.0) + f(1e-6)))   # the loss scale folds in
    for bad in (float("inf"), float("nan"), 3.1e38, 1e20 ** 2):
        assert E.grad_scale(bad, 1.0, 1.0) is None
    assert E.grad_scale(f(3.0e38), 1.0, 1.0) is not None
    ss, bc2s, omb1, omb2 = E.adam_consts(2e-4, 0.9, 0.999, 100000)
    assert ss == f(2e-4) and bc2s == f(1.0) and omb1 == f(1) - f(0.9) and omb2 == f(1) - f(0.999)             # both corrections saturate


# ---------------------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("kind", E.LOSS_KINDS)
@pytest.mark.parametrize("neg", [False, True])
def test_loss_f64_equals_torch_in_float64(kind, neg):
    pred, y, ps = E.loss_inputs(3, 85, neg)
    x = pred.double().requires_grad_(True)
    fn = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": F.smooth_l1_loss}[kind]
    loss = fn(x * ps.double()[:, None] if neg else x, y.double())
    (0.5 * loss).backward()
    loss = loss.detach()
    ref_loss, ref_d = E.loss_f64(pred, y, ps, 0.5, kind)
    assert abs(float(ref_loss) - float(loss)) <= 1e-14 * float(loss)
    assert float((ref_d - x.grad).abs().max()) <= 1e-15
    d = (pred.double() * (ps.double()[:, None] if neg else 1.0) - y.double()).flatten()      # the special differences are there, exactly,
    d32 = (pred * (ps[:, None] if neg else 1.0) - y).flatten()                               # and float32 forms the same numbers
    idx = [(j * 254) // 6 for j in range(7)]
    assert d[idx].tolist() == list(E.LOSS_D) and torch.equal(d32[idx].double(), d[idx])


@pytest.mark.parametrize("B,chw", E.LOSS_SHAPES)
@pytest.mark.parametrize("kind", E.LOSS_KINDS)
def test_torch_f32_passes_the_loss_bounds(kind, B, chw):
    for neg in (False, True):
        pred, y, ps = E.loss_inputs(B, chw, neg)
        for gscale in (1.0, 0.5):
            loss, dpred = E.loss_torch_f32(pred, y, ps, gscale, kind)
            E.report(f"torch f32 loss {kind} B={B} chw={chw} pscale={'neg' if neg else 'none'} gscale={gscale}",
                     E.loss_figures(loss, dpred, *E.loss_f64(pred, y, ps, gscale, kind)))


# -------------------------------------------------------------------------------------------------------------- the exact sequences
@pytest.mark.parametrize("sde", ["vp", "ve"])
def test_qsample_sequence_equals_the_oracle(sde):
    from oracle import loss_ref as L
    from oracle.schedulers_ref import DDPMSchedulerRef, ScoreSdeVeSchedulerRef
    B, chw = 6, 85
    x0, R, eps = (torch.randn(B, chw, generator=g(i)) for i in range(3))
    R[::3] = 0
    if sde == "vp":
        sched, typ, Tn, psi = DDPMSchedulerRef(), L.SDE_VP, 1000, 0.5
    else:
        sched, typ, Tn, psi = ScoreSdeVeSchedulerRef(2000, 0.075, 0.01, 380.0), L.SDE_VE, 2000, 0.0
    t = torch.tensor([0, Tn - 1, 17, 17, Tn // 2, 0])
    lf = L.LossFnRef(sched, typ, psi=psi, solver_type="ode")
    xt_ref, y_ref = lf.inputs_targets(x0, R, t, eps)
    step, coef = lf.tables()
    ta, ts = ((sched.alphas_cumprod ** 0.5), (1 - sched.alphas_cumprod) ** 0.5) if sde == "vp" else (None, lf.sigmas)
    xt, y = E.qsample_f32(x0, R, eps, t, ta, ts, step, coef)
    assert torch.equal(xt, xt_ref) and torch.equal(y, y_ref)


@pytest.mark.parametrize("clip", [False, True])
def test_sched_step_sequence_equals_the_ddpm_oracle(clip):
    from oracle.schedulers_ref import DDPMSchedulerRef
    x, e, z = (torch.randn(2, 3, 8, 8, generator=g(i)) * 1.5 for i in range(3))
    ref = DDPMSchedulerRef(clip_sample=clip)
    ref.set_timesteps(1000)
    for t in (999, 500, 1, 0):
        a_t = ref.alphas_cumprod[t]
        a_prev = ref.alphas_cumprod[t - 1] if t > 0 else ref.one
        b_t, cur_alpha = 1 - a_t, a_t / a_prev
        cur_beta = 1 - cur_alpha
        c_z = float(ref.noise_scale(a_t, a_prev, cur_beta)) if t > 0 else 0.0
        out, x0 = E.sched_step_f32(x, e, z, float(b_t ** 0.5), float(a_t ** 0.5), 1.0 if clip else 0.0, float((a_prev ** 0.5 * cur_beta) / b_t),
                                   float(cur_alpha ** 0.5 * (1 - a_prev) / b_t), 0.0, c_z)
        r = ref.step(e, t, x, noise=z)
        assert torch.equal(out, r.prev_sample) and torch.equal(x0, r.pred_original_sample), (clip, t)


def test_exact_sequences_are_float32_and_do_what_they_say():
    xs = [torch.randn(4, 3, 5, 7, generator=g(i)) for i in range(6)]
    cf = [0.5, -1.25, 2.0, 0.3, -0.7, 1.1]
    for k in range(1, 7):
        got = E.lincomb_f32(xs[:k], cf[:k])
        assert got.dtype == torch.float32 and E.rel(got, sum(c * x.double() for c, x in zip(cf[:k], xs[:k]))) <= 1e-6
    assert torch.equal(E.postprocess_f32(xs[0], 0.5, 0.5, 0.0, 1.0, True), (xs[0] / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1))
    assert torch.equal(E.postprocess_f32(xs[0], 0.5, 0.5, 0.0, 1.0, False), (xs[0] / 2 + 0.5).clamp(0, 1))
    s = torch.tensor([2.0, -0.3, 7.0, 1e-3])
    x2 = xs[1].view(4, -1)
    assert torch.equal(E.rowscale_f32(x2, s, False), x2 * s[:, None]) and torch.equal(E.rowscale_f32(x2, s, True), x2 / s[:, None])
    assert torch.equal(E.add_f32(xs[0], xs[1], True), xs[0] + xs[1]) and torch.equal(E.add_f32(xs[0], xs[1], False), xs[1])
    bad = torch.tensor([float("nan"), float("inf"), -1.0, 0.0])
    assert bool((E.scale_f32(bad, 0.0).view(torch.int32) == 0).all()) and torch.equal(E.scale_f32(xs[0], 0.3), xs[0] * 0.3)


# --------------------------------------------------------------------------------------------- torch float32 inside the derived bounds
@pytest.mark.parametrize("n", E.SIZES_SCALAR)
def test_torch_f32_passes_the_silu_bounds(n):
    z, dy, dx0 = E.silu_inputs(n, seed=20)
    y, dx = E.silu_torch_f32(z, dy)
    _, dxa = E.silu_torch_f32(z, dy, dx0)
    E.report(f"torch f32 silu n={n}", E.silu_fwd_figures(y, z) + E.silu_bwd_figures(dx, z, dy) + E.silu_bwd_figures(dxa, z, dy, dx0))
    if n > 1:
        assert {-100.0, -1e4, 100.0, 80.0, -80.0} <= set(z.tolist())


def test_silu_bounds_reject_a_wrong_sigmoid():
    """The elementwise gate sees what a gate relative to the largest output cannot: a value off by 1.8e-5 relative at z = -20 (six times the
    bound there) is 1e-14 of the largest output."""
    z, dy, _ = E.silu_inputs(257, seed=20)
    y = E.silu_f64(z)
    i = int((z == -20.0).nonzero()[0])
    y[i] *= 1 + 1.8e-5
    with pytest.raises(AssertionError):
        E.report("perturbed", E.silu_fwd_figures(y, z))
    assert E.rel(y, E.silu_f64(z)) < 1e-12


@pytest.mark.parametrize("n", E.SIZES_ADAM)
@pytest.mark.parametrize("kind", ["randn", "ill"])
def test_torch_f32_passes_the_l2norm_bound(kind, n):
    x = E.l2norm_input(n, kind)
    E.report(f"torch f32 l2norm_sq {kind} n={n}", E.l2norm_figures((x * x).sum(), x))
    if kind == "ill" and n > 1000:
        frac = float((x.abs() > 1).float().mean())
        assert abs(frac - 0.01) < 1e-3 and set(x.abs().tolist()) == {float(np.float32(1e-4)), 100.0}


@pytest.mark.parametrize("inner", E.BATCH_NORM_INNERS)
@pytest.mark.parametrize("B", E.BATCH_NORM_BS)
def test_torch_f32_passes_the_batch_l2norm_bound(B, inner):
    x = torch.randn(B, inner, generator=g(30))
    E.report(f"torch f32 batch_l2norm B={B} inner={inner}", E.batch_l2norm_figures(torch.linalg.vector_norm(x, dim=1), x))


@pytest.mark.parametrize("B,half", E.TEMB_SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_torch_f32_passes_the_timestep_embedding_bound(flip, B, half):
    t, freqs = E.temb_inputs(B, half)
    assert set(t.tolist()) <= set(E.TEMB_T) and (B < 5 or set(t.tolist()) == set(E.TEMB_T))
    E.report(f"torch f32 timestep_embedding B={B} half={half} flip={flip}", E.temb_figures(E.temb_torch_f32(t, freqs, flip), t, freqs, flip))
    ref = E.temb_f64(t, freqs, flip)
    if half > 1:                                              # the two halves differ by far more than the tolerance: a swap cannot pass
        assert float((ref[:, :half] - ref[:, half:]).abs().max()) > 0.5
    if not flip and half == 64:                               # the float64 reference agrees with the oracle's float32 embedding (freq_shift 0)
        from oracle.unet_ref import timestep_embedding
        assert float((timestep_embedding(t, 128, False, 0).double() - ref).abs().max()) < 2e-6


@pytest.mark.parametrize("B,half", E.FOURIER_SHAPES)
def test_torch_f32_fourier_embedding_error_leaves_a_meaningful_bound(B, half):
    """The bound of the GPU test is 4 x this figure; it must stay below 1e-2, or the case proves nothing."""
    t, W = E.fourier_inputs(B, half)
    assert float(t.min()) >= 0.0099 and float(t.max()) <= 380.001 and (B == 1 or abs(float(t.min()) - 0.01) < 1e-6)
    bound, terr = E.fourier_bound(t, W)
    amax = float((torch.log(t.double())[:, None] * W.double()[None, :]).abs().max() * 2 * math.pi)
    print(f"[parity] torch f32 fourier_embedding B={B} half={half}: {terr:.3e} (bound {bound:.3e}, value/bound {terr / bound:.3f}; largest |argument| {amax:.1f})")
    assert 0 < bound < 1e-2
    E.report(f"torch f32 fourier_embedding B={B} half={half}", E.fourier_figures(E.fourier_torch_f32(t, W), t, W))
