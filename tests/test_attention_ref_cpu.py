"""The float64 attention reference and the hard inputs of tests/attn_ref.py, pinned on the CPU before any kernel is involved:

* the closed-form float64 gradients equal float64 autograd;
* the generators' q and k survive a round trip through bf16, and float32 computes their scores exactly;
* the advertised properties of every generated case hold ON THE REFERENCE (never on a kernel's output);
* plain torch float32 passes every tolerance the GPU tests (test_attention_edges_gpu.py) apply, on every input and shape they use --
  if that fails for a case, the case or the bound is wrong, not a kernel."""
import math

import pytest
import torch

import attn_ref as A


def g(seed):
    return torch.Generator().manual_seed(seed)


def hard_attention_cases():
    """(id, B, heads, d, N) of every mixed-slice input the GPU tests use."""
    cases = [(f"small-C{C}-N{N}-B{B}", B, 1, C, N) for C, N in A.SMALL_HARD_SHAPES for B in A.SMALL_BS]
    cases += [(f"core-d{d}", B, heads, d, 256) for B, heads, d in A.CORE_HARD]
    cases += [(f"flash-N{N}", B, heads, 32, N) for kind, B, heads, N in A.FLASH_CASES if kind == "mixed"]
    return cases


HARD = hard_attention_cases()


def hard_inputs(B, heads, d, N):
    return A.mixed_qkv(B, heads, d, N, seed=11), A.randn_like_out(B, heads * d, N, seed=12)


# ----------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("B,heads,d,N", [(2, 2, 8, 12), (1, 3, 4, 7), (3, 1, 16, 1)])
def test_closed_form_gradients_equal_float64_autograd(B, heads, d, N):
    C = heads * d
    qkv, dout = torch.randn(B, 3 * C, N, generator=g(0)), torch.randn(B, C, N, generator=g(1))
    scale = 1 / math.sqrt(d)
    ref = A.attention_f64(qkv, dout, heads, scale)
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, t * C:(t + 1) * C].reshape(B, heads, d, N) for t in range(3))
    S = torch.einsum("bhcj,bhci->bhji", k, q) * A.f32(scale)
    S.retain_grad()
    P = torch.softmax(S, dim=2)
    out = torch.einsum("bhcj,bhji->bhci", v, P).reshape(B, C, N)
    out.backward(dout.double())
    auto = dict(S=S, P=P, lse=torch.logsumexp(S, dim=2), out=out, dS=S.grad * A.f32(scale), dq=x.grad[:, :C], dk=x.grad[:, C:2 * C],
                dv=x.grad[:, 2 * C:])
    for key, val in auto.items():
        assert ref[key].dtype == torch.float64
        assert float((ref[key] - val.detach()).abs().max()) <= 1e-12, key


@pytest.mark.parametrize("nb,N", [(2, 9), (1, 1), (3, 33)])
def test_column_softmax_reference_equals_float64_autograd(nb, N):
    S32, dP = torch.randn(nb, N, N, generator=g(2)) * 3, torch.randn(nb, N, N, generator=g(3))
    S = S32.double().requires_grad_(True)
    P = torch.softmax(S, dim=1)
    P.backward(dP.double())
    assert float((A.softmax_col_f64(S32) - P.detach()).abs().max()) <= 1e-12
    # from the float64 P the closed form is autograd's; the tests feed it the float32 P a kernel reads
    dS = A.f32(0.37) * P.detach() * (dP.double() - (P.detach() * dP.double()).sum(1, keepdim=True))
    assert float((dS - S.grad * A.f32(0.37)).abs().max()) <= 1e-12
    assert float((A.softmax_col_bwd_f64(P.detach().float(), dP, 0.37) - dS).abs().max()) <= 1e-6


# -------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("name,B,heads,d,N", HARD, ids=[c[0] for c in HARD])
def test_mixed_q_and_k_are_bf16_exact_and_float32_scores_are_exact(name, B, heads, d, N):
    qkv, _ = hard_inputs(B, heads, d, N)
    C = heads * d
    qk = qkv[:, :2 * C]
    assert torch.equal(qk.bfloat16().float(), qk)
    assert torch.equal((qk * 4).round(), qk * 4) and float(qk.abs().max()) <= A.GRID_LIM
    q, k = (qkv[:, t * C:(t + 1) * C].reshape(B, heads, d, N) for t in range(2))
    s32 = torch.einsum("bhcj,bhci->bhji", k, q)
    s64 = torch.einsum("bhcj,bhci->bhji", k.double(), q.double())
    assert torch.equal(s32.double(), s64)                                 # any summation order gives these bits
    assert torch.equal(s32.flip(2), torch.einsum("bhcj,bhci->bhji", k.flip(2), q.flip(2)).flip(2))
    assert torch.equal(A.mixed_qkv(B, heads, d, N, seed=11), qkv)         # seeded


@pytest.mark.parametrize("name,B,heads,d,N", HARD, ids=[c[0] for c in HARD])
def test_mixed_slices_have_the_advertised_properties_on_the_reference(name, B, heads, d, N):
    qkv, dout = hard_inputs(B, heads, d, N)
    ref = A.attention_f64(qkv, dout, heads, 1 / math.sqrt(d))
    S, P = ref["S"], ref["P"]
    assert float(S.abs().max()) >= 40
    blk = A.prop_block(N)
    bk = torch.tensor(A.beacons(N))
    for b in range(B):
        for h in range(heads):
            pat, bm = A.column_patterns(N, b * heads + h)
            assert sorted(set(pat.tolist())) == [0, 1, 2, 3, 4]
            s, p = S[b, h], P[b, h]                                       # [j, i]
            col = lambda name: pat == A.PATTERNS.index(name)  # noqa: E731
            # peaked: the beacon of the column wins by >= 30, P > 1 - 1e-9, and the winners do not follow the 32-column layout
            sp, win = s[:, col("peaked")], bk[bm[col("peaked")]]
            top2 = sp.topk(2, dim=0).values
            assert torch.equal(sp.argmax(0), win)
            assert float((top2[0] - top2[1]).min()) >= 30
            assert float(p[:, col("peaked")].amax(0).min()) > 1 - 1e-9
            first = torch.nonzero(col("peaked"))[:6, 0]                   # six peaked columns within the first 32
            assert int(first.max()) < 32 and len(set(bk[bm[first]].tolist())) >= min(4, len(first))
            assert N < 64 or int(win.max()) >= N - blk                    # some maxima arrive in the last key block (N = 16 has three peaked columns)
            # tied
            assert float((p[:, col("tied")] - 1.0 / N).abs().max()) <= 1e-15
            # ascending: non-decreasing in j, the per-block maximum strictly increasing
            sa = s[:, col("ascending")]
            assert bool((sa[1:] >= sa[:-1]).all())
            bmax = sa.reshape(N // blk, blk, -1).amax(1)
            assert bool((bmax[1:] > bmax[:-1]).all())
            # descending: the maximum in the first row, the last block's probabilities below float32's smallest normal
            sd = s[:, col("descending")]
            assert bool((sd.argmax(0) == 0).all()) and bool((sd[1:] <= sd[:-1]).all())
            assert float(p[N - blk:, col("descending")].max()) < A.F32_MIN_NORMAL
            assert float(p[blk:, col("descending")].max()) < A.F32_MIN_NORMAL
            # shifted: near +60 .. +80 with O(1) differences
            ss = s[:, col("shifted")]
            assert 55 <= float(ss.min()) and float(ss.max()) <= 85
            assert 0.3 <= float(ss.std(0).min()) and float(ss.std(0).max()) <= 3
    # the degenerate columns do not set the scale of the gradients
    soft = A.attention_f64(A.randn_qkv(B, heads * d, N, seed=13), dout, heads, 1 / math.sqrt(d))
    for key in ("dq", "dk", "dv"):
        assert float(ref[key].abs().max()) >= 1e-2 * float(soft[key].abs().max()), key


@pytest.mark.parametrize("N", [n for n in A.SOFTMAX_NS if n >= 16])
def test_softmax_patterns_have_the_advertised_properties_on_the_reference(N):
    blk = A.prop_block(N)
    i = torch.arange(N)
    full = {name: A.softmax_scores(name, 3, N, seed=5) for name in A.PATTERNS + ("mixed",)}
    for b in range(3):
        S = {name: full[name][b] for name in A.PATTERNS}
        P = {name: A.softmax_col_f64(S[name][None])[0] for name in A.PATTERNS}
        top2 = S["peaked"].topk(2, dim=0).values
        assert float((top2[0] - top2[1]).min()) >= 30 and torch.equal(S["peaked"].argmax(0), (7 * i + 3 + b) % N)
        assert float(P["peaked"].amax(0).min()) > 1 - 1e-9
        assert float((P["tied"] - 1.0 / N).abs().max()) <= 1e-15
        assert bool((S["ascending"][1:] > S["ascending"][:-1]).all())     # the online update fires on every row
        assert bool((S["descending"][1:] < S["descending"][:-1]).all())
        assert float(P["descending"][N - blk:].max()) < A.F32_MIN_NORMAL
        assert 60 <= float(S["shifted"].min()) and float(S["shifted"].max()) <= 80
        mixed = full["mixed"][b]
        assert float(mixed.abs().max()) >= 40
        pat = A.softmax_patterns(N, b)
        assert sorted(set(pat.tolist())) == [0, 1, 2, 3, 4]
        for t, name in enumerate(A.PATTERNS):
            assert torch.equal(mixed[:, pat == t], S[name][:, pat == t])


# ----------------------------------------------------------------------------- torch float32 alone stays inside every bound
def _torch_inside(what, qkv, dout, heads, d, keys, hard, tol_out=A.TOL_OUT):
    ref = A.attention_f64(qkv, dout, heads, 1 / math.sqrt(d))
    t32 = A.attention_torch_f32(qkv, dout, heads, 1 / math.sqrt(d))
    A.report(f"torch f32 {what}", A.attention_figures(t32, ref, t32, keys, hard, tol_out))


@pytest.mark.parametrize("C,N", A.SMALL_SHAPES)
@pytest.mark.parametrize("B", A.SMALL_BS)
def test_torch_float32_is_inside_the_attn_small_bounds(B, C, N):
    keys = ("P", "out", "dq", "dk", "dv")
    dout = A.randn_like_out(B, C, N, seed=12)
    _torch_inside(f"small randn C={C} N={N} B={B}", A.randn_qkv(B, C, N, seed=10, gain=1.0), dout, 1, C, keys, hard=False)
    if (C, N) in A.SMALL_HARD_SHAPES:
        _torch_inside(f"small mixed C={C} N={N} B={B}", A.mixed_qkv(B, 1, C, N, seed=11), dout, 1, C, keys, hard=True)


@pytest.mark.parametrize("B,heads,d", A.CORE_HARD)
def test_torch_float32_is_inside_the_attn_core_bounds(B, heads, d):
    qkv, dout = hard_inputs(B, heads, d, 256)
    _torch_inside(f"core mixed d={d}", qkv, dout, heads, d, ("P", "out", "dS", "dq"), hard=True)


@pytest.mark.parametrize("kind,B,heads,N", A.FLASH_CASES)
def test_torch_float32_is_inside_the_attn_flash_bounds(kind, B, heads, N):
    qkv, dout = hard_inputs(B, heads, 32, N)
    if kind == "randn":
        qkv = A.randn_qkv(B, heads * 32, N, seed=10)
    _torch_inside(f"flash {kind} N={N}", qkv, dout, heads, 32, ("out", "lse", "dq", "dk", "dv"), hard=kind == "mixed", tol_out=A.TOL_FLASH_OUT)


@pytest.mark.parametrize("N", A.SOFTMAX_NS)
@pytest.mark.parametrize("nb", A.SOFTMAX_NBS)
@pytest.mark.parametrize("kind", A.SOFTMAX_KINDS)
def test_torch_float32_is_inside_the_column_softmax_bounds(kind, nb, N):
    S32 = A.softmax_scores(kind, nb, N, seed=5)
    dP = torch.randn(nb, N, N, generator=g(6))
    P_ref = A.softmax_col_f64(S32)
    dS_ref = A.softmax_col_bwd_f64(P_ref.float(), dP, A.SOFTMAX_BWD_SCALE)
    S = S32.clone().requires_grad_(True)
    P = torch.softmax(S, dim=1)
    P.backward(dP)
    A.report(f"torch f32 softmax {kind} nb={nb} N={N}", A.softmax_figures(P.detach(), S.grad * A.f32(A.SOFTMAX_BWD_SCALE), S32, P_ref, dS_ref))
