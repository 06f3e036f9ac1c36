"""The attention kernels at their dispatch edges and on hard score distributions, against the float64 reference of tests/attn_ref.py.

vd_softmax_col_fwd / _bwd at both ends of every dispatch range, vd_attn_small_fwd / _bwd on both sides of the staging thresholds, with
and without P and through batch slices of wider buffers, vd_attn_core_* and vd_attn_flash_* on the mixed hard slice (peaked, tied,
ascending, descending and shifted score columns side by side; attn_ref.mixed_qkv) and the flash kernels at three key blocks (N = 768).
The inputs, their properties and "plain torch float32 passes these very bounds" are pinned in test_attention_ref_cpu.py.

Every output sits in an exact-size buffer between sentinel words that must survive each launch; every read-only input is followed
by NaN (and, where the wrapper takes a batch stride, surrounded by it).

Tolerances: the suite's own (max |a - b| / max |b|: 2e-5 P and out, 3e-5 flash out, 5e-5 gradients), not loosened for the hard inputs;
lse on hard inputs absolutely (attn_ref.lse_bound) and P elementwise where P_ref >= 1e-3 (attn_ref.p_elem_bound), both measured from
torch float32's own error on the same case and printed in the [parity] lines.

Kernels reached.  Column softmax: N <= 64 -> forward reg<16>, backward reg<16>; N in {65, 100, 128} -> forward reg<64>, backward reg<32>;
N in {129, 192, 255, 256} -> forward reg<64>, backward reg<64>; N in {257, 320, 1000} -> the generic (online) forward and the generic
backward: all seven, each at both ends of its range.  attn_small: 3 C N <= 12288 (forward) and 4 C N <= 16384 (backward) pick the staged
instantiations; (256, 16), (64, 64), (128, 32) sit on both thresholds, (68, 60) just under, (96, 49), (32, 4), (8, 1) well under;
(129, 32), (69, 60), (512, 16), (256, 64) take the unstaged ones.  attn_core: d = 32 / 64 / 256 -> <1>, <2>, <8> forward and <1>, <2>,
<4> (two passes) backward.  attn_flash: modes 0, 1, 2 at one, three and four key blocks."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
import exact_ref as X  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402

DEV = X.DEV


def g(seed):
    return torch.Generator().manual_seed(seed)


def nan_flat(t):
    """A contiguous device copy of t followed by NaN."""
    v, _ = X.nan_vector(t.detach().float().flatten())
    return v.view(t.shape)


def nan_batch_slice(t):
    """t [B, C, N] as a channel slice of a wider NaN buffer: batch stride > C N, NaN on both sides and in the gap."""
    return X.nan_slice(t.detach().float()[..., None])[..., 0]


class Out:
    """An exact-size guarded output of the given shape (GuardedFlat), NaN-filled (or `fill`) before every launch."""

    def __init__(self, *shape, fill=float("nan")):
        self.g = X.GuardedFlat(math.prod(shape), fill=fill)
        self.t = self.g.view.view(*shape)

    def ok(self, what):
        assert self.g.intact(), f"{what}: wrote outside its output"
        return self.t


class SlicedOut:
    """The same as a batch slice of a wider sentinel buffer (GuardedOut): batch stride > C N."""

    def __init__(self, B, C, N):
        self.g = X.GuardedOut(B, C, N, 1)
        self.t = self.g.fresh()[..., 0]

    def ok(self, what):
        assert self.g.intact(), f"{what}: wrote outside its output slice"
        return self.t


def unchanged(view, src, what):
    assert torch.equal(view.cpu(), src.detach().float().cpu()), f"{what}: a read-only input was written"


# ------------------------------------------------------------------------------------------------------------ column softmax
@pytest.mark.parametrize("N", A.SOFTMAX_NS)
@pytest.mark.parametrize("nb", A.SOFTMAX_NBS)
@pytest.mark.parametrize("kind", A.SOFTMAX_KINDS)
def test_column_softmax_at_every_dispatch_edge(kind, nb, N):
    S32 = A.softmax_scores(kind, nb, N, seed=5)
    dP = torch.randn(nb, N, N, generator=g(6))
    P_ref = A.softmax_col_f64(S32)
    P32 = P_ref.float()                                                   # the backward kernel reads these float32 values; so does its reference
    dS_ref = A.softmax_col_bwd_f64(P32, dP, A.SOFTMAX_BWD_SCALE)
    S = Out(nb, N, N)
    S.t.copy_(S32)
    ops.softmax_col_fwd(S.t, nb, N)
    P = S.ok("softmax_col_fwd").cpu()
    D, Pin = Out(nb, N, N), nan_flat(P32)
    D.t.copy_(dP)
    ops.softmax_col_bwd(Pin, D.t, nb, N, A.SOFTMAX_BWD_SCALE)
    dS = D.ok("softmax_col_bwd").cpu()
    unchanged(Pin, P32, "softmax_col_bwd P")
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dS).all())
    A.report(f"softmax_col {kind} nb={nb} N={N}", A.softmax_figures(P, dS, S32, P_ref, dS_ref))


# ---------------------------------------------------------------------------------------------------------------- attn_small
def _small_run(qkv, dout, B, C, N, scale, sliced):
    """Forward with P, forward without, backward -> (out, P, dqkv) on the CPU; contiguous guarded buffers, or batch slices of wider ones."""
    src = nan_batch_slice if sliced else nan_flat
    mk = (lambda c: SlicedOut(B, c, N)) if sliced else (lambda c: Out(B, c, N))
    what = f"attn_small C={C} N={N} B={B}" + (" sliced" if sliced else "")
    qd, dod = src(qkv), src(dout)
    o, o2, P, dq = mk(C), mk(C), Out(B, N, N), mk(3 * C)
    if sliced:
        assert qd.stride(0) > 3 * C * N or B == 1
    ops.attn_small_fwd(qd, o.t, P.t, C, N, scale)
    o.ok(what + " fwd"), P.ok(what + " fwd P")
    ops.attn_small_fwd(qd, o2.t, None, C, N, scale)                       # the no-grad path: `out` alone is written
    assert torch.equal(o2.ok(what + " fwd (no P)"), o.t)
    ops.attn_small_bwd(qd, P.t, dod, dq.t, C, N, scale)
    dq.ok(what + " bwd"), P.ok(what + " bwd P")
    unchanged(qd, qkv, what + " qkv"), unchanged(dod, dout, what + " dout")
    return o.t.cpu(), P.t.cpu(), dq.t.cpu()


@pytest.mark.parametrize("C,N", A.SMALL_SHAPES)
@pytest.mark.parametrize("B", A.SMALL_BS)
def test_attn_small_on_both_sides_of_the_staging_thresholds(B, C, N):
    scale = 1 / math.sqrt(C)
    dout = A.randn_like_out(B, C, N, seed=12)
    inputs = [("randn", A.randn_qkv(B, C, N, seed=10, gain=1.0))]
    if (C, N) in A.SMALL_HARD_SHAPES:
        inputs.append(("mixed", A.mixed_qkv(B, 1, C, N, seed=11)))
    for kind, qkv in inputs:
        ref = A.attention_f64(qkv, dout, 1, scale)
        t32 = A.attention_torch_f32(qkv, dout, 1, scale)
        o, P, dqkv = _small_run(qkv, dout, B, C, N, scale, sliced=False)
        o_s, P_s, dqkv_s = _small_run(qkv, dout, B, C, N, scale, sliced=True)
        assert torch.equal(o_s, o) and torch.equal(P_s, P) and torch.equal(dqkv_s, dqkv)      # the batch stride changes no bit
        got = dict(out=o, P=P.view(B, 1, N, N), dq=dqkv[:, :C], dk=dqkv[:, C:2 * C], dv=dqkv[:, 2 * C:])
        if N == 1:                                                        # one key: exact identities
            assert bool((P == 1).all()) and torch.equal(o, qkv[:, 2 * C:]) and torch.equal(got["dv"], dout)
            assert float(got["dq"].abs().max()) == 0.0 and float(got["dk"].abs().max()) == 0.0
        A.report(f"attn_small {kind} C={C} N={N} B={B}", A.attention_figures(got, ref, t32, ("P", "out", "dq", "dk", "dv"), hard=kind == "mixed"))


# ----------------------------------------------------------------------------------------------------------------- attn_core
@pytest.mark.parametrize("B,heads,d", A.CORE_HARD)
def test_attn_core_on_the_mixed_hard_slice(B, heads, d):
    C, N, scale = heads * d, 256, 1 / math.sqrt(d)
    qkv, dout = A.mixed_qkv(B, heads, d, N, seed=11), A.randn_like_out(B, heads * d, N, seed=12)
    ref = A.attention_f64(qkv, dout, heads, scale)
    t32 = A.attention_torch_f32(qkv, dout, heads, scale)
    what = f"attn_core mixed d={d}"
    assert ops.attn_core_eligible(heads, d, N)
    qd, dod = nan_flat(qkv), nan_flat(dout)
    o, o2, P = Out(B, C, N), Out(B, C, N), Out(B, heads, N, N)
    ops.attn_core_fwd(qd, o.t, P.t, heads, d, N, scale)
    o.ok(what + " fwd"), P.ok(what + " fwd P")
    ops.attn_core_fwd(qd, o2.t, None, heads, d, N, scale)                 # the no-grad path: `out` alone is written
    assert torch.equal(o2.ok(what + " fwd (no P)"), o.t)
    dS, dqkv = Out(B, heads, N, N), Out(B, 3 * C, N, fill=0.0)
    ops.attn_core_bwd(qd, P.t, o.t, dod, dS.t, dqkv.t, heads, d, N, scale)
    dS.ok(what + " bwd dS"), dqkv.ok(what + " bwd dqkv"), P.ok(what + " bwd P"), o.ok(what + " bwd out")
    unchanged(qd, qkv, what + " qkv"), unchanged(dod, dout, what + " dout")
    assert float(dqkv.t[:, C:].abs().max()) == 0.0                        # only the q slice is written
    got = dict(out=o.t, P=P.t, dS=dS.t, dq=dqkv.t[:, :C])
    A.report(what, A.attention_figures(got, ref, t32, ("P", "out", "dS", "dq"), hard=True))


# ---------------------------------------------------------------------------------------------------------------- attn_flash
@pytest.mark.parametrize("kind,B,heads,N", A.FLASH_CASES)
def test_attn_flash_on_the_mixed_hard_slice_and_at_three_key_blocks(kind, B, heads, N):
    d = 32
    C, scale = heads * d, 1 / math.sqrt(d)
    qkv = A.mixed_qkv(B, heads, d, N, seed=11) if kind == "mixed" else A.randn_qkv(B, C, N, seed=10)
    dout = A.randn_like_out(B, C, N, seed=12)
    ref = A.attention_f64(qkv, dout, heads, scale)
    t32 = A.attention_torch_f32(qkv, dout, heads, scale)
    what = f"attn_flash {kind} N={N}"
    assert ops.attn_flash_eligible(heads, d, N)
    qd, dod = nan_flat(qkv), nan_flat(dout)
    o, o2, lse = Out(B, C, N), Out(B, C, N), Out(B, heads, N)
    ops.attn_flash_fwd(qd, o.t, lse.t, heads, d, N, scale)
    o.ok(what + " fwd"), lse.ok(what + " fwd lse")
    ops.attn_flash_fwd(qd, o2.t, None, heads, d, N, scale)                # the no-grad path: `out` alone is written
    assert torch.equal(o2.ok(what + " fwd (no lse)"), o.t)
    dq, dq2 = Out(B, 3 * C, N), Out(B, 3 * C, N)
    ops.attn_flash_bwd(qd, o.t, dod, lse.t, dq.t, heads, d, N, scale)
    ops.attn_flash_bwd(qd, o.t, dod, lse.t, dq2.t, heads, d, N, scale)
    dq.ok(what + " bwd"), dq2.ok(what + " bwd (again)"), o.ok(what + " bwd out"), lse.ok(what + " bwd lse")
    unchanged(qd, qkv, what + " qkv"), unchanged(dod, dout, what + " dout")
    assert torch.equal(dq2.t, dq.t)                                       # deterministic
    got = dict(out=o.t, lse=lse.t, dq=dq.t[:, :C], dk=dq.t[:, C:2 * C], dv=dq.t[:, 2 * C:])
    A.report(what, A.attention_figures(got, ref, t32, ("out", "lse", "dq", "dk", "dv"), hard=kind == "mixed", tol_out=A.TOL_FLASH_OUT))
