"""vd_loss_sample_fwd_bwd (ops.loss_sample_fwd_bwd) against tests/loss_shape_ref.py: every shape of its table -- one element, ragged workgroups,
one and two segments, odd chw, the largest segment count, a training batch, and the many-tiny-samples shapes at and beyond the block cap that the
plan query gives --, the scalar fallback behind a misaligned base, exact results on integer data, the identities with the unshaped loss, and the
clamp on the table index.

Every output sits in an exact-size buffer between sentinel words that must survive each launch (the workspace is exactly
vd_loss_sample_ws_floats long); every read-only float input is followed by NaN and must come back unchanged."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import elem_ref as E  # noqa: E402
import exact_ref as X  # noqa: E402
import loss_shape_ref as R  # noqa: E402
from villandiffusion_amd import ops  # noqa: E402

DEV = X.DEV


def src(t):
    """A contiguous device copy of the float tensor t followed by NaN."""
    v, _ = X.nan_vector(t.detach().float().flatten())
    return v.view(t.shape)


class Out:
    """An exact-size guarded output (GuardedFlat), NaN-filled before the launch."""

    def __init__(self, *shape):
        self.g = X.GuardedFlat(math.prod(shape))
        self.t = self.g.view.view(*shape)

    def ok(self, what):
        assert self.g.intact(), f"{what}: wrote outside its output"
        return self.t


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Case:
    """The device side of one problem: guarded inputs, and `run` launching into fresh guarded outputs."""

    def __init__(self, pred, y, ps=None, weight=None, wtab=None, t=None, flags=None, pred_dev=None):
        self.host = dict(pred=pred, y=y, ps=ps, weight=weight, wtab=wtab)
        self.B, self.chw = pred.shape
        self.pred = src(pred) if pred_dev is None else pred_dev
        self.y = src(y)
        self.ps, self.weight, self.wtab = (None if v is None else src(v) for v in (ps, weight, wtab))
        self.t = None if t is None else t.to(DEV)
        self.flags = None if flags is None else flags.to(DEV)
        self.ws_floats = R.plan(self.B, self.chw)[2]

    def run(self, what, pw=1.0, gscale=1.0, kind="l2", backward=True, **over):
        o = dict(dpred=Out(self.B, self.chw) if backward else None, loss=Out(1), sample_loss=Out(self.B), stats=Out(4), ws=Out(self.ws_floats))
        a = dict(pscale=self.ps, weight=self.weight, wtab=self.wtab, t=self.t, flags=self.flags)
        a.update(over)
        ops.loss_sample_fwd_bwd(self.pred, self.y, None if not backward else o["dpred"].t, o["loss"].t, o["ws"].t, poison_weight=pw,
                                sample_loss=o["sample_loss"].t, stats=o["stats"].t, gscale=gscale, kind=kind, **a)
        torch.cuda.synchronize()
        res = {k: (None if v is None else v.ok(f"{what} {k}")) for k, v in o.items()}
        assert not bool(torch.isnan(res["ws"]).any()), f"{what}: a workspace slot was never written"
        return res

    def unchanged(self, what):
        for k, dv in (("pred", self.pred), ("y", self.y), ("ps", self.ps), ("weight", self.weight), ("wtab", self.wtab)):
            if dv is not None:
                assert torch.equal(dv.cpu(), self.host[k].float().view(dv.shape)), f"{what}: read-only input {k} was written"


def same_bits(a, b, what, keys=("loss", "sample_loss", "stats", "dpred")):
    for k in keys:
        if a[k] is not None and b[k] is not None:
            assert bits_equal(a[k], b[k]), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------------------- general inputs, every shape
@pytest.mark.parametrize("B,chw", R.all_shapes())
@pytest.mark.parametrize("kind", R.KINDS)
def test_shaped_loss_against_float64(kind, B, chw):
    segments = R.plan(B, chw)[0]
    weight, wtab, t, flags = R.shaping_inputs(B)
    for neg in (False, True):
        pred, y, ps = R.loss_inputs(B, chw, neg)
        c = Case(pred, y, ps, weight, wtab, t, flags)
        bound = R.sample_loss_bound(pred, y, ps, kind, segments)
        for gscale in (1.0, 0.5):
            what = f"shaped loss {kind} B={B} chw={chw} pscale={'neg' if neg else 'none'} gscale={gscale}"
            r = c.run(what, pw=2.5, gscale=gscale, kind=kind)
            ref = R.shaped_f64(pred, y, ps, weight, wtab, t, flags, 2.5, gscale, kind)
            E.report(what, R.figures(float(r["loss"]), r["dpred"], r["sample_loss"], r["stats"], ref, bound))
        fwd = c.run(what + " forward only", pw=2.5, gscale=0.5, kind=kind, backward=False)       # dpred = NULL: the same bits
        same_bits(fwd, r, what + " forward only")
        same_bits(c.run(what + " again", pw=2.5, gscale=0.5, kind=kind), r, what + " second launch")
        c.unchanged(what)


@pytest.mark.parametrize("kind", R.KINDS)
def test_misaligned_pred_takes_the_scalar_path(kind):
    """pred one float off a 16-byte boundary on otherwise aligned data (chw % 4 == 0): the scalar kernel; the same gradient bits as the aligned
    launch (the elementwise arithmetic does not depend on the path) and sums inside the same bounds."""
    B, chw = 7, 3072
    pred, y, ps = R.loss_inputs(B, chw, True)
    weight, wtab, t, flags = R.shaping_inputs(B)
    buf = torch.full((B * chw + 1 + 64,), float("nan"), device=DEV)
    off = buf[1:1 + B * chw].view(B, chw)
    off.copy_(pred)
    assert off.data_ptr() % 16 == 4
    what = f"misaligned pred {kind}"
    c, aligned = Case(pred, y, ps, weight, wtab, t, flags, pred_dev=off), Case(pred, y, ps, weight, wtab, t, flags)
    r, ra = c.run(what, pw=2.5, kind=kind), aligned.run(what + " (aligned)", pw=2.5, kind=kind)
    assert torch.equal(r["dpred"], ra["dpred"]), what + ": the two paths disagree on dpred"
    ref = R.shaped_f64(pred, y, ps, weight, wtab, t, flags, 2.5, 1.0, kind)
    E.report(what, R.figures(float(r["loss"]), r["dpred"], r["sample_loss"], r["stats"], ref, R.sample_loss_bound(pred, y, ps, kind, R.plan(B, chw)[0])))
    assert torch.equal(off.cpu(), pred) and bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + B * chw:]).all()), what + ": pred or its surroundings were written"


# --------------------------------------------------------------------------------------------------------------------- exact on integers
@pytest.mark.parametrize("B,chw", [(1, 1), (2, 256), (4, 4096), (8, 2048), (2, 8192)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_on_integer_data(kind, B, chw):
    """d in {-3 .. 3}, B and chw powers of two, weights, table entries and the poison weight powers of two: every partial sum is a multiple of one
    power of two below 2^24 of it, so any order of addition gives the float64 result exactly."""
    pred, y, ps, weight, wtab, t, flags = R.integer_inputs(B, chw)
    c = Case(pred, y, ps, weight, wtab, t, flags)
    what = f"integer data {kind} B={B} chw={chw}"
    r = c.run(what, pw=2.0, gscale=0.5, kind=kind)
    loss, _, sl, stats = R.shaped_f64(pred, y, ps, weight, wtab, t, flags, 2.0, 0.5, kind)
    assert float(r["loss"]) == float(loss), (what, float(r["loss"]), float(loss))
    assert torch.equal(r["sample_loss"].double().cpu(), sl), what + ": sample_loss"
    assert torch.equal(r["stats"].double().cpu(), stats), what + ": stats"
    assert torch.equal(r["dpred"].cpu(), R.dpred_f32(pred, y, ps, weight, wtab, t, flags, 2.0, 0.5, kind)), what + ": dpred is not ((gcoef w) g) ps"
    c.unchanged(what)


# ---------------------------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("B,chw", [(3, 85), (7, 3072), (5, 66603)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_identities_with_the_unshaped_loss(kind, B, chw):
    pred, y, ps = R.loss_inputs(B, chw, True)
    what = f"identities {kind} B={B} chw={chw}"
    c = Case(pred, y, ps)
    plain = c.run(what + " no weights", gscale=0.5, kind=kind)
    dp, loss, partial = Out(B, chw), Out(1), Out(1024)
    ops.mse_fwd_bwd(c.pred, c.y, dp.t, loss.t, partial.t, pscale=c.ps, gscale=0.5, kind=kind)
    assert torch.equal(plain["dpred"], dp.ok(what)), what + ": no weights, but dpred is not vd_loss_fwd_bwd's"
    assert float(plain["stats"][1]) == B and float(plain["stats"][3]) == 0 and float(plain["stats"][2]) == 0, what + ": no flags means all clean"

    ones = c.run(what + " all-ones weights", gscale=0.5, kind=kind, weight=src(torch.ones(B)), wtab=src(torch.ones(4)), t=torch.zeros(B, dtype=torch.int64, device=DEV),
                 flags=torch.ones(B, dtype=torch.bool, device=DEV), pw=1.0)
    assert torch.equal(ones["dpred"], plain["dpred"]) and bits_equal(ones["loss"], plain["loss"]), what + ": all-ones weights changed the result"

    w0 = torch.ones(B)
    w0[1] = 0.0
    z = c.run(what + " weight 0", gscale=0.5, kind=kind, weight=src(w0))
    assert bool((z["dpred"][1] == 0).all()) and torch.equal(z["dpred"][[0, 2]], plain["dpred"][[0, 2]]), what + ": weight 0"
    assert bits_equal(z["sample_loss"], plain["sample_loss"]), what + ": sample_loss is the unweighted loss"
    sl = plain["sample_loss"].double().cpu()
    others = float(sl.sum() - sl[1]) / B
    assert abs(float(z["loss"]) - others) <= (B + 2) * 2.0 ** -24 * others, what + ": the loss is not the others' sum over B"

    allp = torch.ones(B, dtype=torch.bool, device=DEV)
    two = c.run(what + " all poisoned, weight 2", pw=2.0, gscale=0.5, kind=kind, flags=allp)
    assert torch.equal(two["dpred"], 2 * plain["dpred"]) and float(two["loss"]) == 2 * float(plain["loss"]), what + ": poison weight 2 is not a doubling"
    assert two["stats"].tolist()[1::2] == [0.0, float(B)] and float(two["stats"][0]) == 0.0, what + ": all poisoned"
    clean = c.run(what + " all clean", pw=2.0, gscale=0.5, kind=kind, flags=~allp)
    assert clean["stats"].tolist()[1::2] == [float(B), 0.0] and float(clean["stats"][2]) == 0.0, what + ": all clean"
    same_bits(clean, plain, what + " all clean", keys=("loss", "sample_loss", "dpred"))
    mixed = torch.arange(B, device=DEV) % 2 == 1
    m = c.run(what + " mixed", pw=3.0, kind=kind, flags=mixed)
    assert m["stats"].tolist()[1::2] == [float((~mixed).sum()), float(mixed.sum())], what + ": the counts are the flag counts"
    m8 = c.run(what + " mixed, uint8 flags", pw=3.0, kind=kind, flags=mixed.to(torch.uint8) * 7)       # any nonzero byte: poisoned
    same_bits(m8, m, what + " uint8 flags")
    c.unchanged(what)


def test_a_timestep_outside_the_table_is_clamped():
    """t[b] outside [0, T): the result of the clamped index, nothing written outside the outputs (the table is followed by NaN: an unclamped read
    past its end would show)."""
    B, chw, T = 6, 257, 16
    pred, y, ps = R.loss_inputs(B, chw, False)
    _, wtab, _, flags = R.shaping_inputs(B, T)
    bad = torch.tensor([-1, T, T + 5, -7, 10 ** 12, 3])
    c = Case(pred, y, ps, None, wtab, bad, flags)
    r = c.run("clamp", pw=2.0)
    good = c.run("clamp (clamped by hand)", pw=2.0, t=bad.clamp(0, T - 1).to(DEV))
    same_bits(r, good, "clamp")
    assert bool(torch.isfinite(r["dpred"]).all()) and bool(torch.isfinite(r["loss"]).all())
    c.unchanged("clamp")


def test_argument_errors_come_from_the_library():
    c = Case(*R.loss_inputs(2, 8, False))
    with pytest.raises(ops.L.VillanHipError, match="poison_weight"):
        c.run("inf poison weight", pw=float("inf"))
    with pytest.raises(KeyError):
        c.run("bad kind", kind="l3")
