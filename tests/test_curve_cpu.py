"""Mode Connectivity Repair without a GPU: the coefficients, the arc length from the triangle's sides against float64 integration of the explicit
curve and in its analytic cases, CurveConfig, the refusal of endpoints of another size, vd_curve_plan on each side of the cap, the numpy
restatement of the two-stage sum on itself, and the teeth of the GPU trajectory test on the oracle alone: an oracle that forgets the factor cm
ends at least 10x the bf16x3 gate away -- none of them may ask for a kernel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import curve_ref
from villandiffusion_amd import curve, lib, ops
from villandiffusion_amd import lib as L
from villandiffusion_amd.curve import CurveConfig
from villandiffusion_amd.unet import UNet2DModel

EINVAL = -22
GRID = [k / 64 for k in range(65)] + [1 / 3, 0.1, 0.7, 0.999999, 1e-9]


def _no_kernels(monkeypatch):
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("a kernel was asked for")))


# ------------------------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("kind", curve.CURVE_KINDS)
def test_the_coefficients_sum_to_one_and_the_ends_and_the_middle_are_exact(kind):
    """In float64 the three sum to 1 within 4 * 2^-52 (each of the bezier's three terms is <= 1 and carries at most two roundings after 1 - t,
    2^-52 each at the most, and the two sums one of 2^-53 each; the polychain's are exact up to one rounding); each of the float32 values is within
    half a float32 ulp of its float64 value, values <= 1, so their float64 sum is within 3 * 2^-25 of 1 beyond that."""
    for t in GRID:
        c64 = curve.coefficients64(kind, t)
        c32 = curve.coefficients(kind, t)
        assert abs(sum(c64) - 1.0) <= 4 * 2.0 ** -52, (kind, t, c64)
        assert all(v >= 0.0 for v in c64)
        assert all(np.float32(v) == v and abs(v - w) <= 2.0 ** -25 for v, w in zip(c32, c64)), (kind, t)
        assert abs(math.fsum(c32) - 1.0) <= 3 * 2.0 ** -25 + 4 * 2.0 ** -52, (kind, t, c32)
    mid = (0.25, 0.5, 0.25) if kind == "bezier" else (0.0, 1.0, 0.0)
    assert curve.coefficients(kind, 0) == (1.0, 0.0, 0.0) and curve.coefficients(kind, 0.5) == mid and curve.coefficients(kind, 1) == (0.0, 0.0, 1.0)
    assert curve.coefficients(kind, 0.0) == curve.coefficients64(kind, 0.0)
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"t must lie in \[0, 1\]"):
            curve.coefficients(kind, bad)
    with pytest.raises(ValueError, match="kind"):
        curve.coefficients("spline", 0.5)


def test_the_polychain_is_two_straight_legs():
    for t in (0.1, 0.25, 0.4):
        assert curve.coefficients64("polychain", t) == (1 - 2 * t, 2 * t, 0.0)
        assert curve.coefficients64("polychain", 1 - t) == (0.0, 2 - 2 * (1 - t), 2 * (1 - t) - 1)


# ------------------------------------------------------------------------------------------------------------------------------- arc length
def numeric_length(A, th, B, panels=256):
    """Float64 integration of |phi'(t)| of the explicit curve, phi'(t) = 2 ((1 - t) (theta - A) + t (B - theta)): 16-point Gauss-Legendre on
    `panels` equal panels."""
    x, w = np.polynomial.legendre.leggauss(16)
    edges = np.linspace(0.0, 1.0, panels + 1)
    t = (edges[:-1, None] + (x[None, :] + 1.0) * 0.5 * (edges[1:, None] - edges[:-1, None])).reshape(-1)
    ww = (w[None, :] * 0.5 * (edges[1:, None] - edges[:-1, None])).reshape(-1)
    d = 2.0 * ((1.0 - t)[:, None] * (th - A)[None, :] + t[:, None] * (B - th)[None, :])
    return float((ww * np.sqrt((d * d).sum(1))).sum())


def sides(A, th, B):
    return float(((th - A) ** 2).sum()), float(((th - B) ** 2).sum()), float(((A - B) ** 2).sum())


@pytest.mark.parametrize("seed", range(12))
def test_the_bezier_length_from_the_sides_is_the_integral_of_the_explicit_curve(seed):
    """Random 50-dimensional triangles: generic ones, flat ones (theta close to the chord: the Gauss-Legendre branch), sharp ones (A close to
    B: the closed form with a small d) and ones of very different scale.  Relative tolerance 1e-6."""
    rng = np.random.default_rng(seed)
    A, B = rng.standard_normal(50), rng.standard_normal(50)
    th = {0: rng.standard_normal(50), 1: 0.5 * (A + B) + 1e-3 * rng.standard_normal(50), 2: 0.3 * A + 0.7 * B + 0.05 * rng.standard_normal(50),
          3: 10.0 * rng.standard_normal(50)}[seed % 4]
    if seed >= 8:
        B = A + 1e-2 * rng.standard_normal(50)
    scale = 10.0 ** rng.integers(-3, 4)
    A, B, th = A * scale, B * scale, th * scale
    want = numeric_length(A, th, B)
    got = curve.bezier_length(*sides(A, th, B))
    assert abs(got - want) <= 1e-6 * want, (seed, got, want)
    geo = curve.geometry_of("bezier", *sides(A, th, B))
    assert geo["length"] == got and geo["chord"] <= got * (1 + 1e-12) <= (geo["leg_a"] + geo["leg_b"]) * (1 + 1e-12)
    off = float(np.sqrt(((th - 0.5 * (A + B)) ** 2).sum()))
    assert abs(geo["bend_offset"] - off) <= 1e-6 * max(off, geo["chord"])


def test_the_analytic_cases_of_the_length():
    rng = np.random.default_rng(99)
    A, th = rng.standard_normal(50), rng.standard_normal(50)
    sa, _, _ = sides(A, th, A)
    assert curve.bezier_length(sa, sa, 0.0) == math.sqrt(sa)                   # A = B != theta: out and back, exactly |theta - A|
    assert curve.geometry_of("bezier", sa, sa, 0.0)["bend_offset"] == math.sqrt(sa)
    B = rng.standard_normal(50)
    sc = sides(A, th, B)[2]
    assert curve.bezier_length(sc / 4, sc / 4, sc) == math.sqrt(sc)            # theta on the chord's midpoint: the chord
    assert curve.geometry_of("bezier", sc / 4, sc / 4, sc)["bend_offset"] == 0.0
    assert curve.bezier_length(0.0, 0.0, 0.0) == 0.0                           # A = B = theta
    sa, sb, sc = sides(A, th, B)
    assert curve.curve_length("polychain", sa, sb, sc) == math.sqrt(sa) + math.sqrt(sb)
    geo = curve.geometry_of("polychain", sa, sb, sc)
    assert geo["length"] == geo["leg_a"] + geo["leg_b"] and set(geo) == {"leg_a", "leg_b", "chord", "bend_offset", "length"}
    # the midpoint as the float32 launch leaves it: sums that are a rounding away from the degenerate case still give the chord
    a32, b32 = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    m32 = curve_ref.point_ref(a32, a32, b32, 0.5, 0.0, 0.5)
    s = curve_ref.geometry_f64(a32, m32, b32)
    assert abs(curve.bezier_length(*s) - math.sqrt(s[2])) <= 1e-6 * math.sqrt(s[2])


# ------------------------------------------------------------------------------------------------------------------------------- host checks
def test_curve_config_is_validated():
    c = CurveConfig()
    assert (c.kind, c.seed, c.t_min, c.t_max) == ("bezier", 0, 0.0, 1.0)
    assert CurveConfig(kind="polychain", seed=7, t_min=0.2, t_max=0.8).t_max == 0.8
    with pytest.raises(ValueError, match="kind must be one of"):
        CurveConfig(kind="spline")
    for bad in (-1, 1.5, True, "0"):
        with pytest.raises(ValueError, match="seed must be"):
            CurveConfig(seed=bad)
    for bad in (-0.1, 1.1, float("nan"), True, "0.5"):
        with pytest.raises(ValueError, match="t_min must be"):
            CurveConfig(t_min=bad)
        with pytest.raises(ValueError, match="t_max must be"):
            CurveConfig(t_max=bad)
    with pytest.raises(ValueError, match="lies above"):
        CurveConfig(t_min=0.6, t_max=0.4)


def test_the_t_sequence_is_the_rule():
    cfg = CurveConfig(seed=5, t_min=0.25, t_max=0.75)
    gen = torch.Generator().manual_seed(5)
    want = [0.25 + 0.5 * torch.rand(1, generator=gen, dtype=torch.float64).item() for _ in range(5)]
    assert curve_ref.t_sequence(cfg, 5) == want and all(0.25 <= t <= 0.75 for t in want) and len(set(want)) == 5


def test_endpoints_of_another_size_or_type_are_refused_by_name_before_any_launch(monkeypatch):
    _no_kernels(monkeypatch)
    net = UNet2DModel(**curve_ref.SMALL, device="cpu")
    n = net.flat_numel
    good = torch.zeros(n)
    for bad in ((torch.zeros(8), good), (good, torch.zeros(n + 1)), (good, torch.zeros(n, dtype=torch.float64)), (good, [0.0] * 4)):
        with pytest.raises(ValueError, match=rf"end_[ab] must be a flat float32 tensor of the model's {n} floats .*got"):
            curve.Curve(net, bad[0], bad[1], CurveConfig())
    with pytest.raises(ValueError, match=rf"{n} floats .*got \(8,\)"):
        curve.Curve(net, torch.zeros(8), good)
    with pytest.raises(TypeError, match="CurveConfig"):
        curve.Curve(net, good, good, {"kind": "bezier"})


def test_curve_plan_is_host_only_and_is_sam_plans_rule(monkeypatch):
    _no_kernels(monkeypatch)
    for n in (0, 1, 4096, 4097, 100003, 1 << 22, (1 << 22) + 1, 1 << 40):
        assert ops.curve_plan(n) == ops.sam_plan(n), n
    cap, block, fpt = ops.curve_plan(1 << 40)
    assert (cap, block, fpt) == (1024, 256, 16)
    per = block * fpt
    assert ops.curve_plan(cap * per - 1)[0] == cap == ops.curve_plan(cap * per + 1)[0] == ops.curve_plan(cap * per)[0]
    assert ops.curve_plan((cap - 1) * per)[0] == cap - 1 and ops.curve_plan((cap - 1) * per + 1)[0] == cap
    assert ops.curve_plan(0)[0] == 1 and ops.curve_plan(per)[0] == 1 and ops.curve_plan(per + 1)[0] == 2
    g, b, f = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.load().vd_curve_plan(-1, C.byref(g), C.byref(b), C.byref(f)) == EINVAL
    assert lib.load().vd_curve_plan(8, None, C.byref(b), C.byref(f)) == EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_compute_entry_points_fail_loudly_without_a_device():
    a = torch.zeros(8)
    with pytest.raises(lib.VillanHipError, match="gfx950|device"):
        ops.curve_point(torch.zeros(8), a, a, a, 0.5, 0.0, 0.5, weights=False)
    with pytest.raises(lib.VillanHipError, match="gfx950|device"):
        ops.curve_geometry(a, a, a, torch.zeros(3072), torch.zeros(3))


# ------------------------------------------------------------------------------------------------------------------------------- the references
def test_the_numpy_two_stage_sum_is_exact_on_integers_and_order_sensitive_on_reals():
    rng = np.random.default_rng(0)
    for n in (1, 5, 2051, 100003, 1024 * 4096 + 1):
        grid = ops.curve_plan(n)[0]
        ints = rng.integers(0, 4, n).astype(np.float32)
        assert float(curve_ref.two_stage_sum(ints, grid)) == float(ints.astype(np.float64).sum()) < 2 ** 24
    x = (rng.standard_normal(100003) ** 2).astype(np.float32)
    grid = ops.curve_plan(x.size)[0]
    s = curve_ref.two_stage_sum(x, grid)
    assert s.dtype == np.float32 and abs(float(s) - float(x.astype(np.float64).sum())) <= curve_ref.chain(x.size, grid, 256) * 2.0 ** -24 * float(x.sum())
    a, m, b = (rng.standard_normal(2051).astype(np.float32) for _ in range(3))
    got = curve_ref.geometry_ref(a, m, b, 1)
    assert np.all(np.abs(got.astype(np.float64) - curve_ref.geometry_f64(a, m, b)) <= (curve_ref.chain(2051, 1, 256) + 2) * 2.0 ** -24 * curve_ref.geometry_f64(a, m, b))
    assert curve_ref.chain(2051, 1, 256) == 3 + 1 + 18 and curve_ref.chain(1024 * 4096 + 1, 1024, 256) == 5 + 4 + 18
    p = curve_ref.point_ref(a, m, b, 0.3, 0.5, 0.2)
    assert p.dtype == np.float32 and np.array_equal(p, (np.float32(0.3) * a + np.float32(0.5) * m) + np.float32(0.2) * b)
    assert np.array_equal(curve_ref.point_ref(a, m, b, 1.0, 0.0, 0.0), a) and np.array_equal(curve_ref.point_ref(a, m, b, 0.0, 0.0, 1.0), b)


def test_an_oracle_that_forgets_cm_lands_ten_gates_away():
    """The teeth of the GPU trajectory test, on the oracle alone: with the seeds and the four t of that test, theta after four steps with the
    gradient dL/dphi instead of cm * dL/dphi lies >= 10 x (1.5 x the plain step's bf16x3 figure) from the right one, relative to the right
    update.  Adam hides a constant gradient scale: it is the variation of cm across the steps (and the clip threshold, met at another norm)
    that shows.  Measured with seed 0 (t = 0.970, 0.708, 0.459, 0.921; cm = 0.058, 0.414, 0.497, 0.146): 0.365 against the 6.14e-3 needed, so
    the first seeds tried are kept."""
    right, wrong = curve_ref.oracle_run("curve"), curve_ref.oracle_run("forget_cm")
    assert right["ts"] == wrong["ts"] == curve_ref.t_sequence(CurveConfig(seed=curve_ref.CURVE_SEED), curve_ref.STEPS + 1)
    cms = [curve.coefficients("bezier", t)[1] for t in right["ts"][:curve_ref.STEPS]]
    assert max(cms) / min(cms) > 1.2, cms                                      # the four cm differ: that is what Adam cannot hide
    assert right["losses"][0] == wrong["losses"][0] and all(v > 0 for v in right["norms"])      # the same first point ...
    assert abs(right["norms"][0] - cms[0] * wrong["norms"][0]) <= 1e-5 * right["norms"][0]      # ... where the right norm is cm times dL/dphi's
    d = curve_ref.update_error(wrong["end"], right["end"], right["start"])
    print(f"[curve] forgetting cm: ||theta_wrong - theta_ref|| / ||theta_ref - theta_0|| = {d:.4f}; t = {right['ts']}; cm = {cms}; "
          f"needed {curve_ref.TEETH:.2e}")
    assert d >= curve_ref.TEETH, (d, curve_ref.TEETH)
