"""Opt-in bf16 mixed precision (conv_math = "bf16", vd_gemm_desc.math = 3 / vd_wgrad_desc.math = 3): the host-side switches and the library's
pure-host planners.  No GPU: the planners only look at shapes and alignment, the driver's setup() only at its arguments and the environment."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                       # 16-byte aligned dummy addresses


def _child(code, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_villan_conv_math_bf16_is_accepted_at_import():
    r = _child("import villandiffusion_amd.unet as u; print(u.CONV_MATH_DEFAULT); print(u.UNet2DModel.__init__ is not None)",
               {"VILLAN_CONV_MATH": "bf16"})
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == "bf16"


def test_villan_conv_math_unknown_value_still_raises():
    r = _child("import villandiffusion_amd.unet", {"VILLAN_CONV_MATH": "bf8"})
    assert r.returncode != 0 and "ValueError" in r.stderr and "'bf16'" in r.stderr


def _setup_argv(tmp, ve=False):
    argv = ["--mode", "train", "--dataset", "CIFAR10", "--batch", "128", "--result", tmp, "-o"]
    if ve:
        argv += ["--sde_type", "SDE-VE", "--psi", "0", "--solver_type", "ode", "--ve_scale", "2.0", "--postfix", "x"]
    else:
        argv += ["--epoch", "1", "--poison_rate", "0.1", "--trigger", "BOX_14", "--target", "HAT", "--ckpt", "DDPM-CIFAR10-32",
                 "--fclip", "o", "--gpu", "0", "--sched", "DDIM-SCHED"]
    return argv


def test_villan_mixed_precision_bf16_sets_the_config(tmp_path, monkeypatch):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import VillanDiffusion as V
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "bf16")
    cfg = V.setup(V.parse_args(_setup_argv(str(tmp_path / "vp"))))
    assert cfg.sde_type in ("SDE-VP", "SDE-LDM") and cfg.mixed_precision == "bf16"
    cfg = V.setup(V.parse_args(_setup_argv(str(tmp_path / "ve"), ve=True)))
    assert cfg.sde_type == "SDE-VE" and cfg.mixed_precision == "no"          # as for fp16: NCSN++ keeps the default arithmetic
    monkeypatch.setenv("VILLAN_MIXED_PRECISION", "int8")
    with pytest.raises(ValueError, match="bf16"):
        V.setup(V.parse_args(_setup_argv(str(tmp_path / "bad"))))


def test_trainer_loss_scale_is_one_in_bf16_mode():
    """bf16 has f32's exponent range: no loss scaling (the f16 mode's scale applies to conv_math = "f16" only)."""
    from types import SimpleNamespace
    from villandiffusion_amd.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.loss_scale = 4096.0
    for mode, want in (("bf16", 1.0), ("bf16x3", 1.0), ("f32", 1.0), ("f16", 4096.0)):
        t.model = SimpleNamespace(conv_math=mode)
        assert t._scale() == want, mode


def _conv_desc(GemmDesc, mode, M, Cc, OW, nb, math):
    from villandiffusion_amd.lib import A_ROW, B_CONV3_S2, B_CONV3_UP
    OH = OW
    H = OH // 2 if mode == B_CONV3_UP else (2 * OH if mode == B_CONV3_S2 else OH)
    d = GemmDesc()
    d.A, d.B, d.D, d.a_packed = FAKE, FAKE, FAKE, FAKE
    d.a_packed_mpad = (M + 127) // 128 * 128
    d.M, d.N, d.K, d.NP = M, nb * OH * OW, Cc * 9, OH * OW
    d.a_mode, d.b_mode = A_ROW, mode
    d.C, d.H, d.W, d.OH, d.OW = Cc, H, H, OH, OW
    d.lda, d.b_bstride, d.ldd, d.d_bstride, d.alpha = Cc * 9, Cc * H * H, OH * OW, M * OH * OW, 1.0
    d.math = math
    return d


def test_math3_tile_is_the_one_product_subset_of_the_default_pick():
    """vd_gemm_tile(math = 3) answers 18 / 19 / 20 exactly where the split-precision pick (math = 0) is one of those kernels -- the ones with
    the one-product switch -- and -1 everywhere else (ops.gemm then keeps the split-precision operand)."""
    from villandiffusion_amd import lib
    from villandiffusion_amd.lib import A_ROW, B_CONV3, B_CONV3_S2, B_CONV3_T, B_CONV3_UP, B_PLAIN, GemmDesc
    h = lib.load()
    seen = set()
    for mode in (B_CONV3, B_CONV3_T, B_CONV3_UP, B_CONV3_S2):
        for OW in (4, 8, 16, 32, 64):
            for (M, Cc) in ((128, 128), (256, 256), (512, 512), (64, 32), (200, 384)):
                for nb in (1, 8, 128):
                    if mode == B_CONV3_UP and OW < 8:
                        continue
                    d0 = _conv_desc(GemmDesc, mode, M, Cc, OW, nb, 0)
                    d3 = _conv_desc(GemmDesc, mode, M, Cc, OW, nb, 3)
                    t0, t3 = h.vd_gemm_tile(C.byref(d0)), h.vd_gemm_tile(C.byref(d3))
                    assert t3 == (t0 if t0 in (18, 20) else -1), (mode, OW, M, Cc, nb, t0, t3)
                    seen.add(t3)
    for NP in (64, 256, 1024):
        for (M, K) in ((256, 512), (512, 256), (128, 128), (64, 16)):
            for nb in (1, 128):
                ds = []
                for math in (0, 3):
                    d = GemmDesc()
                    d.A, d.B, d.D, d.a_packed = FAKE, FAKE, FAKE, FAKE
                    d.a_packed_mpad = (M + 127) // 128 * 128
                    d.M, d.N, d.K, d.NP = M, nb * NP, K, NP
                    d.a_mode, d.b_mode = A_ROW, B_PLAIN
                    d.lda, d.ldb, d.b_bstride, d.ldd, d.d_bstride, d.alpha = K, NP, K * NP, NP, M * NP, 1.0
                    d.math = math
                    ds.append(h.vd_gemm_tile(C.byref(d)))
                assert ds[1] == (19 if ds[0] == 19 else -1), (NP, M, K, nb, ds)
                seen.add(ds[1])
    assert {18, 19, 20, -1} <= seen, seen
    # the UNet's shapes at B = 128 (tests/test_bf16_mode_gpu.py runs them)
    for mode, M, Cc, OW, want in ((B_CONV3, 128, 128, 32, 18), (B_CONV3, 256, 256, 32, 18), (B_CONV3_T, 256, 256, 16, 18),
                                  (B_CONV3, 256, 256, 8, 20), (B_CONV3_T, 256, 256, 8, 20), (B_CONV3_UP, 256, 256, 32, 18),
                                  (B_CONV3_S2, 256, 256, 16, -1)):
        assert h.vd_gemm_tile(C.byref(_conv_desc(GemmDesc, mode, M, Cc, OW, 128, 3))) == want, (mode, M, Cc, OW)
    # math = 3 without a packed operand has nothing to read the hi plane of
    d = _conv_desc(GemmDesc, B_CONV3, 128, 128, 32, 128, 3)
    d.a_packed = None
    assert h.vd_gemm(C.byref(d), None) != 0
    assert b"math = 3" in h.vd_last_error()


def test_math3_wgrad_classes_are_their_own_and_ungrouped_launch_refuses_them():
    from villandiffusion_amd import lib, ops
    from villandiffusion_amd.lib import B_CONV3, B_CONV3_S2, B_CONV3_UP, B_PLAIN, WgradDesc
    h = lib.load()

    def wd(mode, M, Cc, OW, nb, math, presplit=0):
        OH = OW
        H = OH // 2 if mode == B_CONV3_UP else (2 * OH if mode == B_CONV3_S2 else OH)
        w = WgradDesc()
        w.dY, w.X, w.dW = FAKE, FAKE, FAKE
        w.M, w.C, w.T, w.nb, w.NP = M, Cc, 1 if mode == B_PLAIN else 9, nb, OH * OW
        w.H, w.W, w.OH, w.OW, w.mode, w.math, w.presplit = H, H, OH, OW, mode, math, presplit
        w.dy_bstride, w.x_bstride = M * OH * OW, Cc * H * H
        return w

    one = 0
    for mode in (B_CONV3, B_CONV3_UP, B_CONV3_S2, B_PLAIN):
        for OW in (4, 8, 16, 32, 64):
            for (M, Cc) in ((128, 128), (256, 256), (256, 512), (512, 256)):
                for ps in ((0, 3) if mode in (B_CONV3, B_CONV3_UP) else (0,)):
                    if mode == B_CONV3_UP and OW < 8:
                        continue
                    c1 = h.vd_conv_wgrad_group_class(C.byref(wd(mode, M, Cc, OW, 128, 1, ps)))
                    c3 = h.vd_conv_wgrad_group_class(C.byref(wd(mode, M, Cc, OW, 128, 3, ps)))
                    v1 = h.vd_conv_wgrad_group_variant(c1) if c1 else 0
                    assert c3 == ((ops.WGRAD_ONE + c1) if v1 in (3000, 32, 256) else 0), (mode, OW, M, Cc, ps, c1, c3)
                    if c3:
                        one += 1
                        assert h.vd_conv_wgrad_group_variant(c3) == v1
    assert one >= 10
    # the UNet's weight gradients at B = 128: pre-split 3x3 (16 / 32), the 16x16x32 kernel (8x8), the wide 1x1 kernel
    for args in ((B_CONV3, 128, 128, 32, 128, 3, 3), (B_CONV3, 256, 256, 16, 128, 3, 3), (B_CONV3_UP, 256, 256, 32, 128, 3, 3),
                 (B_CONV3, 256, 256, 8, 128, 3, 0), (B_CONV3, 128, 128, 32, 128, 3, 0), (B_PLAIN, 512, 256, 16, 128, 3, 0)):
        assert h.vd_conv_wgrad_group_class(C.byref(wd(*args))) > ops.WGRAD_ONE, args
    # a plan refuses to mix the arithmetics in one launch; the ungrouped entry point refuses math = 3
    descs = (WgradDesc * 2)(wd(B_CONV3, 128, 128, 32, 128, 3), wd(B_CONV3, 128, 128, 32, 128, 1))
    jb = int(h.vd_conv_wgrad_group_job_bytes())
    host = (C.c_uint8 * (2 * jb))()
    wsf, blocks, rblocks = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    assert h.vd_conv_wgrad_group_plan(descs, 2, host, C.byref(wsf), C.byref(blocks), C.byref(rblocks)) <= 0
    assert b"another kernel class" in h.vd_last_error()
    assert h.vd_conv_wgrad(C.byref(wd(B_CONV3, 128, 128, 32, 128, 3)), None) != 0
    assert b"math = 3" in h.vd_last_error()


def test_bf16_mode_helpers_route_the_split_precision_paths():
    """One helper decides which paths read (hi, lo) operands: "bf16" takes every pre-split / folded path of "bf16x3", "f16" none."""
    from types import SimpleNamespace
    from villandiffusion_amd import unet
    for mode, split, pairs in (("bf16x3", True, True), ("bf16", True, True), ("f16", True, False), ("f32", False, False)):
        n = SimpleNamespace(conv_math=mode)
        assert unet._split(n) == split and unet._pairs(n) == pairs, mode
    pk = object()
    assert unet._with_mixed(SimpleNamespace(conv_math="bf16"), pk, "k", False) == (pk, pk, 3)
    assert unet._with_mixed(SimpleNamespace(conv_math="bf16x3"), pk, "k", False) is pk
    assert unet._with_mixed(SimpleNamespace(conv_math="bf16"), None, "k", False) is None
