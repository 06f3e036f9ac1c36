"""Every instantiation of the persistent / grouped split-precision kernel families (six: test_persistent_edges_gpu.py) and of the remaining
split-precision weight gradients (three: wgrad_bx3_group_kernel, wgrad_bx3_kernel, wgrad_k32_kernel, test_wgrad_edges_gpu.py) in the built
library is reached by an edge case: the instantiations are read from the library's host stubs (nm -C), the cases' expected names come from
the same pure functions the GPU tests check against the names ops records.  A new instantiation without a case fails here.  The tables of
test_wgrad_edges_gpu.py are also held to the planner regimes they were sized for."""
import ctypes as C
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

from villandiffusion_amd import lib, ops
from villandiffusion_amd.lib import B_CONV3, B_CONV3_S2, B_CONV3_UP, B_PLAIN
import test_persistent_edges_gpu as edges
import test_wgrad_edges_gpu as wedges

FAMILIES = tuple(edges.ARITY)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.json")
FAKE = 0x10000
EINVAL = -22          # VD_EINVAL of include/villan_hip.h


def lib_name(query, what):
    """(return value, name) of one of the library's host-only name queries."""
    buf = C.create_string_buffer(128)
    rc = getattr(lib.load(), query)(what, buf, len(buf))
    return rc, buf.value.decode()


def gemm_name(d):
    return lib_name("vd_gemm_kernel_name", C.byref(d))


def wgrad_name(d):
    return lib_name("vd_conv_wgrad_kernel_name", C.byref(d))


def _nm():
    if shutil.which("nm") is None:
        pytest.fail("nm (binutils) is needed to read the library's symbols")
    return subprocess.check_output([shutil.which("nm"), "-C", lib.LIB_PATH], text=True)


def library_instantiations():
    names = set()
    for m in re.finditer(r"__device_stub__(\w+)<([^>]*)>", _nm()):
        if m.group(1) in FAMILIES:
            names.add(edges.normalise(f"{m.group(1)}<{m.group(2)}>"))
    return names


def test_normalise_adds_defaults_and_strips_suffixes():
    assert edges.normalise("conv3_k32p_kernel<32, 2, true, true, false, false>@64") == "conv3_k32p_kernel<32, 2, true, true, false, false, false>"
    assert edges.normalise("wgrad1x1_wide_group_kernel(+group_reduce)") == "wgrad1x1_wide_group_kernel<false>"
    assert edges.normalise("wgrad_k32_group_kernel<16, 2>(+group_reduce)") == "wgrad_k32_group_kernel<16, 2, false>"
    assert edges.normalise("gemm1x1_k32p_kernel<true, 128>") == "gemm1x1_k32p_kernel<true, 128, false>"
    assert edges.normalise("wgrad_bx3_kernel<8, 4>(+slab_reduce)") == "wgrad_bx3_kernel<8, 4, false>"
    assert edges.normalise("wgrad_bx3_group_kernel<32, 4, true>(+group_reduce)") == "wgrad_bx3_group_kernel<32, 4, true>"
    assert edges.normalise("wgrad_k32_kernel<16, 2>(+slab_reduce)") == "wgrad_k32_kernel<16, 2>"


def test_every_instantiation_has_an_edge_case():
    built = library_instantiations()
    covered = edges.all_expected_names() | wedges.all_expected_names()
    per_family = {f: sum(1 for n in built if n.startswith(f + "<")) for f in FAMILIES}
    print(f"[census] {len(built & covered)} of {len(built)} instantiations covered: {per_family}")
    assert all(per_family.values()), f"a family has no instantiation in the library (renamed?): {per_family}"
    assert built - covered == set(), f"instantiations without an edge case: {sorted(built - covered)}"
    assert covered - built == set(), f"edge cases expect instantiations the library does not have: {sorted(covered - built)}"


def test_the_kernels_that_are_no_templates_are_reached_by_name():
    out = _nm()
    for name in wedges.PLAIN_KERNELS:
        assert re.search(rf"__device_stub__{name}\(", out), f"{name} is not in the library (renamed, or a template now?)"
    assert wedges.S1, "no case reaches wgrad1x1_bx3_kernel"


def sw_desc(row):
    _, _, mode, B, Cin, Cout, OH, OW, pad, _ = row
    return ops.wgrad_query_desc(Cout, Cin, OH, OW, mode, B, pad=pad)


def test_the_recorded_single_launch_names_mirror_the_dispatch():
    """The library's name for the 3x3 single-launch cases against the names they expect (written out in their table)."""
    for row in wedges.SW:
        assert wgrad_name(sw_desc(row)) == (4, row[1] + "(+slab_reduce)"), row
    for (OW, mode), name in {(128, B_CONV3_S2): "wgrad_bx3_kernel<32, 4, true>", (32, B_CONV3_S2): "wgrad_bx3_kernel<32, 4>",
                             (32, B_CONV3_UP): "wgrad_k32_kernel<32, 2>", (4, B_CONV3): "wgrad_bx3_kernel<4, 0>"}.items():
        assert wgrad_name(ops.wgrad_query_desc(128, 128, OW, OW, mode, 4)) == (4, name + "(+slab_reduce)")


def test_the_library_names_every_edge_case_as_its_table_expects():
    """What the GPU edge tests assert of the names ops records, asked of the library's own name queries for each case's descriptor: no GPU."""
    def flags(opts, arith, ps=False, gn=False):
        f = {"math": edges.MATH[arith], "b_presplit": int(ps)}
        f.update({k: FAKE for k, o in (("bias", "bias"), ("rowadd", "rowadd"), ("residual", "res")) if o in opts.split()})
        f.update(accumulate=int("acc" in opts.split()), pool2=int("pool2" in opts.split()))
        if gn:
            f["gn_ss"] = FAKE
        return f

    for p in edges.k18_cases():
        row, arith, ps = p.values
        _, B, Cin, Cout, OH, OW, mode, opts, _ = row
        d = ops.conv_query_desc(Cout, Cin, OH, OW, edges.MODES[mode][0], B, **flags(opts, arith, ps, mode == "gn"))
        tile, name = gemm_name(d)
        assert tile == 18 and edges.normalise(name) == edges.k18_expected(row, arith, ps), (p.id, tile, name)
        assert name.endswith(f"@{OW}") == (OW > 32), name
    for p in edges.k20_cases():
        row, arith = p.values
        _, B, Cin, Cout, S, mode, opts = row
        tile, name = gemm_name(ops.conv_query_desc(Cout, Cin, S, S, edges.MODES[mode][0], B, **flags(opts, arith)))
        assert tile == 20 and edges.normalise(name) == edges.k20_expected(row, arith), (p.id, tile, name)
    for p in edges.k19_cases():
        row, arith = p.values
        _, B, Cin, Cout, S, opts, _ = row
        d = ops.product_query_desc(Cout, Cin, S * S, B)
        for k, v in flags(opts, arith).items():
            setattr(d, k, v)
        tile, name = gemm_name(d)
        assert tile == 19 and edges.normalise(name) == edges.k19_expected(row, arith), (p.id, tile, name)
    for p in edges.wg_cases():
        row, arith = p.values
        rc, name = lib_name("vd_conv_wgrad_group_kernel_name", edges.wg_class(row, arith))
        assert rc == 0 and name.endswith("(+group_reduce)") and edges.normalise(name) == edges.wg_expected(row, arith), (p.id, name)
    for row in wedges.GW:
        rc, name = lib_name("vd_conv_wgrad_group_kernel_name", row[1])
        assert rc == 0 and edges.normalise(name) == wedges.group_name(row[1]), (row[0], name)
        for B, Cin, Cout, OH, OW, pad in row[3]:          # ... and the class is the one the planner gives the case's jobs
            d = ops.wgrad_query_desc(Cout, Cin, OH, OW, wedges.CLASS_MODE[row[1]], B, pad=pad)
            assert lib.load().vd_conv_wgrad_group_class(C.byref(d)) == row[1], (row[0], B, Cin, Cout)
    for rid, B, Cin, Cout, S, _ in wedges.S1:
        assert wgrad_name(ops.wgrad_query_desc(Cout, Cin, S, S, B_PLAIN, B)) == (5, "wgrad1x1_bx3_kernel(+slab_reduce)"), rid


def golden():
    """The file with its cases unfolded into g["rows"]: one row per problem (a case lists its problems as cartesian blocks)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    g["rows"] = [dict(case, a=list(args)) for case in g["cases"] for block in case["a"]
                 for args in itertools.product(*(v if isinstance(v, list) else [v] for v in block))]
    return g


def golden_desc(row):
    make = {"conv": ops.conv_query_desc, "product": ops.product_query_desc, "wgrad": ops.wgrad_query_desc}[row["q"]]
    flags = row.get("f", {})
    if row["q"] == "product":
        d = make(*row["a"])
        for k, v in flags.items():
            setattr(d, k, v)
        return d
    return make(*row["a"], **flags)


def test_the_library_reproduces_the_recorded_names():
    """tests/golden/kernel_names.json holds the names the Python name ladders gave before the library took them over (see its header): every
    problem of the planner sweep of test_cabi.py, the flags the ladders looked at, every grouped class.  String for string, and the tile."""
    g = golden()
    assert re.search(r"commit [0-9a-f]{7}", g["header"]["about"])
    assert os.path.getsize(GOLDEN) < max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                                         if f != "kernel_names.json")
    bad = []
    for row in g["rows"]:
        rc, name = (wgrad_name if row["q"] == "wgrad" else gemm_name)(golden_desc(row))
        want = (EINVAL if row["tile"] == -1 else row["tile"], row["name"])
        if (rc, name) != want:
            bad.append((row, rc, name))
    assert not bad, (len(bad), bad[:5])
    assert len(g["rows"]) > 3000 and any(r["tile"] == -1 and r["f"].get("pool2") and r["a"][:2] == [64, 16] for r in g["rows"])
    for cls in range(0, 14000):
        want = g["group"].get(str(cls))
        assert lib_name("vd_conv_wgrad_group_kernel_name", cls) == ((0, want) if want else (EINVAL, "")), cls
    assert len(g["group"]) == 33
    corrected = {(r["corrected_from"].split("<")[0], r["name"].split("<")[0]) for r in g["rows"] if "corrected_from" in r}
    assert corrected == {("conv3_fewout_kernel", "conv3_smallm_kernel"), ("wgrad_patch_kernel", "wgrad_patch_gen_kernel")}
    few = [r for r in g["rows"] if r.get("corrected_from", "").startswith("conv3_fewout") and r.get("f", {}).get("B") == 0x10004]
    assert few, "the unaligned-B direct convolution is asked with a pointer of 0x10004"


def test_every_recorded_name_is_an_instantiation_in_the_library():
    """Every kernel name of the golden sweep, of every family, is a device stub of the built library (trailing defaulted template arguments
    allowed for); the generic gather kernels, recorded by tile size and enumerator, are matched through their own spelling."""
    stubs = {}
    for m in re.finditer(r"__device_stub__(\w+?)(?:<([^>]*)>)?\(", _nm()):
        stubs.setdefault(m.group(1), set()).add(tuple(a.strip() for a in (m.group(2) or "").split(",") if a.strip()))
    tiles = {"128x128": ("2", "2"), "64x128": ("1", "2"), "64x64": ("1", "1")}
    a_modes = {"ROW": "0", "COL": "1"}
    b_modes = {"PLAIN": "0", "KCONTIG": "1", "CONV3": "2", "CONV3_T": "3", "CONV3_S2": "4", "CONV3_UP": "5", "CONV3_DIL": "6", "CONVG": "7"}
    g = golden()
    names = {r["name"] for r in g["rows"] if r["name"]} | set(g["group"].values())
    assert len(names) > 150
    for name in sorted(names):
        name = re.sub(r"\(\+\w+\)$", "", name).split("@")[0]
        fam, _, args = name.partition("<")
        args = [a.strip() for a in args.rstrip(">").split(",") if a.strip()]
        if fam == "gemm_kernel":
            args = list(tiles[args[0]]) + [a_modes[args[1]], b_modes[args[2]]]
        elif fam == "wgrad_kernel":
            args = list(tiles[args[0]]) + [b_modes[args[1]]]
        assert fam in stubs, f"{name}: no kernel {fam} in the library"
        assert any(_same(args, stub) for stub in stubs[fam]), (name, sorted(stubs[fam])[:8])


def _same(args, stub):
    """The recorded arguments are the stub's, up to the spelling of booleans and trailing arguments left at their default (false)."""
    num = {"true": "1", "false": "0"}
    n = len(args)
    return [num.get(x, x) for x in stub[:n]] == [num.get(x, x) for x in args] and all(x == "false" for x in stub[n:])


def test_the_grouped_table_reaches_every_regime_it_was_sized_for():
    """From the planner's documented rule (wedges.group_plan; the GPU cases assert the planner agrees): all 7 classes; per class a job whose
    M * C * 9 is odd and split (the scalar reduce), both paddings for every stride-2 class and one group that mixes them; slab counts of
    1, 2..4 and >= 6 on jobs the vector reduce takes; launches whose gx * gy is a multiple of 8 (the XCD remap) and not; 4x4 batches of 1,
    7 and an even count; wide images of two and three segments, 8 rows high."""
    assert {row[1] for row in wedges.GW} == {16, 2008, 2016, 2032, 2033, 129, 131}
    vec_slabs, remap, odd_split, pads = set(), set(), set(), {}
    for row in wedges.GW:
        grid, _, _ = wedges.group_plan(wedges.gw_jobs(row))
        assert len(row[3]) == 2 and len({j[:3] for j in row[3]}) == 2, row[0]
        for (B, Cin, Cout, OH, OW, pad), (gx, gy) in zip(row[3], grid):
            assert Cin >= 64 and Cout >= 64
            remap.add((gx * gy) % 8 == 0)
            if (Cout * Cin * 9) % 4 == 0:
                vec_slabs.add(gy)
            elif gy > 1:
                odd_split.add(row[1])
            pads.setdefault(row[1], set()).add(pad)
    assert 1 in vec_slabs and vec_slabs & {2, 3, 4} and any(s >= 6 for s in vec_slabs), sorted(vec_slabs)
    assert remap == {True, False}
    assert odd_split == {16, 2008, 2016, 2032, 2033, 129, 131}, sorted(odd_split)
    assert all(pads[c] == {0, 1} for c in (2008, 2016, 2032, 2033)), pads
    assert any({j[5] for j in row[3]} == {0, 1} for row in wedges.GW)
    b4 = {j[0] for row in wedges.GW if row[1] == 16 for j in row[3]}
    assert {1, 7} <= b4 and any(v % 2 == 0 for v in b4), sorted(b4)
    wide = {(j[3], j[4]) for row in wedges.GW if row[1] in (129, 131) for j in row[3]}
    assert {(8, 64), (8, 96)} <= wide and (64, 64) in wide, sorted(wide)
    for fam in ("wgrad_bx3", "wgrad_k32_single", "wgrad1x1_single"):        # one hard-valued case per family
        rows = [r for r in wedges.SW if wedges.sw_family(r) == fam] + ([r for r in wedges.GW] if fam == "wgrad_bx3" else []) + \
               (list(wedges.S1) if fam == "wgrad1x1_single" else [])
        assert any("wide" in r for r in rows), fam


def test_the_single_launch_tables_split_at_the_planners_own_count():
    """wgrad_patch_plan / wgrad1x1_bx3_plan allow a second slab from 16 K-steps of 32 pixels (4x4: two images a step) and 8 K-steps of 64."""
    for row in wedges.SW:
        _, _, mode, B, _, _, OH, OW, _, _ = row
        assert (B * OH * OW + 31) // 32 >= 16, row
        assert mode in (B_CONV3, B_CONV3_S2, B_CONV3_UP)
    for rid, B, Cin, Cout, S, _ in wedges.S1:
        assert (S * S) % 8 == 0 and (B * S * S // 8 + 7) // 8 >= 8, rid
    assert any((r[1] * r[4] * r[4] // 8) % 8 for r in wedges.S1)              # a ragged last K-step
    assert any((r[2] * r[3]) % 4 for r in wedges.S1)                          # slab_reduce_scalar_kernel
