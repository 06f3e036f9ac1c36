"""Every instantiation of the persistent / grouped split-precision kernel families (six: test_persistent_edges_gpu.py) and of the remaining
split-precision weight gradients (three: wgrad_bx3_group_kernel, wgrad_bx3_kernel, wgrad_k32_kernel, test_wgrad_edges_gpu.py) in the built
library is reached by an edge case: the instantiations are read from the library's host stubs (nm -C), the cases' expected names come from
the same pure functions the GPU tests check against the names ops records.  A new instantiation without a case fails here.  The tables of
test_wgrad_edges_gpu.py are also held to the planner regimes they were sized for."""
import re
import shutil
import subprocess

import pytest

from villandiffusion_amd import lib, ops
from villandiffusion_amd.lib import B_CONV3, B_CONV3_S2, B_CONV3_UP
import test_persistent_edges_gpu as edges
import test_wgrad_edges_gpu as wedges

FAMILIES = tuple(edges.ARITY)


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


def test_the_recorded_single_launch_names_mirror_the_dispatch():
    """ops.wgrad_single_name against the names the 3x3 single-launch cases expect (written out in their table)."""
    for row in wedges.SW:
        _, name, mode, _, _, _, _, OW, _, _ = row
        assert edges.normalise(ops.wgrad_single_name(OW, mode)) == edges.normalise(name), row
    assert ops.wgrad_single_name(128, B_CONV3_S2) == "wgrad_bx3_kernel<32, 4, true>"
    assert ops.wgrad_single_name(32, B_CONV3_S2) == "wgrad_bx3_kernel<32, 4>"
    assert ops.wgrad_single_name(32, B_CONV3_UP) == "wgrad_k32_kernel<32, 2>"
    assert ops.wgrad_single_name(4, B_CONV3) == "wgrad_bx3_kernel<4, 0>"


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
