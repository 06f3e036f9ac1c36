"""Every instantiation of the six persistent / grouped split-precision kernel families in the built library is reached by a case of
test_persistent_edges_gpu.py: the instantiations are read from the library's host stubs (nm -C), the cases' expected names come from
the same pure functions the GPU test checks against the names ops records.  A new instantiation without a case fails here."""
import re
import shutil
import subprocess

import pytest

from villandiffusion_amd import lib
import test_persistent_edges_gpu as edges

FAMILIES = tuple(edges.ARITY)


def library_instantiations():
    out = subprocess.check_output([shutil.which("nm") or "nm", "-C", lib.LIB_PATH], text=True)
    names = set()
    for m in re.finditer(r"__device_stub__(\w+)<([^>]*)>", out):
        if m.group(1) in FAMILIES:
            names.add(edges.normalise(f"{m.group(1)}<{m.group(2)}>"))
    return names


def test_normalise_adds_defaults_and_strips_suffixes():
    assert edges.normalise("conv3_k32p_kernel<32, 2, true, true, false, false>@64") == "conv3_k32p_kernel<32, 2, true, true, false, false, false>"
    assert edges.normalise("wgrad1x1_wide_group_kernel(+group_reduce)") == "wgrad1x1_wide_group_kernel<false>"
    assert edges.normalise("wgrad_k32_group_kernel<16, 2>(+group_reduce)") == "wgrad_k32_group_kernel<16, 2, false>"
    assert edges.normalise("gemm1x1_k32p_kernel<true, 128>") == "gemm1x1_k32p_kernel<true, 128, false>"


def test_every_instantiation_has_an_edge_case():
    if shutil.which("nm") is None:
        pytest.fail("nm (binutils) is needed to read the library's symbols")
    built = library_instantiations()
    covered = edges.all_expected_names()
    per_family = {f: sum(1 for n in built if n.startswith(f + "<")) for f in FAMILIES}
    print(f"[census] {len(built & covered)} of {len(built)} instantiations covered: {per_family}")
    assert built - covered == set(), f"instantiations without an edge case: {sorted(built - covered)}"
    assert covered - built == set(), f"edge cases expect instantiations the library does not have: {sorted(covered - built)}"
