"""The device-resident prior's entry points (plba_marginalize_to_prior, plba_get_prior) on the surface: declared by the header, bound by
the Python layer as product-only entries (the CPU oracle restates the reference, which keeps no device state), exported by the library."""
import os
import re
import subprocess

import pytest

NAMES = ("marginalize_to_prior", "get_prior")


def test_header_declares_both_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "plba.h")).read()
    assert re.search(r"int\s+plba_marginalize_to_prior\s*\(\s*plba_problem\*\s*p\s*,\s*int\s+first_kf\s*,\s*int\s+\w+\s*,\s*int32_t\*\s*out3\s*\)", h)
    assert re.search(r"int\s+plba_get_prior\s*\(\s*plba_problem\*\s*p\s*,\s*plba_prior\*\s*out\s*\)", h)


def test_signatures_and_product_only(pkg):
    for n in NAMES:
        assert n in pkg.abi.SIGNATURES, n
        assert n in pkg.abi.PRODUCT_ONLY, n


@pytest.mark.parametrize("name", NAMES)
def test_library_exports(hip_lib_path, name):
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_path], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT plba_%s$" % name, out, re.M), name
