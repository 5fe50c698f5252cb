"""CPU: the C-ABI library builds for gfx950 and loads; without a GPU it refuses, and the product never reaches for the oracle.
(The headers against the binding tables and the exports: tests/test_cabi_headers.py.)"""
import ctypes
import os
import re

import pytest

from flatland_marl_amd import hip_backend as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    return hb.build()


def test_no_cpu_fallback(libpath):
    """without a GPU fl_create must fail loudly (no compute happens on the host)."""
    L = hb.lib()
    if L.fl_device_count() > 0:
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    rc = L.fl_create(1, 1, 4, 4, 0, ctypes.byref(h))
    assert rc == 2
    assert b"no HIP device" in L.fl_last_error()


def test_product_does_not_reference_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "flatland_marl_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".sh")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"import\s+oracle|from\s+oracle|fl_oracle|libfl_oracle|oracle/orc|orc\.", src), \
                    os.path.join(dirpath, f)
