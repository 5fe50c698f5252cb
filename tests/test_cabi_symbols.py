"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/flatland_hip.h declares."""
import ctypes
import os
import re

import pytest

from flatland_marl_amd import hip_backend as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    return hb.build()


def test_header_symbols_exported(libpath):
    hdr = open(os.path.join(ROOT, "include", "flatland_hip.h")).read()
    declared = set(re.findall(r"\b(fl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(hb.SYMBOLS), declared ^ set(hb.SYMBOLS)
    L = ctypes.CDLL(libpath)
    for s in declared:
        assert hasattr(L, s), s


def test_binding_matches_the_header_declarations(libpath):
    """every function of the header: the binding passes as many arguments as the header declares parameters (a short list would
    truncate a pointer silently) and reads the declared return type"""
    hdr = open(os.path.join(ROOT, "include", "flatland_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    decls = re.findall(r"([A-Za-z_][A-Za-z_0-9 ]*?[ *]+)(fl_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert len(decls) == 41 and {name for _, name, _ in decls} == set(hb.SYMBOLS)
    restypes = {"const char *": ctypes.c_char_p, "size_t": ctypes.c_size_t, "double": ctypes.c_double, "void": None, "int": ctypes.c_int}
    L = hb.lib()
    n_not_int = 0
    for ret, name, params in decls:
        params = params.strip()
        n = 0 if params == "void" else len(params.split(","))
        fn = getattr(L, name)
        assert len(fn.argtypes) == n, (name, len(fn.argtypes), n)
        ret = " ".join(ret.split())
        assert fn.restype is restypes[ret], (name, ret, fn.restype)
        n_not_int += ret != "int"
    assert n_not_int == 4


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
