"""CPU: every ctypes table against the header it binds (hip_backend.ABI: the ten headers of libflatland_hip.so; generators.ABI:
flatland_gen.h) -- the names in order, the return type and every parameter by type -- the libraries' exports, and the constants
Python restates against the headers' #defines and enumerators.  The reading of the headers is tests/cabi.py."""
import ctypes as C
import os
import re

import pytest

from flatland_marl_amd import generators as gen
from flatland_marl_amd import hip_backend as hb
from flatland_marl_amd import policy
from tests import cabi

COUNTS = {"flatland_hip.h": 41, "flatland_policy.h": 2, "flatland_train.h": 2, "flatland_policy_train.h": 5, "flatland_predict.h": 1,
          "flatland_wrappers.h": 2, "flatland_policy_bf16.h": 4, "flatland_policy_head_bf16.h": 4, "flatland_param_grads.h": 4,
          "flatland_ppo.h": 4, "flatland_gen.h": 5}
TABLES = {**hb.ABI, **gen.ABI}
RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "void": None, "const char *": C.c_char_p}
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "double": C.c_double}


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_every_header_has_a_table():
    assert sorted(os.listdir(cabi.INCLUDE)) == sorted(TABLES) and len(hb.ABI) == 10 and list(gen.ABI) == ["flatland_gen.h"]
    assert list(TABLES) == list(COUNTS)                                    # the headers' order is the one the counts were written in


@pytest.mark.parametrize("header", list(COUNTS))
def test_table_matches_the_header(header):
    decls, table = cabi.declarations(header), TABLES[header]
    assert [name for _, name, _ in decls] == list(table)
    assert len(decls) == COUNTS[header]
    if header in hb.ABI:
        assert hb.symbols(header) == tuple(table)
    for ret, name, params in decls:
        argtypes, restype = table[name]
        assert restype is RESTYPES[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (t, p) in enumerate(zip(argtypes, params)):
            k = cabi.kind(p)
            assert _is_pointer(t) if k == "pointer" else t is SCALARS[k], (name, i, p, t)


def test_the_type_check_tells_types_apart():
    """what the loop above rests on: the classifier's answers, its refusal of a type it does not know, and that the scalar kinds are
    different ctypes types (but for uint64_t and size_t, which are one where both are the 8-byte unsigned long)"""
    assert [cabi.kind(p) for p in ("fl_batch *h", "const float *const *params", "void *hip_stream", "int n", "const int n", "int32_t n",
                                   "uint32_t seed", "uint64_t thr", "size_t bytes", "double gamma")] \
        == ["pointer"] * 3 + ["int", "int", "int32_t", "uint32_t", "uint64_t", "size_t", "double"]
    for p in ("float x", "long n", "unsigned int n", "fl_batch h", "int"):
        with pytest.raises(ValueError):
            cabi.kind(p)
    distinct = [C.c_int, C.c_uint32, C.c_size_t, C.c_double]
    assert all(a is not b for i, a in enumerate(distinct) for b in distinct[i + 1:]) and not any(_is_pointer(t) for t in distinct)
    assert C.sizeof(C.c_uint64) == C.sizeof(C.c_size_t) == 8 and C.c_uint64 not in (C.c_int, C.c_uint32, C.c_double)
    assert _is_pointer(C.POINTER(C.c_void_p)) and _is_pointer(C.POINTER(C.c_int))


def test_no_name_is_in_two_groups():
    groups = list(TABLES.values()) + [hb.DEBUG_ABI]
    names = [name for g in groups for name in g]
    assert len(names) == len(set(names)) == 69 + 5 + 10
    assert hb.symbols() == tuple(name for h in hb.ABI for name in hb.ABI[h]) and len(hb.symbols()) == 69
    assert gen.SYMBOLS == tuple(gen.ABI["flatland_gen.h"])


def test_the_libraries_export_every_name():
    L, G = C.CDLL(hb.build()), C.CDLL(gen.build())
    for name in hb.symbols() + tuple(hb.DEBUG_ABI):
        assert hasattr(L, name), name
    for name in gen.SYMBOLS:
        assert hasattr(G, name), name
    bound = hb.bind(C.CDLL(hb.LIB_PATH), ["flatland_ppo.h"])              # the named group alone, on the library it was given
    assert bound.fl_gae.argtypes == hb.ABI["flatland_ppo.h"]["fl_gae"][0] and bound.fl_policy_head.argtypes is None
    assert hb.bind(C.CDLL(gen.LIB_PATH)).flg_generate.argtypes is None      # a library without the names: every one is skipped


def _int(header, name):
    return int(cabi.define(header, name), 0)


def test_constants_are_the_headers():
    hip = "flatland_hip.h"
    assert _int(hip, "FL_OK") == hb.FL_OK == 0
    errors = sorted(set(re.findall(r"\bFL_ERR_[A-Z_]+", cabi.text(hip))))
    assert {_int(hip, name): name for name in errors} == hb.ERR_NAMES and len(errors) == 6
    assert _int(hip, "FL_ACTION_ABSENT") == hb.ACTION_ABSENT
    assert _int(hip, "FL_STATE_COLS") == hb.STATE_COLS == len(hb.STATE_NAMES)
    assert _int(hip, "FL_AUX_COLS") == hb.AUX_COLS
    assert (_int(hip, "FL_STEP_AUTO_RESET"), _int(hip, "FL_STEP_FILTER_REQUIRED")) == (hb.FL_STEP_AUTO_RESET, hb.FL_STEP_FILTER_REQUIRED) == (1, 2)
    assert _int(hip, "FL_OBS_KEEP_TREE_ROWS") == hb.FL_OBS_KEEP_TREE_ROWS
    pol = "flatland_policy.h"
    assert _int(pol, "FL_POLICY_HEAD_NPARAMS") == hb.POLICY_HEAD_NPARAMS
    assert {None: _int(pol, "FL_POLICY_SELECT_NONE"), "soft": _int(pol, "FL_POLICY_SELECT_SOFT"),
            "hard": _int(pol, "FL_POLICY_SELECT_HARD")} == hb.POLICY_SELECT
    assert float(cabi.define(pol, "FL_POLICY_U_REFERENCE")) == hb.POLICY_U_REFERENCE
    assert _int("flatland_policy_train.h", "FL_POLICY_HEAD_SAVED_FLOATS") == hb.POLICY_SAVED_FLOATS == 4097
    assert _int("flatland_policy_train.h", "FL_POLICY_HEAD_ROW_FLOATS") == hb.POLICY_ROW_FLOATS == 9612
    assert _int("flatland_ppo.h", "FL_PPO_STATS") == hb.PPO_STATS == 8
    assert cabi.define("flatland_ppo.h", "FL_PPO_MAX_ROWS") == "(1 << 28)"
    assert _int("flatland_param_grads.h", "FL_PARAM_GRADS_MAX_SLICES") == hb.PARAM_GRADS_MAX_SLICES
    assert _int("flatland_param_grads.h", "FL_PARAM_GRADS_BLOCK") == policy.REDUCE_BLOCK
    with pytest.raises(KeyError):
        cabi.define(hip, "FL_NO_SUCH_CONSTANT")
