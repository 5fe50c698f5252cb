"""CPU: the library's layout tables (csrc/fl_policy_layout.h: the arrays of saved_dev and rows_dev, the head's 38 parameters) read
through fl_debug_policy_layout -- which runs no HIP call -- against hip_backend's literal tables and the public header's constants."""
import ctypes as C

import pytest

from flatland_marl_amd import hip_backend as hb
from tests import cabi

SAVED, ROWS, PARAMS = 0, 1, 2


@pytest.fixture(scope="module")
def layout():
    hb.build()
    fn = hb._sym("fl_debug_policy_layout")

    def read(table):
        """[(name, a, b)] of every entry of `table`"""
        out = []
        for i in range(fn(table, -1, None, 0, None, None)):
            name, a, b = C.create_string_buffer(32), C.c_int(-1), C.c_int(-1)
            assert fn(table, i, name, len(name), C.byref(a), C.byref(b)) == 0, (table, i)
            out.append((name.value.decode(), a.value, b.value))
        return out
    return fn, read


def _running(widths):
    return [sum(widths[:i]) for i in range(len(widths))]


@pytest.mark.parametrize("table,want,total,define", ((SAVED, hb.POLICY_SAVED_LAYOUT, 4097, "FL_POLICY_HEAD_SAVED_FLOATS"),
                                                      (ROWS, hb.POLICY_ROWS_LAYOUT, 9612, "FL_POLICY_HEAD_ROW_FLOATS")))
def test_arrays_are_the_python_tables(layout, table, want, total, define):
    got = layout[1](table)
    assert [(n, k) for n, k, _ in got] == list(want)                          # names and widths, in order
    assert [b for _, _, b in got] == _running([k for _, k in want])           # the floats a row before each array
    assert got[-1][1] + got[-1][2] == total == int(cabi.define("flatland_policy_train.h", define))


def test_array_counts():
    assert len(hb.POLICY_SAVED_LAYOUT) == 11 and len(hb.POLICY_ROWS_LAYOUT) == 36


def test_parameters_are_the_python_table(layout):
    got = layout[1](PARAMS)
    assert len(got) == hb.POLICY_HEAD_NPARAMS == 38
    assert [(o, k) if k else (o,) for _, o, k in got] == list(hb.POLICY_HEAD_PARAM_SHAPES)
    assert all(name in ("bf16", "") for name, _, _ in got)
    assert tuple(i for i, (name, _, _) in enumerate(got) if name == "bf16") == hb.POLICY_HEAD_BF16_MATRICES
    assert sum(o * (k + 1) for _, o, k in got if k) == 1698694                # the float64 partials of a slice (tests/test_param_grads.py)


def test_count_query_and_refusals(layout):
    fn, _ = layout
    name, a, b = C.create_string_buffer(32), C.c_int(7), C.c_int(7)
    args = (name, len(name), C.byref(a), C.byref(b))
    for table, count in ((SAVED, 11), (ROWS, 36), (PARAMS, 38)):
        assert fn(table, -1, None, 0, None, None) == count and fn(table, -5, *args) == count
        assert fn(table, count - 1, *args) == 0
        assert fn(table, count, *args) == -1 and fn(table, 1 << 20, *args) == -1
    for table in (-1, 3, 99):
        assert fn(table, -1, *args) == -1 and fn(table, 0, *args) == -1
    a.value = b.value = 7
    assert fn(SAVED, 0, None, 0, C.byref(a), C.byref(b)) == -1 and fn(SAVED, 0, name, len(name), None, None) == -1     # nowhere to write
    assert (a.value, b.value) == (7, 7)
    short = C.create_string_buffer(3)                                         # a short name buffer: cut, still terminated
    assert fn(ROWS, 0, short, len(short), C.byref(a), C.byref(b)) == 0 and short.value == b"at" and (a.value, b.value) == (256, 0)
