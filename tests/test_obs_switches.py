"""CPU: the observation launcher's table of environment switches (csrc/fl_obs_switches.h) as the library lists it -- fl_debug_obs_switches, no GPU --
and what is held to it: DESIGN.md's paragraph about the switches, and the sources, which read the environment in that one place."""
import ctypes as C
import os
import re

from flatland_marl_amd import hip_backend as hb
from tests import util

CSRC = os.path.join(util.ROOT, "flatland_marl_amd", "csrc")
# a bin class replaces the batch's own options: the switch that asks for exact classes only, and those that shape the options
BINS = {"FL_OBS_NO_BINS", "FL_OBS_FORCE", "FL_OBS_NO_FB", "FL_OBS_NO_BK", "FL_OBS_NO_OWN_FILTER", "FL_OBS_NO_MERGE", "FL_OBS_ROUND16"}
CLASSES = {"FL_OBS_NO_FIX", "FL_OBS_NT", "FL_OBS_LDS_LIMIT", "FL_OBS_TSHIFT"}
VALUES = {"FL_OBS_NT": "int", "FL_OBS_TSHIFT": "int", "FL_OBS_ROUND16": "int", "FL_OBS_LDS_LIMIT": "bytes", "FL_OBS_FORCE": "keys"}


def test_the_table_as_the_library_lists_it():
    table = hb.obs_switches()
    assert len(table) == 21 and all(re.fullmatch(r"FL_OBS_[A-Z0-9_]+", name) for name in table)
    assert {name: kind for name, (kind, _) in table.items() if kind != "flag"} == VALUES
    assert {name for name, (_, out) in table.items() if out == "bins"} == BINS
    assert {name for name, (_, out) in table.items() if out == "classes"} == CLASSES
    assert {out for _, out in table.values()} == {"nothing", "bins", "classes"}
    assert "FL_OBS_NO_TAB" not in table      # retired: FL_OBS_FORCE="tab=0" is the same
    # the call: the bytes it needs, and a buffer too small for them is left alone
    fn = hb.lib().fl_debug_obs_switches
    need = fn(None, 0)
    small = C.create_string_buffer(b"x" * (need - 2), need - 1)
    assert fn(small, need - 1) == need and small.raw == b"x" * (need - 2) + b"\0"
    buf = C.create_string_buffer(need)
    assert fn(buf, need) == need and len(buf.value) == need - 1 and buf.value.decode().count("\n") == len(table)
    assert buf.value.decode().splitlines()[0] == "FL_OBS_VERBOSE flag nothing"


def test_designs_paragraph_names_the_tables_switches():
    text = open(os.path.join(util.ROOT, "DESIGN.md")).read()
    para = re.search(r"^\* Diagnostic environment switches of the launcher.*?(?=^\* )", text, re.M | re.S).group(0)
    table = hb.obs_switches()
    assert set(re.findall(r"FL_OBS_[A-Z0-9_]+", para)) == set(table)
    bins = re.search(r"The bin classes\s+are ruled out by:([^.]*)\.", para).group(1)
    assert set(re.findall(r"FL_OBS_[A-Z0-9_]+", bins)) == {name for name, (_, out) in table.items() if out == "bins"} == BINS
    classes = re.search(r"Every\s+launch class, split kernels included, is ruled out by:(.*?)\)\.", para, re.S).group(1)
    assert set(re.findall(r"FL_OBS_[A-Z0-9_]+", classes)) == {name for name, (_, out) in table.items() if out == "classes"}
    readme = open(os.path.join(util.ROOT, "README.md")).read()
    assert "OBS_SWITCH_TABLE" in re.search(r"To add a row for a new unit or option:.*", readme).group(0)


def test_the_environment_is_read_in_one_place():
    """the launcher asks obs_switches(); no switch's name is a string anywhere but in the table's rows"""
    def code(name):
        return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())
    header = code("fl_obs_switches.h")
    assert "getenv" not in code("fl_obs.hip") and header.count("getenv") == 1 and "getenv(r.name)" in header
    rows = re.search(r"OBS_SWITCH_TABLE\[\] = \{(.*?)\n\};", header, re.S).group(1)
    assert sorted(re.findall(r'\{"(FL_OBS_[A-Z0-9_]+)", OBS_SW_[A-Z]+, &ObsSwitches::', rows)) == sorted(hb.obs_switches())
    assert '"FL_OBS_' not in header.replace(rows, "")
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".h")) and name != "fl_obs_switches.h":
            assert not re.search(r'"FL_OBS_[A-Z0-9_]+"', code(name)), name
    assert "fl_obs_switches.h" not in "".join(code(n) for n in os.listdir(CSRC) if n.endswith(".h") or n == "fl_obs_unit.hip")      # host only
