"""CPU: the table of observation-kernel cases (tests/obs_kernel_cases.py) against the launcher, and against itself.

The launcher's diagnostic fl_debug_obs_config_of (host code, no GPU) is asked what obs_pick_config chooses for every row it models -- the builder
alone or both builders, 31 nodes, every agent listed -- under the row's switches, in a child process per distinct switch set (the launcher reads
its switches once per process).  The answer must be the row's expectation, so a row cannot drift from the kernel it was written for without a GPU
noticing first.  The completeness tests are conditions on the table: every runtime-carving kernel the build instantiates, the split kernels with a
runtime-carving body and both values of every launcher option have a row."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from tests import obs_kernel_cases as cases
from tests import util

KEYS = ("nt", "lds", "tab", "nh", "wl", "tmask", "dual", "items", "merged", "compact", "fix")


def _ask(queries):
    """child: [(A, R, U, tall, max_branch, pred_depth, depth)] -> the diagnostic's answers"""
    from flatland_marl_amd import hip_backend as hb
    L = ctypes.CDLL(hb.LIB_PATH)       # plain dlopen: no torch, no GPU
    out = []
    for A, R, U, tall, max_branch, pred, depth in queries:
        buf = (ctypes.c_int * 11)()
        rc = L.fl_debug_obs_config_of(A, R, U, tall, max_branch, pred, depth, 30, buf)
        out.append(dict(zip(KEYS, buf)) if rc == 0 else None)
    return out


def _query(row):
    maps = cases.maps_of(row.recipe)
    A, R, U, tall = cases.sizes_of(maps)
    return [A, R, U, tall, 3 if row.recipe == "threeway" else 2, row.pred_depth, row.call[1] if row.call[0] == "both" else 0]


def _expected_answer(row):
    """what the diagnostic answers for a launch that reports row.expect (BatchedRailEnv.last_obs_launch): the fields both of them have.  The
    diagnostic knows no per-env sizes, so a split row is the runtime carving there (class 0: the condition of the split launch); for a launch class
    it answers the CLASS's carving, whose next-hop tables are the class's own choice, so `nh` is compared on the runtime carving only."""
    e = row.expect
    want = {"nt": e["nt"], "merged": (e["mode"] - 3) % 3 + 1 if e["mode"] >= 3 else 0, "fix": 0 if e["split"] else e["fix"]}
    for field, key in (("tab", "tab"), ("wl_bytes", "wl"), ("dual", "dual"), ("compact_t", "compact")):
        if field in e:
            want[key] = e[field]
    if "nh" in e and not e["fix"]:
        want["nh"] = int(e["nh"] or e.get("tab", 0))
    return want


def _check(row, got):
    assert got is not None, f"{row.id}: the launcher finds no configuration"
    e = row.expect
    want = _expected_answer(row)
    assert {k: got[k] for k in want} == want, (row.id, got)
    # the kernel: MODE from the builders of the call and `merged`, VAR from the tables and the work lists
    both = row.call[0] == "both"
    mode = (2 if both else 5) + got["merged"] if got["merged"] else (2 if both else 0)
    var = 1 if got["tab"] else 2 if got["wl"] == 0 else 0
    if not e["fix"] or e["split"]:
        assert (mode, var) == (e["mode"], e["var"]), (row.id, got)
    if "tmask" in e:
        assert got["tmask"] & 1 == e["tmask"], (row.id, got)
    if "own_filter" in e and got["merged"]:
        assert got["tmask"] >> 1 == e["own_filter"], (row.id, got)     # (the second set of time masks is the own-path filter's)
    if "items" in e:
        assert (got["items"] != 0) == bool(e["items"]), (row.id, got)
    assert got["lds"] <= (80 if got["merged"] == 3 else 160) * 1024, (row.id, got)


def test_the_launcher_chooses_what_every_modelled_row_expects():
    rows = [r for r in cases.ROWS if cases.cpu_modelled(r)]
    by_switches = {}
    for r in rows:
        by_switches.setdefault(json.dumps(r.switches, sort_keys=True), []).append(r)
    assert len(rows) >= 40 and len(by_switches) >= 20
    for key, group in by_switches.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("FL_OBS_")}
        child = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps([_query(r) for r in group])],
                               env=dict(env, PYTHONPATH=util.ROOT, **json.loads(key)), capture_output=True, text=True, timeout=120)
        assert child.returncode == 0, child.stderr[-2000:]
        answers = json.loads(child.stdout.splitlines()[-1])
        for r, got in zip(group, answers):
            _check(r, got)


def _build_units():
    """the observation-kernel units of csrc/build.sh: {"m": runtime-carving MODEs, "f": classes, "s": (class, second class) of the split kernels}"""
    text = open(os.path.join(util.ROOT, "flatland_marl_amd", "csrc", "build.sh")).read()
    units = re.search(r"^UNITS=\((.*?)\)", text, re.M | re.S).group(1).split()
    out = {"m": set(), "f": set(), "s": set()}
    for u in units:
        m = re.fullmatch(r"fl_obs_([mfs])(\d+)b?(?::(\d+))?", u)
        if m:
            out[m.group(1)].add((int(m.group(2)), int(m.group(3) or 0)) if m.group(1) == "s" else int(m.group(2)))
    return out


def test_every_runtime_carving_kernel_of_the_build_has_a_row():
    units = _build_units()
    assert units["m"] == set(cases.RUNTIME_MODES), "a runtime-carving unit was added to (or removed from) build.sh: the table needs its rows"
    got = {(r.expect["mode"], r.expect["var"]) for r in cases.ROWS if r.expect["fix"] == 0}
    assert got == cases.RUNTIME_KERNELS and len(cases.RUNTIME_KERNELS) == 26, sorted(cases.RUNTIME_KERNELS ^ got)
    # the runtime-carving body of every kernel is the runtime carving's own kernel too: no MODE hides behind a class
    assert {m for m, _ in got} == units["m"]


def test_the_split_kernels_with_a_runtime_body_have_a_row():
    units = _build_units()
    got = {(r.expect["fix"], r.expect["split"]) for r in cases.ROWS}
    assert cases.SPLIT_KERNELS <= got, got
    assert {k for k, k2 in units["s"] if k2 == 0} == {2, 3, 4, 9}, "a split unit was added to build.sh: the table (or the test that pins it) needs a row"
    for fix, split in cases.SPLIT_KERNELS:
        assert (fix, 0) in units["s"] and fix in cases.SPLIT_RCAP
        rows = [r for r in cases.ROWS if (r.expect["fix"], r.expect["split"]) == (fix, split)]
        # the runtime bodies of these two are k_obs<4,0> / k_obs<2,2>, and the batch has maps on both sides of the class's capacity
        assert {(r.expect["mode"], r.expect["var"]) for r in rows} == {{2: (4, 0), 4: (2, 2)}[fix]}
        for r in rows:
            rails = [int((m["grid"] != 0).sum()) for m in cases.maps_of(r.recipe)]
            assert min(rails) <= cases.SPLIT_RCAP[fix] < max(rails), (r.id, rails)


def test_every_option_appears_with_both_of_its_values():
    fields = set(cases.OPTION_VALUES)
    # every field of ObsOptions (csrc/fl_obs_layout.h) but items_cap, a capacity without a fallback of its own, is in the table -- a new field needs rows
    text = open(os.path.join(util.ROOT, "flatland_marl_amd", "csrc", "fl_obs_layout.h")).read()
    decl = re.search(r"struct ObsOptions \{ int ([^;]*); \};", text).group(1)
    assert {f.strip() for f in decl.split(",")} - {"items_cap"} <= fields, decl
    for field, values in cases.OPTION_VALUES.items():
        seen = {r.expect[field] for r in cases.ROWS if field in r.expect}
        assert set(values) <= seen, (field, values, seen)
    # threads 512 and 256 on each of the two-stage kernels
    for nt in (512, 256):
        assert {r.expect["mode"] for r in cases.ROWS if r.expect["nt"] == nt} >= {0, 1, 2}, nt
    assert {r.expect["mode"] for r in cases.ROWS if r.expect.get("dual") == 0 and r.call[0] == "both"}, "dual = 0 with both builders"
    assert any(r.handles is not None and r.call[0] == "cutils" for r in cases.ROWS) and any(r.handles is not None and r.call[0] == "tree" for r in cases.ROWS)


def test_rows_are_well_formed():
    from flatland_marl_amd.hip_backend import BatchedRailEnv, obs_switches
    assert 45 <= len(cases.ROWS) <= 80
    lists = cases.handle_lists()
    names = set(obs_switches())      # the library's table (csrc/fl_obs_switches.h): a misspelt switch would be a row that tests the default
    for r in cases.ROWS:
        assert r.recipe in cases.RECIPES and r.call[0] in ("cutils", "both", "tree"), r.id
        assert set(r.expect) <= set(BatchedRailEnv.LAUNCH_FIELDS) and {"mode", "var", "fix", "split", "nt"} <= set(r.expect), r.id
        assert set(r.switches) <= names, r.id
        if r.handles is not None:
            hs = lists[r.handles]
            assert r.recipe == "subset" and sorted(hs) == list(range(len(hs))) and 1 < len(hs) < 20, r.id     # a strict subset


if __name__ == "__main__":
    print(json.dumps(_ask(json.loads(sys.argv[1]))))
