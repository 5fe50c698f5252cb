"""CPU: the whole launch plan of the observation launcher -- kernel MODE / VAR, launch class, split kind and its second class, threads, LDS
bytes, the accepted options, and how many envs run the class's body -- for batches that fl_debug_obs_config_of cannot describe: envs of
different rail cells (the split launches), FL_OBS_KEEP_TREE_ROWS, a handle subset, larger trees, the upstream builder alone.  The library's
hook fl_debug_obs_plan runs the host half of fl_launch_obs_* up to the enqueue (csrc/fl_obs.hip: obs_plan_*), so no GPU is needed.
tests/obs_plan_table.json is the launcher's own recorded output (tools/obs_plan_sweep.py --table), captured before the class table of
csrc/fl_obs_layout.h replaced the per-class specialisations: a change that is meant to keep every choice leaves every row as it is."""
import collections
import ctypes
import json
import os

import pytest

from flatland_marl_amd import hip_backend as hb

WORDS = 25   # FL_OBS_LAUNCH_WORDS (csrc/fl_obs.h): [0] MODE [1] VAR [2] class [3] split [4] second class of a split-2 kernel [5] threads [6] LDS bytes ...
KINDS = {"cutils": 0, "both": 1, "tree": 2}
FIELDS = ("kind", "A", "U", "tall", "max_branch", "max_nodes", "pred_depth", "max_depth", "tree_pred", "keep_mode", "label", "n_cu")


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(os.path.dirname(__file__), "obs_plan_table.json")) as f:
        return json.load(f)


def _plan(L, row):
    cells = [r for r, n in row["levels"] for _ in range(n)]
    R = (ctypes.c_int * len(cells))(*cells)
    rec, n_fit = (ctypes.c_int * WORDS)(), ctypes.c_int()
    args = [KINDS[row["kind"]]] + [row[k] for k in FIELDS[1:]]
    rc = L.fl_debug_obs_plan(*args, R, len(cells), rec, ctypes.byref(n_fit))
    return [rc, n_fit.value] + list(rec)


def test_every_recorded_launch_plan_is_still_the_launchers_choice(table):
    L = ctypes.CDLL(hb.LIB_PATH)       # plain dlopen: no torch, no GPU
    wrong = [(row, got) for row, got in ((row, _plan(L, row)) for row in table) if got != row["out"]]
    assert not wrong, "%d of %d plans differ, the first: %r" % (len(wrong), len(table), wrong[0])


def test_the_recorded_plans_cover_every_class_and_split_kind(table):
    """what keeps the table from going hollow: every launch class is some row's choice, and so is every kind of split launch"""
    ok = [row for row in table if row["out"][0] == 0]
    assert len(table) >= 300 and len(ok) >= 300
    assert {row["out"][4] for row in ok} >= set(range(1, 22))
    split = collections.Counter((row["out"][5], row["out"][4], row["out"][6]) for row in ok if row["out"][5])
    assert set(split) == {(1, 2, 0), (1, 3, 0), (1, 4, 0), (1, 9, 0), (2, 4, 14), (2, 9, 19)}, split
    # a split row serves a part of its batch (none of its envs, or all of them, is no split), and at the half-fit turning point (both builders,
    # 80 agents, depth 3, eight envs of 232 / 233 rail cells) three envs that fit class 2 leave the batch to the bin class 13, four take the split
    assert all(0 < row["out"][1] < sum(n for _, n in row["levels"]) for row in ok if row["out"][5])
    half = {row["levels"][0][1]: row["out"][4:6] for row in ok
            if (row["kind"], row["A"], row["max_depth"], row["keep_mode"]) == ("both", 80, 3, 0) and [r for r, _ in row["levels"]] == [232, 233]}
    assert half == {3: [13, 0], 4: [2, 1]}, half
    # FL_OBS_KEEP_TREE_ROWS: the host takes none of classes 1, 5 and 11 (and a handle subset no class at all)
    assert not [row for row in ok if row["keep_mode"] and row["kind"] == "both" and row["out"][4] in (1, 5, 11)]
    assert [row for row in ok if row["keep_mode"] and row["kind"] == "both" and row["A"] <= 32 and row["out"][4] == 0]
    assert [row for row in ok if row["label"] and row["kind"] == "cutils"] and not [row for row in ok if row["label"] and row["out"][4]]
    assert all(row["out"][2 + 24] == (row["label"] if row["kind"] != "both" else 0) for row in ok)
