"""CPU side of the constructed observation states (tests/obs_state_cases.py; fixtures tests/golden/obs_states_<map>_<set>_<k>.npz from the real
reference's two tree builders, oracle/refharness/capture_obs_states.py): every row of the table is named by a case and reached, judged on what
the reference returned -- its value at the pin differs from the control's and has the row's kind; for the time rows the builder's own
predicted_pos / predicted_dir show which of the three times its if / elif / elif took; for the long-list rows the number of predicted stays on
the cell exceeds the chunk constants of csrc/fl_obs_layout.h -- and the oracle set to the state (orc_set_state) equals the reference in every
array of both builders, without a tolerance."""
import os
import re

import numpy as np
import pytest

from oracle import orc
from tests import handmaps, obs_state_cases as oc, util

LAYOUT = os.path.join(util.ROOT, "flatland_marl_amd", "csrc", "fl_obs_layout.h")


@pytest.fixture(scope="module")
def fixtures():
    return {s: oc.load_set(*s) for s in oc.SETS}


def layout_constants():
    text = open(LAYOUT).read()
    return {k: int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("CF_CHUNK_LDS", "CF_CHUNK_HBM", "CF_FIRST_HBM", "CF_DIRECT")}


def test_the_modules_data_is_what_it_says(fixtures):
    real = [c for c in oc.CASES if c["control_of"] is None]
    assert len(real) >= 40 and all(c["doc"] and c["rows"] for c in real)
    for (m, s) in oc.SETS:
        grid = oc.MAPS[m]()["grid"]
        A = len(oc.AGENTS[m][s])
        assert grid.shape[0] <= 12 and grid.shape[1] <= 12 and A == (8 if s == "small" else 24)
        assert all(handmaps.known_cell_type(v) for v in grid.ravel())      # the attribute rows are defined everywhere
        fx = fixtures[(m, s)]
        assert np.array_equal(fx["grid"], grid) and fx["grid"].dtype == np.uint16      # the builders reproduce the reference env's rail
        assert fx["names"] == [n for part in oc.parts_of(m, s) for n in part] == [c["name"] for c in oc.CASES if (c["map"], c["set"]) == (m, s)]
        for v in oc.VARIANTS[(m, s)]:
            st = oc.static_of(m, s, v)
            assert len(st["speed"]) == A and all(int(1 / sp) - 1 <= 63 for sp in st["speed"])      # FL_MAX_SPEED_COUNT
    for c in oc.CASES:
        fx = fixtures[(c["map"], c["set"])]
        assert np.array_equal(fx[c["name"] + "/state"], c["state"]) and np.array_equal(fx[c["name"] + "/aux"], c["aux"]), c["name"]
        if c["control_of"] is not None:      # ONE agent's row differs from its case's
            assert int((c["state"] != oc.BY_NAME[c["control_of"]]["state"]).any(axis=1).sum()) == 1, c["name"]
    # the search behind the time rows: float32 truncates one lower at eleven speeds, at every walk length; float64 is the exact quotient
    # everywhere; 0.3 and 0.7 agree in all three
    t = oc.TRUNCATIONS
    assert sorted({round(1 / s) for s, *_ in t}) == [7, 13, 14, 15, 26, 28, 30, 52, 56, 60, 63] and len(t) == 11 * oc.MAX_WALK
    assert all(v32 == v64 - 1 and v64 == exact for _, _, v32, v64, exact in t)
    assert (1 / 7, 1, 6, 7, 7) in t


def _pin_values(fx, case, p):
    key = oc.pin_key(p)
    col = oc.COL[oc.TABLE[p["row"]]["col"]]
    return fx[case["name"] + "/" + key][p["agent"]][:, col], fx[p["control_name"] + "/" + key][p["agent"]][:, col]


def _check_chain(fx, case, p, spec, consts):
    st = oc.static_of(case["map"], case["set"], case["variant"])
    P = p["param"] if p["builder"] == "py" else 30
    pos, dirs = fx["%s/pred_pos_p%d" % (case["name"], P)], fx["%s/pred_dir_p%d" % (case["name"], P)]
    ch = oc.chain_of(st["grid"], pos, dirs, case["state"][:, 3], p["agent"], st["speed"][p["agent"]], p["at"])
    w = "%s %s at %s: %s" % (case["name"], p["row"], p["at"], ch)
    assert ch is not None and ch["branch"] == spec["branch"], w
    others = [k for k, a in enumerate(ch["agents"]) if a != p["agent"]]
    if "cond" in spec:
        assert any(ch["cond"][k] for k in others) == spec["cond"], w
    if "cond_at_pt" in spec:      # what flatland_cutils reads differs from the direction at the matching time
        assert any(ch["cond_at_pt"][k] for k in others) == spec["cond_at_pt"] != spec["cond"], w
    if "hidden" in spec:
        assert ch["later"][spec["hidden"]], w
    if spec.get("own"):
        assert p["agent"] in ch["agents"], w
    if spec.get("done"):
        assert any(case["state"][a, 3] == oc.DONE for a in ch["agents"]), w
    if spec.get("pt_is_last"):
        assert ch["pt"] == ch["T"] - 1 and ch["times"][2] == ch["pt"], w
    if spec.get("long"):
        n = oc.visits_of(pos, p["at"][0:2], st["grid"].shape[1])
        assert n > max(consts.values()), "%s: %d stays on the cell, the constants are %s" % (w, n, consts)


def test_every_table_row_is_reached_by_a_case_that_names_it(fixtures):
    """Every row of obs_state_cases.TABLE is named by a case, and every pin of every case holds on what the reference returned: at the
    pin's node the value of the row's column differs between case and control and has the row's kind; the time rows took the branch of
    the reference's if / elif / elif that they name.  No row is waived."""
    consts = layout_constants()
    assert consts["CF_CHUNK_LDS"] >= consts["CF_CHUNK_HBM"] >= 1
    claimed = {}
    for case in oc.CASES:
        fx = fixtures[(case["map"], case["set"])]
        A = len(case["state"])
        pinned = set()
        for p in case["pins"]:
            row = oc.TABLE[p["row"]]
            w = "case %s does not reach %s (%s, agent %d, node %s)" % (case["name"], p["row"], p["builder"], p["agent"], p["node"])
            assert p["builder"] in row["builders"] and p["node"] is not None, w
            assert p["param"] in (case["py_pred"] if p["builder"] == "py" else case["cu_pred"]), w
            v, c = _pin_values(fx, case, p)
            kind, arg = oc.kind_of(p["row"], p["builder"])
            if kind == "never":      # flatland_cutils never fills location_has_target: inf at every node (0 at the root) where upstream has a distance
                up = fx[case["name"] + "/py_d3_p30"][p["agent"]][:, oc.COL["other_target"]]
                assert np.isfinite(up[1:]).any() and set(v[1:].tolist()) <= {-1.0} and v[0] == 0 and set(c[1:].tolist()) <= {-1.0}, w
            elif kind == "reoriented":      # the only branch of the root is its FORWARD branch (row 22 of the dense tree), not the one behind it
                assert np.isfinite(v[22]) and np.isneginf(v[[1, 43, 64]]).all() and v[22] != c[22], w
            else:
                assert v[p["node"]] != c[p["node"]] and oc.KINDS[kind](p["builder"], v[p["node"]], c[p["node"]], A, arg), w + ": %s vs %s" % (v[p["node"]], c[p["node"]])
            if row["chain"] is not None and (p["builder"] == "py" or "py" not in row["builders"]):
                assert p["at"] is not None, w
                _check_chain(fx, case, p, row["chain"], consts)
            pinned.add((p["row"], p["builder"]))
        for r in case["rows"]:
            for b in oc.TABLE[r]["builders"]:
                assert (r, b) in pinned or any((r, b) in {(q["row"], q["builder"]) for q in o["pins"]} for o in oc.CASES if r in o["rows"]), (case["name"], r, b)
            assert any(q["row"] == r for q in case["pins"]), "case %s names %s without a pin" % (case["name"], r)
            claimed.setdefault(r, []).append(case["name"])
    assert sorted(claimed) == sorted(oc.TABLE), sorted(set(oc.TABLE) - set(claimed))
    # every row is pinned in every builder it is for
    for r, row in oc.TABLE.items():
        have = {q["builder"] for c in oc.CASES for q in c["pins"] if q["row"] == r}
        assert have == set(row["builders"]), (r, have)


def test_chain_of_is_the_if_elif_elif():
    """the recomputation the reach test relies on, on a hand-made horizon: 3 agents, one cell"""
    grid = oc.MAPS["yard"]()["grid"]
    Wd = grid.shape[1]
    cell = 4 * Wd + 4      # (4, 4): column-major on the width
    pos = np.full((6, 3), -1, dtype=np.int32)
    dirs = np.zeros((6, 3), dtype=np.int32)
    states = np.array([oc.MOVING] * 3)
    pos[2, 0] = cell; dirs[2, 0] = oc.W      # the walker itself at pt
    pos[1, 1] = cell; dirs[1, 1] = oc.E      # agent 1 at pt - 1, head-on
    pos[3, 2] = cell; dirs[3, 2] = oc.E      # agent 2 at pt + 1
    ch = oc.chain_of(grid, pos, dirs, states, 0, 1.0, (4, 4, oc.W, 2))
    assert ch["branch"] == 1 and ch["agents"] == [1] and ch["cond"] == [True] and ch["later"] == {2: True}
    pos[2, 2] = cell; dirs[2, 2] = oc.W      # agent 2 also at pt, following: the first branch, without the condition
    ch = oc.chain_of(grid, pos, dirs, states, 0, 1.0, (4, 4, oc.W, 2))
    assert ch["branch"] == 0 and ch["agents"] == [0, 2] and ch["cond"] == [False, False] and ch["later"] == {1: True, 2: True}
    states[2] = oc.DONE
    assert oc.chain_of(grid, pos, dirs, states, 0, 1.0, (4, 4, oc.W, 2))["cond"] == [False, True]
    assert oc.chain_of(grid, pos, dirs, states, 0, 0.25, (4, 4, oc.W, 2)) is None      # t = 8 lies beyond a horizon of 6
    assert oc.visits_of(pos, (4, 4), Wd) == 3      # (agent 2 stays from t = 2 to 3: one item)


CUTILS = ("attr", "forest", "adjacency", "node_order", "edge_order", "valid")
PROPS = ("p_dist_target", "p_deadlocked", "p_ready")


@pytest.mark.parametrize("set_id", ["%s_%s" % s for s in oc.SETS])
def test_oracle_set_to_the_state_equals_the_reference(fixtures, set_id):
    (m, s) = next(x for x in oc.SETS if "%s_%s" % x == set_id)
    fx = fixtures[(m, s)]
    for c in (c for c in oc.CASES if (c["map"], c["set"]) == (m, s)):
        o = orc.OracleEnv(oc.static_of(m, s, c["variant"]))
        o.set_state(c["state"], c["aux"], 0, False)
        assert np.array_equal(o.state(), c["state"])
        for P in c["py_pred"]:
            for depth in (2, 3):
                exp = fx["%s/py_d%d_p%d" % (c["name"], depth, P)]
                got = o.obs_pytree(depth, P)
                assert got.dtype == exp.dtype and np.array_equal(got, exp), "%s depth-%d tree, predictor depth %d: %s" % (
                    c["name"], depth, P, np.argwhere(got != exp)[:4].tolist())
        for P in c["cu_pred"]:
            o.set_state(c["state"], c["aux"], 0, False)      # (a fresh builder per depth in the capture: no deadlock is carried over)
            got = o.obs_cutils(31, P)
            for k in CUTILS:
                exp = fx["%s/cu_p%d_%s" % (c["name"], P, k)]
                assert got[k].dtype == exp.dtype and np.array_equal(got[k], exp), "%s flatland_cutils %s, pred_depth %d: %s" % (
                    c["name"], k, P, np.argwhere(got[k] != exp)[:4].tolist())
            for col, k in enumerate(PROPS):
                assert np.array_equal(got["props"][:, col], fx["%s/cu_p%d_%s" % (c["name"], P, k)]), "%s %s" % (c["name"], k)
