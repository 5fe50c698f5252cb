"""GPU parity of the tree-observation kernels (k_obs<MODE, VAR>: csrc/fl_obs_passb.h, fl_obs_trees.h, fl_obs_body.h) with the REAL reference's two
builders on constructed agent states: tests/obs_state_cases.py lists them, tests/golden/obs_states_<map>_<set>_<k>.npz holds what the reference
returned (oracle/refharness/capture_obs_states.py), tests/test_obs_states.py (CPU) asserts that they reach the branches they exist for.

One batch per (map, agent set): its cases AND their controls are the envs (B = 76 for the yard's eight agents; 6 for its crowd of 24), every env
set to its state with fl_set_state.  obs_cutils (per predictor depth the cases name), obs_tree(2 | 3, depth) and obs_both are compared with the
FIXTURE -- not the oracle -- bit for bit, for the envs whose case names the depth; check() afterwards.

Pass B exists in several compiled forms, so the same comparison runs under the switch sets of SWITCH_SETS (the rows of tests/obs_kernel_cases.py
that change pass B), each in ONE fresh child process (the launcher reads its switches once per process), one after the other.  Every child
asserts from last_obs_launch() that the option it exists for took effect on these small shapes; all of them do (A = 8 or 24, 20 or 19 rail
cells), so no set had to be replaced.  A child that fails is not run again; one that ends with a signal or at its time limit fails the test with
its stderr, and the children after it are not started (they fail, saying so)."""
import json
import sys
import time

import numpy as np
import pytest

from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw
from tests import util

pytestmark = pytest.mark.gpu
CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"), ("edge_order", "edge_order"),
          ("valid_actions", "valid"))
PROPS = ("p_dist_target", "p_deadlocked", "p_ready")
CHILD_TIMEOUT = 60      # a guard, not a measurement (a child takes a few seconds: four small batches, some forty launches)

# id -> (the child's environment, what last_obs_launch() must report after obs_cutils() and after obs_both(): field -> value, or
# ("ne", value) / ("ge", value); a pair of dicts: (after obs_cutils, after obs_both))
_MERGED = {"mode": ("ge", 3), "nt": 1024, "own_filter": 1, "tmask": 1, "tshift": ("ne", 3), "wl_bytes": ("ge", 1)}
SWITCH_SETS = {
    "none": ({}, dict(_MERGED, fix=("ne", 0))),                                            # the launch classes these shapes fall into
    "nofix": ({"FL_OBS_NO_FIX": "1"}, dict(_MERGED, fix=0)),                                # the runtime carving of the one-pass kernels
    # conflicts handled in place (no time masks, no conflict work list), items in HBM scratch
    "notmask": ({"FL_OBS_FORCE": "tmask=0,items=0", "FL_OBS_NO_SPLIT": "1"}, {"tmask": 0, "items": 0, "fix": 0}),
    "noown": ({"FL_OBS_NO_OWN_FILTER": "1"}, {"own_filter": 0, "tmask": 1, "mode": ("ge", 3)}),
    "nomerge": ({"FL_OBS_NO_MERGE": "1"}, ({"mode": 0}, {"mode": 2})),                       # the two-stage kernels
    "wl0": ({"FL_OBS_FORCE": "wl=0"}, {"wl_bytes": 0, "var": 2, "wl_head": ("ge", 4096)}),   # work lists in HBM scratch with an LDS head
    "wl0-nohead": ({"FL_OBS_FORCE": "wl=0", "FL_OBS_NO_WL_HEAD": "1"}, {"wl_bytes": 0, "var": 2, "wl_head": 0}),
    "tshift3": ({"FL_OBS_TSHIFT": "3"}, {"tshift": 3, "tmask": 1}),
    "round16": ({"FL_OBS_ROUND16": "2"}, {"nt": 512, "mode": ("ge", 3)}),                   # rounds of 16 agents, two workgroups a CU
}


def _matches(record, expect):
    bad = {}
    for k, v in expect.items():
        ok = (record[k] != v[1] if v[0] == "ne" else record[k] >= v[1]) if isinstance(v, tuple) else record[k] == v
        if not ok:
            bad[k] = (record[k], v)
    return bad


def _run(set_id):
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    expect = SWITCH_SETS[set_id][1]
    exp_alone, exp_both = expect if isinstance(expect, tuple) else (expect, expect)
    n_env = n_launch = 0
    for (m, s) in oc.SETS:
        cases = [c for c in oc.CASES if (c["map"], c["set"]) == (m, s)]
        fx = oc.load_set(m, s)
        B = len(cases)
        env = BatchedRailEnv([oc.static_of(m, s, c["variant"]) for c in cases])
        assert (env.A, env.H <= 12, env.W <= 12) == (len(oc.AGENTS[m][s]), True, True)
        states, aux = np.stack([c["state"] for c in cases]), np.stack([c["aux"] for c in cases])

        def inject():      # (a flatland_cutils launch leaves its deadlock flags in the env; the reference's builder was fresh for every call)
            env.set_state(states, aux, np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8))

        inject()
        util.same(env.state()[0], states, f"{m}/{s} rows read back after the injection", dtype=True)
        tag = f"[{set_id}] {m}/{s}"

        def compare_cutils(got, P, how):
            got = {k: v.cpu().numpy() for k, v in got.items()}
            for b, c in enumerate(cases):
                if P in c["cu_pred"]:
                    for g, e in CUTILS:
                        util.same(got[g][b], fx["%s/cu_p%d_%s" % (c["name"], P, e)], f"{tag} {c['name']} {how} pred_depth {P} {g}", dtype=True)
                    for col, k in enumerate(PROPS):
                        util.same(got["props"][b][:, col], fx["%s/cu_p%d_%s" % (c["name"], P, k)], f"{tag} {c['name']} {how} pred_depth {P} {k}", dtype=True)

        def compare_tree(tree, depth, P, how):
            tree = tree.cpu().numpy()
            for b, c in enumerate(cases):
                if P in c["py_pred"]:
                    util.same(tree[b], fx["%s/py_d%d_p%d" % (c["name"], depth, P)], f"{tag} {c['name']} {how} depth-{depth} tree, predictor depth {P}", dtype=True)

        for P in sorted({P for c in cases for P in c["cu_pred"]}, reverse=True):
            inject()
            env.pred_depth = P
            compare_cutils(env.obs_cutils(), P, "obs_cutils")
            record = env.last_obs_launch()
            if P == 500:      # (the launch classes are built for the solution's depth; a short horizon takes the runtime carving)
                print("RECORD", set_id, m, s, "alone", json.dumps(record), flush=True)
                bad = _matches(record, exp_alone)
                assert not bad, f"{tag} obs_cutils pred_depth {P}: the launch ran {record}; (got, expected) {bad}"
            n_launch += 1
        env.pred_depth = 500
        for P in sorted({P for c in cases for P in c["py_pred"]}, reverse=True):
            for depth in (2, 3):
                compare_tree(env.obs_tree(depth, P), depth, P, "obs_tree")
                assert env.last_obs_launch()["mode"] == 1
                inject()
                got, tree = env.obs_both(depth, P)
                record = env.last_obs_launch()
                if P == 30:
                    if depth == 2:
                        print("RECORD", set_id, m, s, "both", json.dumps(record), flush=True)
                    bad = _matches(record, exp_both)
                    assert not bad, f"{tag} obs_both({depth}, {P}): the launch ran {record}; (got, expected) {bad}"
                compare_tree(tree, depth, P, "obs_both")
                compare_cutils(got, 500, "obs_both")
                n_launch += 2
        env.check()
        util.same(env.state()[0], states, f"{tag} rows after the launches", dtype=True)
        env.close()
        n_env += B
    print("DONE", set_id, n_env, "envs", n_launch, "launches")


def test_no_case_is_left_out():
    assert sorted(c["name"] for s in oc.SETS for c in oc.CASES if (c["map"], c["set"]) == s) == sorted(c["name"] for c in oc.CASES)
    assert sorted(n for s in oc.SETS for n in oc.load_set(*s)["names"]) == sorted(c["name"] for c in oc.CASES)
    assert max(sum((c["map"], c["set"]) == s for c in oc.CASES) for s in oc.SETS) < 100      # tens of envs a batch


_GPU_LOST = []      # the child that ended on a signal or at its time limit: nothing more is started on that card by this file


@pytest.mark.parametrize("set_id", list(SWITCH_SETS))
def test_kernels_equal_the_reference_on_constructed_states(set_id):
    if _GPU_LOST:
        pytest.fail("%s: not started, the child %s ended %s" % (set_id, _GPU_LOST[0][0], _GPU_LOST[0][1]))
    t0 = time.time()
    lines = sw.fresh_child(__file__, [set_id], SWITCH_SETS[set_id][0], CHILD_TIMEOUT, lost=_GPU_LOST)
    print("%s: %.1f s\n%s" % (set_id, time.time() - t0, "\n".join(ln for ln in lines if ln.startswith(("RECORD ", "DONE ")))))
    assert any(ln.startswith("DONE %s " % set_id) for ln in lines)


if __name__ == "__main__":
    _run(sys.argv[1])
