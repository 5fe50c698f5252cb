"""GPU: every row of tests/obs_kernel_cases.py -- each runtime-carving kernel k_obs<MODE, VAR>, the split kernels fl_obs_s2 / fl_obs_s4 and the
fallback value of every launcher option -- against the CPU oracle, bit for bit, at the smallest shape of the repository that reaches it.

One case per row, one fresh child process per case (the launcher reads its switches once per process): the child builds a small batch over the
row's maps, steps it with the device-side action streams and shadows EVERY env by oracle.orc.OracleEnv; on every step the state, the row's
observation (the seven flatland_cutils tensors and / or the upstream tree) and what the launch ran (BatchedRailEnv.last_obs_launch()) must be
the oracle's resp. the row's.  A child that fails is not run again; its stderr is the case's failure."""
import json
import sys
import time

import numpy as np
import pytest

from tests import obs_kernel_cases as cases
from tests import obs_switch_runs as sw
from tests import util

CUTILS = sw.CUTILS
SEED = 9
# a guard, not a measurement: five times the slowest child of the first full run on an MI355X (split-cfg5x2-d3: two 400-agent envs)
CHILD_TIMEOUT = 60


def _matches(record, expect):
    bad = {}
    for k, v in expect.items():
        if (record[k] < 4096) if v == "head" else (record[k] != v):     # ("head": an LDS head of the HBM work lists, at least OBS_WL_HEAD_MIN bytes)
            bad[k] = (record[k], v)
    return bad


def _run(row):
    from flatland_marl_amd import synth, workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    from oracle import orc
    B, steps, _ = cases.RECIPES[row.recipe]
    maps = cases.maps_of(row.recipe)
    envs = []
    for b in range(B):
        e = dict(maps[b % len(maps)])
        e["mt_key"], e["mt_pos"] = wl.replica_rng(b)
        e["malf_rate"] = 1.0 / 200.0
        envs.append(e)
    env = BatchedRailEnv(envs, max_nodes=row.max_nodes, pred_depth=row.pred_depth)
    A = env.A
    oracles = [orc.OracleEnv(e) for e in envs]
    dms = [o.distance_map() for o in oracles]
    handles = None if row.handles is None else cases.handle_lists()[row.handles]
    kind_of_call, depth = row.call[0], (row.call[1] if len(row.call) > 1 else 0)
    multi_c, multi_t = np.zeros(B, bool), np.zeros(B, bool)
    record = None
    for t in range(steps):
        kind = 2 if t % 10 else 0
        env.step_synth(SEED, 0, kind, auto_reset=False)
        ob = tr = None
        if kind_of_call == "cutils":
            ob = env.obs_cutils(handles=handles)
        elif kind_of_call == "both":
            ob, tr = env.obs_both(depth, 30)
        else:
            tr = env.obs_tree(depth, 30, handles=handles)
        record = env.last_obs_launch()
        if t == 0:
            print("RECORD", row.id, json.dumps(record), flush=True)
        bad = _matches(record, row.expect)
        assert not bad, f"{row.id} step {t}: the launch ran {record}; (got, expected) {bad}"
        st, _ = env.state()
        ob = {k: v.cpu().numpy() for k, v in ob.items()} if ob is not None else None
        tr = tr.cpu().numpy() if tr is not None else None
        for b, o in enumerate(oracles):
            if kind == 2:
                s = o.state()
                acts = synth.spfollow_actions(SEED, b, t, s[:, 3], s[:, 0:2], s[:, 2], np.asarray(envs[b]["grid"]), *dms[b])
            else:
                acts = synth.uniform_actions(SEED, b, t, A)
            o.step(acts)
            np.testing.assert_array_equal(st[b], o.state(), err_msg=f"{row.id} env {b} step {t} state")
            if ob is not None:
                exp = o.obs_cutils(row.max_nodes, row.pred_depth, handles=handles)
                for key, okey in CUTILS:
                    np.testing.assert_array_equal(ob[key][b], exp[okey], err_msg=f"{row.id} env {b} step {t} {key}")
                multi_c[b] |= bool((exp["adjacency"][:, :, 0] >= 0).any())
            if tr is not None:
                exp_t = o.obs_pytree(depth, 30, handles=handles)
                np.testing.assert_array_equal(tr[b], exp_t, err_msg=f"{row.id} env {b} step {t} depth-{depth} tree")
                multi_t[b] |= bool((~(np.isinf(exp_t[:, 1:, 0]) & (exp_t[:, 1:, 0] < 0))).any())
    env.check()
    assert (env.state()[0][:, :, 0] >= 0).sum() > B, "trains are on the maps"
    assert (multi_c.all() or kind_of_call == "tree") and (multi_t.all() or kind_of_call == "cutils"), "every env's compared trees had more than one node at some step"
    if row.expect["split"]:      # both bodies of the split kernel were under the oracle: envs on either side of the class's rail cells
        rails = np.array([int((np.asarray(e["grid"]) != 0).sum()) for e in envs])
        assert {bool(r <= cases.SPLIT_RCAP[row.expect["fix"]]) for r in rails} == {True, False}, rails
    print("DONE", row.id)


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", [r.id for r in cases.ROWS])
def test_row_matches_the_oracle_and_runs_the_kernel_it_names(row_id):
    row = cases.BY_ID[row_id]
    t0 = time.time()
    lines = sw.fresh_child(__file__, [row_id], row.switches, CHILD_TIMEOUT)
    print("%s: %.1f s  %s" % (row_id, time.time() - t0, "".join(ln for ln in lines if ln.startswith("RECORD "))))
    assert ("DONE %s" % row_id) in lines


@pytest.mark.gpu
def test_each_handle_reports_its_own_last_launch():
    """two handles of different shapes (cfg1 and cfg2 size) in one process: a launch of one leaves the other's record alone"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    e1 = BatchedRailEnv([util.static_of(util.load("cfg1_uniform"))])
    e2 = BatchedRailEnv([util.static_of(util.load("cfg2_uniform"))] * 2)
    assert (e1.B, e1.A) != (e2.B, e2.A)
    assert e1.last_obs_launch()["mode"] == -1 and e2.last_obs_launch()["mode"] == -1
    e1.step_synth(SEED, 0, 0, auto_reset=False)
    e2.step_synth(SEED, 0, 0, auto_reset=False)
    e1.obs_tree(2, 30)
    r1 = e1.last_obs_launch()
    assert r1["mode"] == 1 and e2.last_obs_launch()["mode"] == -1
    e2.obs_cutils()
    r2 = e2.last_obs_launch()
    assert r2["mode"] not in (-1, 1) and r2 != r1
    assert e1.last_obs_launch() == r1                    # ... after the other handle has launched
    e1.obs_both(2, 30)
    r1b = e1.last_obs_launch()
    assert r1b["mode"] not in (-1, 1) and r1b != r1 and e2.last_obs_launch() == r2
    e2.obs_tree(3, 30)
    assert e2.last_obs_launch()["mode"] == 1 and e1.last_obs_launch() == r1b
    e1.check(); e2.check()


if __name__ == "__main__":
    _run(cases.BY_ID[sys.argv[1]])
