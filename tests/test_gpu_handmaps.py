"""GPU: the table kernels of flatland_marl_amd/csrc/fl_dmap.hip (distance map, segment table, next-hop, hop8, env list) and the observation kernels that read
those tables, on the hand-made rail maps of tests/handmaps.py -- BFS levels of several 64-state chunks, cycles of single-way states, targets
that cannot be reached, more than 1 024 envs in the env list and the looping grid of a large masked rebuild.  The fixtures hold what the real
reference does on these maps (oracle/refharness/capture_handmaps.py); tests/test_handmaps.py pins the CPU oracle to them and asserts which
path each one reaches.  Every comparison is integer or exact-float equality.

flatland_cutils raised on none of these maps, the mesh included (cutils_raised is 0 at every recorded step): check() must never raise here.

One part of the fixtures is no function of the env: the road type of an agent on a cell of no Flatland type (mesh12 only;
handmaps.known_cell_type).  There the kernels are held to the oracle's value."""
import sys
import time

import numpy as np
import pytest

from tests import handmaps, util
from tests import obs_switch_runs as sw

CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"),
          ("edge_order", "edge_order"), ("valid_actions", "valid"))
PROPS = ("p_dist_target", "p_deadlocked", "p_ready")
CANVAS = (12, 12)
SEED = 23
CHILD_TIMEOUT = 60      # a guard, not a measurement


def _fixture(name):
    return util.load("handmap_" + name)


def _cutils_equals_golden(got, fx, t, b, tag):
    """the seven flatland_cutils tensors of env b against step t of a fixture"""
    ok = handmaps.defined_attr(fx, t)
    attr = got["agent_attr"][b]
    util.same(attr[ok], fx["o_attr"][t][ok], f"{tag} agent_attr")
    no_type = ~ok[:, handmaps.ROAD_TYPE_COLS].all(axis=1)
    assert (attr[no_type][:, handmaps.ROAD_TYPE_COLS] == [1] + [0] * 10).all(), f"{tag}: road type 0 on a cell of no Flatland type, as the oracle says"
    for g, e in CUTILS[1:]:
        util.same(got[g][b], fx["o_" + e][t], f"{tag} {g}")
    for col, k in enumerate(PROPS):
        util.same(got["props"][b][:, col], fx["o_" + k][t], f"{tag} {k}")


def _cutils_equals_oracle(got, exp, b, tag):
    for g, e in CUTILS + (("props", "props"),):
        util.same(got[g][b], exp[e], f"{tag} {g}")


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _replay(fx, fused, steps=None, tag=""):
    """one env on a fixture's map follows the fixture's episode: distance map, state, reward, done, both upstream trees and the flatland_cutils
    tensors at every step; flatland_cutils raised nowhere, so check() raises nowhere"""
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    assert not fx["cutils_raised"].any()
    env = BatchedRailEnv([util.static_of(fx)])
    dm, slot = env.distance_map(0)
    util.same(dm, fx["dm_u16"], f"{tag} distance map")
    util.same(slot, fx["target_slot"], f"{tag} target slots")
    n = len(fx["state"]) if steps is None else min(steps + 1, len(fx["state"]))
    for t in range(n):
        if t > 0:
            rew, done, _ = env.step(torch.from_numpy(fx["actions"][t - 1][None, :].copy()).cuda())
            util.same(rew.cpu().numpy()[0], fx["reward"][t - 1], f"{tag} t={t} reward")
            util.same(done.cpu().numpy()[0], fx["done"][t - 1], f"{tag} t={t} done")
        util.same(env.state()[0][0], fx["state"][t], f"{tag} t={t} state")
        env.check()
        got = None
        for d in (2, 3):
            if fused:
                got, tree = env.obs_both(d, 30)
            else:
                tree = env.obs_tree(d, 30)
            util.same(tree.cpu().numpy()[0], fx["py_d%d_p30" % d][t], f"{tag} t={t} depth-{d} tree")
            if not fused:
                env.check()
        if not fused:
            got = env.obs_cutils()
        env.check()
        _cutils_equals_golden(_host(got), fx, t, 0, f"{tag} t={t}")
    record = env.last_obs_launch()
    env.close()
    return record


@pytest.mark.gpu
@pytest.mark.parametrize("name", handmaps.EPISODES)
@pytest.mark.parametrize("fused", [False, True])
def test_kernels_on_hand_made_maps(name, fused):
    _replay(_fixture(name), fused, tag=name)


@pytest.mark.gpu
def test_distance_map_with_levels_of_five_chunks_and_more_states_than_the_ring():
    """mesh33: 4 356 states a target (the BFS ring holds 4 096), levels of up to 260 states -- five 64-state chunks of one level, the ring wraps"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    fx = _fixture("mesh33")
    env = BatchedRailEnv([util.static_of(fx)])
    dm, slot = env.distance_map(0)
    util.same(dm, fx["dm_u16"], "mesh33 distance map")
    util.same(slot, fx["target_slot"], "mesh33 target slots")
    env.check()                                     # (no FL_ERR_CAPACITY: the ring never holds more than two levels)
    env.close()


def _small_envs():
    """the four five-agent maps on one canvas: different rail cells and unique targets per env under one Rcap / Ucap"""
    return [handmaps.padded(util.static_of(_fixture(n)), *CANVAS) for n in handmaps.SMALL]


@pytest.mark.gpu
def test_mixed_batch_of_hand_made_maps_matches_the_oracles():
    from flatland_marl_amd import synth
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    from oracle import orc
    envs = _small_envs()
    assert len({int((e["grid"] != 0).sum()) for e in envs}) > 2 and {len({tuple(t) for t in e["target"].tolist()}) for e in envs} == {4, 5}
    env = BatchedRailEnv(envs)
    oracles = [orc.OracleEnv(e) for e in envs]
    for b, o in enumerate(oracles):
        util.same(env.distance_map(b)[0], o.distance_map()[0], f"env {b} distance map")
    for t in range(40):
        env.step_synth(SEED, 0, 1, auto_reset=False)
        if t % 2:
            got, tree = env.obs_both(3, 30)
            depth = 3
        else:
            got, tree, depth = env.obs_cutils(), env.obs_tree(2, 30), 2
        got, tree, st = _host(got), tree.cpu().numpy(), env.state()[0]
        for b, o in enumerate(oracles):
            o.step(synth.forward_biased_actions(SEED, b, t, env.A))
            tag = f"{handmaps.SMALL[b]} step {t}"
            util.same(st[b], o.state(), f"{tag} state")
            _cutils_equals_oracle(got, o.obs_cutils(31, 500), b, tag)
            util.same(tree[b], o.obs_pytree(depth, 30), f"{tag} depth-{depth} tree")
    env.check()
    assert (env.state()[0][:, :, 0] >= 0).any(axis=1).all(), "trains are on every map"
    env.close()


def _many_envs(B):
    """B envs over the four small maps in turn, no two with the same (grid, unique targets): none shares its static tables with another.  The
    targets of the first three agents walk over the map's rail cells with the env's index."""
    bases = _small_envs()
    cells = [np.argwhere(e["grid"] != 0) for e in bases]
    out, seen, j = [], set(), [0] * len(bases)
    for b in range(B):
        m = b % len(bases)
        while True:
            tg = np.array(bases[m]["target"], dtype=np.int32)
            k = j[m]
            for i in range(3):
                first = int(np.flatnonzero((cells[m] == tg[i]).all(axis=1))[0])
                tg[i] = cells[m][(first + k % len(cells[m])) % len(cells[m])]
                k //= len(cells[m])
            j[m] += 1
            unique = []
            for t in map(tuple, tg.tolist()):
                if t not in unique:
                    unique.append(t)
            if (m, tuple(unique)) not in seen:
                seen.add((m, tuple(unique)))
                break
        out.append(dict(bases[m], target=tg))
    return out


@pytest.mark.gpu
def test_more_envs_than_a_round_of_the_env_list_and_the_looping_rebuild_grid():
    """2 100 envs with tables of their own: three rounds of k_env_list at construction (the offset carried from round to round); a masked
    rebuild across the rounds' borders; and a rebuild of every env through the mask path, whose table kernels get the fixed grid of 2 048 looping
    workgroups (k_distance_map then reuses its LDS for a second piece of work)"""
    import torch
    from flatland_marl_amd import synth
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    from oracle import orc
    B = 2100
    envs = _many_envs(B)
    env = BatchedRailEnv(envs)
    A = env.A
    oracles = [orc.OracleEnv(e) for e in envs]
    dms = [o.distance_map()[0] for o in oracles]
    assert max(len(d) for d in dms) == 5 and min(len(d) for d in dms) < 4           # different U under one Ucap
    assert B * ((5 + 3) // 4) > 2048                                               # a full build is more work than the looping grid has workgroups

    def tables(tag):
        for b in range(B):
            util.same(env.distance_map(b)[0], dms[b], f"{tag}: env {b} distance map")

    def observations(tag):
        got, tree = env.obs_both(2, 30)
        got, tree, st = _host(got), tree.cpu().numpy(), env.state()[0]
        for b, o in enumerate(oracles):
            util.same(st[b], o.state(), f"{tag}: env {b} state")
            _cutils_equals_oracle(got, o.obs_cutils(31, 500), b, f"{tag}: env {b}")
            util.same(tree[b], o.obs_pytree(2, 30), f"{tag}: env {b} depth-2 tree")

    def run(t0, n):
        for t in range(t0, t0 + n):
            env.step_synth(SEED, 0, 1, auto_reset=False)
            for b, o in enumerate(oracles):
                o.step(synth.forward_biased_actions(SEED, b, t, A))

    tables("after construction")
    run(0, 8)
    observations("after construction")
    mask = torch.zeros(B, dtype=torch.uint8)
    mask[[0, 1, 511, 1022, 1023, 1024, 1025, 1500, 2046, 2047, 2048, 2049, B - 2, B - 1]] = 1
    env.rebuild_distance_maps(mask.cuda())
    run(8, 3)
    tables("after the masked rebuild")
    observations("after the masked rebuild")
    env.rebuild_distance_maps(torch.ones(B, dtype=torch.uint8).cuda())
    run(11, 3)
    tables("after the rebuild of every env through a mask")
    observations("after the rebuild of every env through a mask")
    env.check()
    assert (env.state()[0][:, :, 0] >= 0).any(axis=1).mean() > 0.5, "trains are on the maps"
    env.close()


# ---- the launcher's fallbacks: the kernels that read the successor and next-hop tables from HBM, and the ones without time masks
# (lds64k-cfg2-d2 also expects nh = 0, but gets there through an LDS limit of 64 KB: next-hop tables of some twenty rail cells fit any limit, so
# on these maps that row's switches leave nh = 1 and there is nothing of the row to run)
FALLBACK_ROWS = ("snext0-cfg2-alone", "snext0-cfg2-d2", "nonh-cfg2-d2", "notmask-cfg2-alone", "notmask-cfg3-d2")
FALLBACK_FIELDS = ("snext", "nh", "tmask")
FALLBACK_MAPS = ("oval", "lasso", "disconnected")


def _run_fallback(row_id):
    from tests import obs_kernel_cases as cases
    row = cases.BY_ID[row_id]
    want = {k: row.expect[k] for k in FALLBACK_FIELDS if k in row.expect}
    assert want and set(want.values()) == {0}
    for name in FALLBACK_MAPS:
        record = _replay(_fixture(name), row.call[0] == "both", steps=36, tag=f"{row_id} {name}")
        print("RECORD", row_id, name, {k: record[k] for k in ("mode", "var", "fix", "split") + FALLBACK_FIELDS}, flush=True)
        assert {k: record[k] for k in want} == want and not record["split"], (row_id, name, record)
    print("DONE", row_id)


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", FALLBACK_ROWS)
def test_launcher_fallbacks_on_cycles_and_unreachable_targets(row_id):
    """the oval, the lasso and the disconnected rail under the switches of the rows of tests/obs_kernel_cases.py that turn the LDS successor
    table, the LDS next-hop tables and the time masks off -- a cycle and an unreachable target look different in exactly those tables.  One fresh
    child per row (the launcher reads its switches once per process); FL_OBS_NO_SPLIT on top of the row's switches: these maps are smaller than
    every launch class, and a split launch would run the class's body on them instead of the fallback."""
    from tests import obs_kernel_cases as cases
    row = cases.BY_ID[row_id]
    t0 = time.time()
    lines = sw.fresh_child(__file__, [row_id], dict(row.switches, FL_OBS_NO_SPLIT="1"), CHILD_TIMEOUT)
    print("%s: %.1f s\n%s" % (row_id, time.time() - t0, "\n".join(ln for ln in lines if ln.startswith("RECORD "))))
    assert ("DONE %s" % row_id) in lines


if __name__ == "__main__":
    _run_fallback(sys.argv[1])
