"""The hand-made rail maps of tests/handmaps.py (fixtures captured from the real reference by oracle/refharness/capture_handmaps.py): the CPU
oracle equals the reference on every one of them, bit for bit; the builders reproduce the fixtures' grids and agents; and every fixture still
reaches the path of flatland_marl_amd/csrc/fl_dmap.hip and of the tree walks it exists for -- measured from the fixture with plain numpy, so that a later edit
cannot quietly turn a map into an easy one.  flatland_cutils raised on none of the maps, the mesh included.  The kernels' side:
tests/test_gpu_handmaps.py."""
import numpy as np
import pytest

from tests import handmaps, util

CUTILS = ("attr", "forest", "adjacency", "node_order", "edge_order", "valid")
DM_QCAP = 4096      # flatland_marl_amd/csrc/fl_dmap.hip: the BFS ring of one target
INF16 = 0xFFFF


def fixture(name):
    return util.load("handmap_" + name)


@pytest.mark.parametrize("name", handmaps.MAPS)
def test_fixtures_load_without_pickle_and_the_builders_reproduce_them(name):
    fx = np.load(util.GOLD + "/handmap_%s.npz" % name, allow_pickle=False)
    m = handmaps.MAPS[name]()
    assert fx["grid"].dtype == np.uint16
    for k in ("grid", "init_pos", "init_dir", "target", "earliest"):
        np.testing.assert_array_equal(fx[k], m[k], err_msg=k)
    for k in fx.files:
        assert fx[k].dtype != object, k


@pytest.mark.parametrize("name", handmaps.MAPS)
def test_oracle_distance_maps_on_hand_made_maps(name):
    from oracle import orc
    fx = fixture(name)
    dm, slot = orc.OracleEnv(fx).distance_map()
    np.testing.assert_array_equal(dm, fx["dm_u16"])
    np.testing.assert_array_equal(slot, fx["target_slot"])


@pytest.mark.parametrize("name", handmaps.EPISODES)
def test_oracle_on_hand_made_maps(name):
    from oracle import orc
    fx = fixture(name)
    e = orc.OracleEnv(fx)
    assert len(fx["actions"]) >= 30 and not fx["cutils_raised"].any()
    for t in range(len(fx["state"])):
        if t > 0:
            rew, done, _ = e.step(fx["actions"][t - 1])
            np.testing.assert_array_equal(rew, fx["reward"][t - 1], err_msg=f"t={t} reward")
            np.testing.assert_array_equal(done, fx["done"][t - 1], err_msg=f"t={t} done")
        np.testing.assert_array_equal(e.state(), fx["state"][t], err_msg=f"t={t}")
        for d in (2, 3):
            np.testing.assert_array_equal(e.obs_pytree(d, 30), fx["py_d%d_p30" % d][t], err_msg=f"t={t} depth {d}")
        o = e.obs_cutils(31, 500)
        ok = handmaps.defined_attr(fx, t)      # (all of it but the road type of an agent on a cell of no Flatland type: mesh12 only)
        assert ok.all() or name == "mesh12"
        np.testing.assert_array_equal(o["attr"][ok], fx["o_attr"][t][ok], err_msg=f"t={t} attr")
        assert (o["attr"][:, handmaps.ROAD_TYPE_COLS].sum(axis=1) == 1).all()
        for k in CUTILS[1:]:
            np.testing.assert_array_equal(o[k], fx["o_" + k][t], err_msg=f"t={t} {k}")
        for col, k in enumerate(("p_dist_target", "p_deadlocked", "p_ready")):
            np.testing.assert_array_equal(o["props"][:, col], fx["o_" + k][t], err_msg=f"t={t} {k}")


def _start_states(fx):
    return [(int(r), int(c), int(d)) for (r, c), d in zip(fx["init_pos"], fx["init_dir"])]


def _own_distance(fx):
    """the distance map of every agent's own target at its own start state"""
    return np.array([int(fx["dm_u16"][fx["target_slot"][i]][s]) for i, s in enumerate(_start_states(fx))])


def test_each_fixture_reaches_the_path_it_exists_for():
    # ---- wide BFS levels: k_distance_map expands a level in chunks of 64 states
    fx = fixture("mesh12")
    widest = max(int(handmaps.level_sizes(slab).max()) for slab in fx["dm_u16"])
    assert widest > 64, widest                                               # a second chunk
    centre = int(np.flatnonzero((fx["dm_targets"] == (6, 6)).all(axis=1))[0])
    assert int(handmaps.level_sizes(fx["dm_u16"][centre]).max()) == 90
    assert max(bin(handmaps.nibble(g, d)).count("1") for g in fx["grid"].ravel() for d in range(4)) == 3      # DFS-slot node tables
    fx = fixture("mesh33")
    finite = int((fx["dm_u16"][0] != INF16).sum())
    widest = max(int(handmaps.level_sizes(slab).max()) for slab in fx["dm_u16"])
    assert finite > DM_QCAP and widest > 128, (finite, widest)               # more states than the ring holds; three chunks and more
    assert len(fx["dm_targets"]) <= 3 and (fx["dm_targets"] == (16, 16)).all(axis=1).any()
    # ---- cycles of single-way states (SEG_CYCLE): from the ring itself (mu = 0) and, on the lasso, from the spur (mu > 0)
    fx = fixture("oval")
    cycles = [handmaps.chain(fx["grid"], s) for s in _start_states(fx)]
    assert all(c == (0, 18) for c in cycles), cycles
    assert {int(d) for (r, c), d in zip(fx["init_pos"], fx["init_dir"]) if r == 1} == {handmaps.E, handmaps.W}      # both directions of travel
    assert not (np.vectorize(lambda g: bin(int(g)).count("1"))(fx["grid"]) > 2).any()                                  # no switch
    assert (_own_distance(fx) != INF16).all()                                                                          # own targets inside the loop
    fx = fixture("lasso")
    cyc = {s: handmaps.chain(fx["grid"], s) for s in _start_states(fx)}
    assert cyc[(1, 3, handmaps.E)] is None                                   # clockwise: the walk ends at the facing switch
    assert cyc[(1, 5, handmaps.W)] == (0, 18)                                # counter-clockwise: a cycle through the trailing switch
    assert cyc[(6, 4, handmaps.N)] == (3, 18)                                # from the spur: the first repeated state is not the start
    assert cyc[(5, 4, handmaps.S)] is None                                   # towards the dead end
    assert bin(int(fx["grid"][handmaps.LASSO_SWITCH])).count("1") > 2 and bin(int(fx["grid"][handmaps.LASSO_DEAD_END])).count("1") == 1
    # ---- unreachable targets: 0xFFFF at the agent's own start state
    assert (_own_distance(fx) == INF16).tolist() == [False, True, False, False, True]
    fx = fixture("disconnected")
    assert (_own_distance(fx) == INF16).tolist() == [True, True, False, False, False]
    # ---- the diamond crossing; one target and one more than the wavefronts of a distance-map workgroup
    u1, u5 = fixture("crossing_u1"), fixture("crossing_u5")
    assert (u1["grid"] == 0x8421).sum() == 1 and np.array_equal(u1["grid"], u5["grid"])
    assert len(u1["dm_targets"]) == 1 and len(u5["dm_targets"]) == 5
    assert (_own_distance(u1) == INF16).tolist() == [False, True, False, True, False]
    t5 = [tuple(t) for t in u5["target"].tolist()]
    assert (4, 4) in t5 and any(bin(int(u5["grid"][t])).count("1") == 1 for t in t5)      # the crossing itself, a dead-end cell
    # ---- the episodes move: trains are on the map, some arrive, and the trees have children
    for name in handmaps.EPISODES:
        fx = fixture(name)
        assert (fx["state"][:, :, 0] >= 0).any(axis=0).all(), name
        assert np.isfinite(fx["py_d3_p30"][:, :, 1:, 0]).any(), name
        assert (fx["o_adjacency"][:, :, :, 0] >= 0).any(), name
    assert sum(int((fixture(n)["state"][-1][:, 3] == 6).sum()) for n in handmaps.EPISODES) >= 10
