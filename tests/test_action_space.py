"""CPU: the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py (possible_actions_sorted_by_distance :14-56,
find_all_cells_where_agent_can_choose :145-176, on_decision_cell :197-198).  The numpy restatement (tests/action_space_np.py) equals
every array the real reference recorded (tests/golden/action_space_*.npz, tools/capture_action_space.py), bit for bit; the fixtures
hold every property a transcription gets wrong easily; fl_action_space and fl_decision_cells are declared, exported and bound; the
shim has flatland.contrib.wrappers.flatland_wrappers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from flatland_marl_amd import hip_backend as hb
from tests import action_space_np as an
from tests import cabi
from tests import util


def test_every_source_is_there():
    assert an.files() == sorted(an.SOURCES)


@pytest.mark.parametrize("source", an.SOURCES)
def test_restatement_equals_the_reference(source):
    n = 0
    for g in an.groups(source):
        cells = an.decision_cells(g["grid"])
        assert util.same_bits(cells, g["cells"]), g["name"]
        for s in range(len(g["steps"])):
            got = an.action_space(g["grid"], g["dm"], g["slot"], g["init_pos"], g["state"][s], cells)
            for k, mine in zip(an.KINDS, got):
                assert util.same_bits(mine, g[k][s]), (g["name"], int(g["steps"][s]), k)
            n += 1
    assert n > 0


@pytest.mark.parametrize("name", sorted(an.WRAPPED))
def test_the_wrapped_episodes_are_recorded(name):
    w = an.wrapped_episode(name)
    S, A = w["reduced"].shape
    assert 20 <= S <= 80 and w["reduced"].max() == 2 and w["reduced"].min() == 0
    assert (w["inner"] >= 1).all()      # (an agent off the map is always handed back: the inner loop runs once while one waits)
    assert w["present"].any(axis=1).all()
    assert (w["reward"][w["present"] == 0] == 0).all()
    assert np.array_equal(util.load(an.WRAPPED_STATICS[name])["init_pos"].shape, (A, 2))


def test_a_wrapped_episode_skips_agents_and_sums_their_rewards():
    """agents left out of an outer step's dicts while others are handed back, a reward that is no integer (the discounted sum of
    skipped rewards), and the end of the episode"""
    w = an.wrapped_episode("wrapped_lasso")
    assert (w["present"].sum(axis=1) < w["present"].shape[1]).any()
    assert (w["reward"] != np.round(w["reward"])).any()
    assert w["done_all"][-1] == 1 and not w["done_all"][:-1].any()


def _agents():
    """every recorded (agent, state) as a dict of what the properties below look at"""
    for g in an.all_groups():
        grid = g["grid"]
        for s in range(len(g["steps"])):
            for a in range(len(g["slot"])):
                r, c, d, state = (int(v) for v in g["state"][s][a][:4])
                n = int(g["sp_count"][s][a])
                on_map = an.MOVING <= state <= an.MALF
                vpos = tuple(int(v) for v in g["init_pos"][a]) if state == an.READY else (r, c) if on_map else None
                cand = []       # (movement, action, distance) in N, E, S, W order, as the reference's loop makes them
                if vpos is not None:
                    moves = [m for m in range(4) if an.transitions(grid, vpos[0], vpos[1], d)[m]]
                    for m in moves:
                        act = an.FORWARD if m == d else an.RIGHT if m == (d + 1) % 4 else an.LEFT if m == (d - 1) % 4 else an.FORWARD
                        nr, nc = vpos[0] + an.DR[m], vpos[1] + an.DC[m]
                        v = g["dm"][int(g["slot"][a]), nr, nc, m] if 0 <= nr < grid.shape[0] and 0 <= nc < grid.shape[1] else 0xFFFF
                        cand.append((m, act, np.inf if v == 0xFFFF else float(v)))
                yield dict(group=g["source"] + "/" + g["name"], state=state, dir=d, pos=(r, c) if r >= 0 else None, on_map=on_map,
                           init=tuple(int(v) for v in g["init_pos"][a]), n=n, act=[int(v) for v in g["sp_action"][s][a][:n]],
                           dist=[float(v) for v in g["sp_dist"][s][a][:n]], cand=cand, dec=int(g["on_decision"][s][a]),
                           kind=int(g["cells"][r, c]) if r >= 0 else None)


def _pairs(x):
    return [(p, q) for i, p in enumerate(x["cand"]) for q in x["cand"][i + 1:]]


def _adjacent(x, p, q):
    """the list holds candidate p directly in front of candidate q"""
    return any((x["act"][k], x["dist"][k], x["act"][k + 1], x["dist"][k + 1]) == (p[1], p[2], q[1], q[2]) for k in range(x["n"] - 1))


PROPERTIES = {
    "a list of three": lambda x: x["n"] == 3 and len(x["cand"]) == 3,
    "a doubled single candidate": lambda x: len(x["cand"]) == 1 and x["n"] == 2 and x["act"][0] == x["act"][1] and x["dist"][0] == x["dist"][1],
    "the dead-end turn: movement dir + 2 as MOVE_FORWARD": lambda x: any(m == (x["dir"] + 2) % 4 and a == an.FORWARD for m, a, _ in x["cand"]),
    "a finite tie whose order is N, E, S, W and not the order of the actions":
        lambda x: any(p[2] == q[2] and np.isfinite(p[2]) and p[1] > q[1] and _adjacent(x, p, q) for p, q in _pairs(x)),
    "a list whose first action number exceeds its second": lambda x: x["cand"] and x["n"] >= 2 and x["act"][0] > x["act"][1],
    "an infinite distance": lambda x: x["cand"] and any(np.isinf(v) for v in x["dist"]),
    "an infinite tie": lambda x: len(x["cand"]) >= 2 and sum(np.isinf(v) for v in x["dist"]) >= 2,
    "WAITING": lambda x: x["state"] == an.WAITING and x["act"] == [0, 0] and x["dist"] == [0.0, 0.0] and x["dec"] == 1,
    "READY_TO_DEPART read from initial_position": lambda x: x["state"] == an.READY and x["pos"] is None and x["act"][0] != 0 and x["dec"] == 1,
    "MALFUNCTION_OFF_MAP": lambda x: x["state"] == an.MALF_OFF and x["act"] == [0, 0] and x["dec"] == 1,
    "MOVING": lambda x: x["state"] == an.MOVING and x["act"][0] != 0,
    "STOPPED": lambda x: x["state"] == an.STOPPED and x["act"][0] != 0,
    "MALFUNCTION": lambda x: x["state"] == an.MALF and x["act"][0] != 0,
    "DONE": lambda x: x["state"] == an.DONE and x["pos"] is None and x["act"] == [0, 0] and x["dist"] == [0.0, 0.0] and x["dec"] == 1,
    "an on-map agent on a switch": lambda x: x["on_map"] and x["kind"] & 1 and x["dec"] == 1,
    "an on-map agent next to a switch only": lambda x: x["on_map"] and x["kind"] == 2 and x["pos"] != x["init"] and x["dec"] == 1,
    "an on-map agent on its own start cell only": lambda x: x["on_map"] and x["kind"] == 0 and x["pos"] == x["init"] and x["dec"] == 1,
    "an on-map agent on no decision cell": lambda x: x["on_map"] and x["kind"] == 0 and x["pos"] != x["init"] and x["dec"] == 0,
}
MAP_PROPERTIES = {
    "a map without any switch": lambda g: (g["grid"] != 0).any() and not (g["cells"] != 0).any(),
    "a map where every cell is a switch": lambda g: (g["grid"] != 0).all() and (g["cells"] & 1).all(),
    "a map taller than wide": lambda g: g["grid"].shape[0] > g["grid"].shape[1],
}


@pytest.fixture(scope="module")
def recorded():
    return list(_agents())


@pytest.mark.parametrize("prop", sorted(PROPERTIES))
def test_the_fixtures_hold_the_property(recorded, prop):
    where = sorted({x["group"] for x in recorded if PROPERTIES[prop](x)})
    print("%s: %d group(s), first %s" % (prop, len(where), where[:1]))
    assert where, "no recorded agent shows: " + prop


@pytest.mark.parametrize("prop", sorted(MAP_PROPERTIES))
def test_the_fixtures_hold_the_map(prop):
    where = [g["source"] + "/" + g["name"] for g in an.all_groups() if MAP_PROPERTIES[prop](g)]
    print("%s: %s" % (prop, where[:3]))
    assert where, "no recorded map is: " + prop


def test_the_entry_points_are_declared_exported_and_bound():
    """include/flatland_wrappers.h (a header of its own, like flatland_predict.h) against its ctypes table: what is this header's own;
    the types, the counts and the exports are tests/test_cabi_headers.py's"""
    decls = cabi.declarations("flatland_wrappers.h")
    assert [name for _, name, _ in decls] == list(hb.symbols("flatland_wrappers.h")) == ["fl_action_space", "fl_decision_cells"]
    assert '#include "flatland_hip.h"' in cabi.text("flatland_wrappers.h")
    params = {name: ps for _, name, ps in decls}
    assert params["fl_action_space"] == ["fl_batch *h", "int b0", "int nb", "int elem_kind", "uint8_t *sp_action_dev", "void *sp_dist_dev",
                                         "uint8_t *sp_count_dev", "uint8_t *on_decision_dev", "const uint8_t *reduced_dev",
                                         "uint8_t *actions_dev"]
    assert params["fl_decision_cells"] == ["fl_batch *h", "int b0", "int nb", "uint8_t *cells_dev"]
    for cls, names in ((hb.BatchedRailEnv, ("shortest_path_actions", "on_decision_cell", "decision_cells", "reduced_actions",
                                            "step_shortest_path")),
                       (hb.MixedBatch, ("shortest_path_actions", "on_decision_cell", "decision_cells", "reduced_actions",
                                        "step_shortest_path"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_the_shim_has_the_contrib_wrappers():
    """reference-style code imports flatland.contrib.wrappers.flatland_wrappers: the five names come through the shim (a fresh
    interpreter with the shim in front of its path: no other `flatland` can answer)"""
    import flatland_marl_amd
    shim = os.path.join(os.path.dirname(os.path.abspath(flatland_marl_amd.__file__)), "shim")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from flatland.contrib.wrappers.flatland_wrappers import (possible_actions_sorted_by_distance, find_all_cells_where_agent_can_choose,\n"
            "    RailEnvWrapper, ShortestPathActionWrapper, SkipNoChoiceCellsWrapper)\n"
            "import flatland.contrib.wrappers.flatland_wrappers as m, flatland_marl_amd.rail_env as r\n"
            "assert m.__file__.startswith(%r), m.__file__\n"
            "assert SkipNoChoiceCellsWrapper is r.SkipNoChoiceCellsWrapper and ShortestPathActionWrapper is r.ShortestPathActionWrapper\n"
            "assert issubclass(SkipNoChoiceCellsWrapper, RailEnvWrapper) and issubclass(ShortestPathActionWrapper, RailEnvWrapper)\n"
            "assert not hasattr(m, 'DeadlockWrapper')\n"
            "print('ok')\n" % (shim, util.ROOT, shim))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=util.ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
