"""CPU: ShortestPathPredictorForRailEnv.get() / get_shortest_paths (predictions.py:97-180, rail_env_shortest_paths.py:203-274).
The numpy restatement (tests/predictions_np.py) equals every array the real reference recorded (tests/golden/predictions_*.npz,
tools/capture_predictions.py), bit for bit; the fixtures hold every property a transcription gets wrong easily; fl_predict is declared,
exported and bound."""
import numpy as np
import pytest

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import predictions_cases as pc
from tests import predictions_np as pn


def test_every_source_is_there():
    assert pc.files() == sorted(pc.SOURCES)


@pytest.mark.parametrize("source", pc.SOURCES)
def test_restatement_equals_the_reference(source):
    n = 0
    for g in pc.groups(source):
        for D in g["depths"]:
            for s in range(len(g["steps"])):
                pred, wp, ln, visited = pn.predict(g["grid"], g["dm"], g["slot"], g["init_pos"], g["target"], g["speed"], g["state"][s], D)
                where = (g["name"], D, int(g["steps"][s]))
                for mine, ref in ((pred, g[("pred", D)][s]), (wp, g[("wp", D)][s]), (ln, g[("len", D)][s])):
                    assert mine.dtype == ref.dtype and mine.shape == ref.shape and mine.tobytes() == ref.tobytes(), where
                for a, v in enumerate(visited):
                    k = int(g[("devlen", D)][s][a])
                    assert [tuple(int(q) for q in x) for x in g[("dev", D)][s][a][:k]] == v, where + (a,)
                    assert (g[("dev", D)][s][a][k:] == -1).all()
                n += 1
    assert n > 0


def _agents():
    """every recorded (agent, state, depth) as a dict of what the properties below look at"""
    for g in pc.all_groups():
        for D in g["depths"]:
            for s in range(len(g["steps"])):
                for a in range(len(g["slot"])):
                    pred, n = g[("pred", D)][s][a], int(g[("len", D)][s][a])
                    yield dict(D=D, pred=pred, n=n, wp=g[("wp", D)][s][a], state=int(g["state"][s][a][3]), dir=int(g["state"][s][a][2]),
                               target=tuple(int(v) for v in g["target"][a]), speed=float(g["speed"][a]),
                               tpc=int(np.reciprocal(np.float64(g["speed"][a]))), stops=pred[:, 4] == 4,
                               dev=[tuple(int(q) for q in x) for x in g[("dev", D)][s][a][:int(g[("devlen", D)][s][a])]])


def _pos(row):
    return (int(row[1]), int(row[2]))


PROPERTIES = {
    "a path cut at max_depth whose last row is a stop away from the target":
        lambda x: x["n"] == x["D"] and x["D"] > 1 and x["tpc"] == 1 and x["pred"][x["D"], 4] == 4 and _pos(x["pred"][x["D"]]) != x["target"]
        and _pos(x["pred"][x["D"]]) == tuple(int(v) for v in x["wp"][x["D"] - 1][:2]) and not x["stops"][:x["D"]].any(),
    "a path that ends on the target early":
        lambda x: 1 < x["n"] < x["D"] and tuple(int(v) for v in x["wp"][x["n"] - 1][:2]) == x["target"],
    "a None path": lambda x: x["n"] == 0 and x["stops"][1:].all() and not x["stops"][0],
    "DONE": lambda x: x["state"] == 6 and x["n"] == 1 and _pos(x["pred"][0]) == x["target"] and x["stops"][1:].all(),
    "WAITING": lambda x: x["state"] == 0,
    "READY_TO_DEPART": lambda x: x["state"] == 1,
    "MALFUNCTION_OFF_MAP": lambda x: x["state"] == 2,
    "STOPPED on the map": lambda x: x["state"] == 4,
    "MALFUNCTION on the map": lambda x: x["state"] == 5,
    "times_per_cell > max_depth with no stop row": lambda x: x["tpc"] > x["D"] and x["n"] > 1 and not x["stops"].any(),
    "a speed at which float32 would give another times_per_cell":
        lambda x: int(np.reciprocal(np.float32(x["speed"]))) != x["tpc"],
    "a start next to the target": lambda x: x["n"] == 2 and tuple(int(v) for v in x["wp"][1][:2]) == x["target"],
    "a dev_pred_dict entry whose stop-row direction differs from the walked one":
        lambda x: any(st and int(r[3]) != x["dir"] and (int(r[1]), int(r[2]), x["dir"]) in x["dev"] for r, st in zip(x["pred"], x["stops"])),
}


@pytest.fixture(scope="module")
def recorded():
    return list(_agents())


@pytest.mark.parametrize("prop", sorted(PROPERTIES))
def test_the_fixtures_hold_the_property(recorded, prop):
    assert any(PROPERTIES[prop](x) for x in recorded), "no recorded agent shows: " + prop


def test_get_handle_keys():
    """`if handle:` (predictions.py:122-123): get(3) is agent 3 alone, get(0) and get(None) every agent"""
    extras = [g["extra"] for g in pc.all_groups() if g["extra"]]
    assert extras
    for e in extras:
        assert e["get3"].tolist() == [3] and e["get0"].tolist() == e["getnone"].tolist() and len(e["get0"]) > 3


def test_fl_predict_is_declared_exported_and_bound():
    """include/flatland_predict.h (a header of its own, like flatland_policy.h and flatland_train.h) against its ctypes table: what is
    this header's own; the types, the counts and the exports are tests/test_cabi_headers.py's"""
    decls = cabi.declarations("flatland_predict.h")
    assert [name for _, name, _ in decls] == list(hb.symbols("flatland_predict.h")) == ["fl_predict"]
    assert decls[0][2] == [
        "fl_batch *h", "int b0", "int nb", "int max_depth", "int elem_kind", "void *pred_dev", "int32_t *path_dev", "int32_t *path_len_dev"]
    assert '#include "flatland_hip.h"' in cabi.text("flatland_predict.h")
    assert callable(getattr(hb.BatchedRailEnv, "predictions")) and callable(getattr(hb.MixedBatch, "predictions"))
