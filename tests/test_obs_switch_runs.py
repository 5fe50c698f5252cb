"""CPU: the helpers the observation GPU tests stand on -- util.same / plain_static and tests/obs_switch_runs.py (rows, policy_form, fresh_child,
run_switch_sets, assert_same_bytes) -- fail where they must.  The children here are a few lines of Python written to tmp_path; nothing needs
a GPU."""
import json
import os
import textwrap

import numpy as np
import pytest

from tests import handmaps, util
from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw

N, E, S, W = 0, 1, 2, 3


# ---- util.same
def test_same_passes_on_equal_arrays():
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    for kw in ({}, dict(dtype=True), dict(bytes=True), dict(dtype=True, bytes=True)):
        util.same(a, a.copy(), "equal", **kw)
    util.same(a.tolist(), a, "a list against an array")


def test_same_raises_on_another_shape():
    with pytest.raises(AssertionError, match=r"shapes: int64\(6,\), expected int64\(2, 3\)"):
        util.same(np.zeros(6, dtype=np.int64), np.zeros((2, 3), dtype=np.int64), "shapes")
    with pytest.raises(AssertionError, match="broadcast"):      # (np.array_equal would not broadcast either; `!=` would)
        util.same(np.zeros((1, 3)), np.zeros((2, 3)), "broadcast")


def test_same_raises_on_another_dtype_only_when_asked():
    a, b = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int64)
    util.same(a, b, "values only")
    with pytest.raises(AssertionError, match=r"dtypes: int32\(5,\), expected int64\(5,\)"):
        util.same(a, b, "dtypes", dtype=True)


@pytest.mark.parametrize("kw", [{}, dict(dtype=True), dict(bytes=True)])
def test_same_names_the_first_mismatch(kw):
    exp = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    got = exp.copy()
    got[1, 2, 0] = 99.5
    with pytest.raises(AssertionError) as e:
        util.same(got, exp, "y3/bend both forest", **kw)
    assert str(e.value) == "y3/bend both forest: 1 mismatches, first at [1, 2, 0]: got 99.5, expected 20.0"


def test_same_tells_the_zeros_apart_only_by_bytes():
    a, b = np.array([0.0, 1.0], dtype=np.float32), np.array([-0.0, 1.0], dtype=np.float32)
    util.same(a, b, "by value", dtype=True)
    with pytest.raises(AssertionError, match="by bytes: equal values, other bytes"):
        util.same(a, b, "by bytes", bytes=True)
    nan = np.array([np.nan], dtype=np.float32)
    util.same(nan, nan.copy(), "the same NaN", bytes=True)
    with pytest.raises(AssertionError):
        util.same(nan, nan.copy(), "a NaN by value")


def test_same_bits_is_a_predicate():
    a = np.array([0.0, 1.0], dtype=np.float32)
    assert util.same_bits(a, a.copy()) and not util.same_bits(a, -a) and not util.same_bits(a, a.astype(np.float64)) and not util.same_bits(a, a[:1])


# ---- the builders
def test_plain_static_of_two_agents_on_the_yard():
    grid = handmaps.STEP_MAPS["yard"]()["grid"]
    st = util.plain_static(grid, [(4, 6, W, 4, 0), (4, 2, E, 4, 7)], [1.0, 0.5])
    assert list(st) == ["grid", "init_pos", "init_dir", "target", "speed", "earliest", "latest", "T", "malf_rate", "malf_min", "malf_max", "mt_key", "mt_pos"]
    assert st["grid"] is grid
    arrays = dict(init_pos=("int32", [[4, 6], [4, 2]]), init_dir=("int32", [W, E]), target=("int32", [[4, 0], [4, 7]]), speed=("float64", [1.0, 0.5]),
                  earliest=("int32", [0, 0]), latest=("int32", [200, 200]), mt_key=("uint32", list(range(624))))
    for k, (dt, v) in arrays.items():
        assert st[k].dtype == dt and st[k].tolist() == v, k
    assert (st["T"], st["malf_rate"], st["malf_min"], st["malf_max"], st["mt_pos"]) == (400, 0.0, 0, 0, 624)
    assert all(type(st[k]) is t for k, t in (("T", int), ("malf_rate", float), ("malf_min", int), ("malf_max", int), ("mt_pos", int)))
    far = util.plain_static(grid, [(4, 6, W, 4, 0), (4, 2, E, 4, 7)], [1.0, 0.5], latest=1000, T=2000, target=[(1, 0), (1, 6)])
    assert far["latest"].tolist() == [1000, 1000] and far["T"] == 2000 and far["target"].tolist() == [[1, 0], [1, 6]] and far["target"].dtype == np.int32
    assert far["init_pos"].tolist() == st["init_pos"].tolist()


def test_rows_of_agents_on_and_off_the_map():
    grid = handmaps.STEP_MAPS["yard"]()["grid"]
    spec = [(4, 6, W, 4, 0), (4, 1, E, 4, 4), (4, 1, E, 4, 7)]
    st, aux = sw.rows(grid, spec, [oc.on(oc.MOVING, 4, 5, W, malf=3), oc.off(oc.DONE, d=W), oc.off(oc.WAITING)])
    assert st.dtype == np.int32 and aux.dtype == np.int32
    assert st.tolist() == [[4, 5, W, oc.MOVING, 3, 0, 0, 0, -1, 4, 5, W], [-1, -1, W, oc.DONE, 0, 0, 0, 0, 1, -1, -1, -1],
                           [-1, -1, E, oc.WAITING, 0, 0, 0, 0, -1, -1, -1, -1]]
    assert aux.tolist() == [[-1, 0, 0, 0], [-1, 0, 0, 1], [-1, 0, 0, 0]]


def test_rows_refuses_a_train_facing_a_way_its_cell_does_not_allow():
    grid = handmaps.STEP_MAPS["yard"]()["grid"]
    assert handmaps.nibble(grid[4, 5], W) != 0 and handmaps.nibble(grid[4, 5], N) == 0      # a cell of the bottom line: east and west only
    sw.rows(grid, [(4, 5, W, 4, 0)], [oc.on(oc.MOVING, 4, 5, W)])
    with pytest.raises(AssertionError):
        sw.rows(grid, [(4, 5, W, 4, 0)], [oc.on(oc.MOVING, 4, 5, N)])


def test_policy_form_of_a_hand_made_adjacency():
    """two agents, four nodes a tree: agent 0 has two edges and a padding row, agent 1 one edge; env 3 of a batch"""
    cu = dict(adjacency=np.array([[[0, 1, 0], [0, 2, 2], [-2, -2, -2]], [[0, 1, 1], [-2, -2, -2], [-2, -2, -2]]], dtype=np.int32),
              node_order=np.array([[1, 0, 0, -2], [1, 0, -2, -2]], dtype=np.int32), edge_order=np.array([[0, 0, -1], [0, -2, -2]], dtype=np.int32))
    adj, no, eo = sw.policy_form(cu, 3, 2, max_nodes=4)
    assert adj.dtype == no.dtype == eo.dtype == np.int64
    assert adj.tolist() == [[[24, 25, 0], [24, 26, 2], [-2, -2, -2]], [[28, 29, 1], [-2, -2, -2], [-2, -2, -2]]]      # (3 * 2 + agent) * 4
    assert no.tolist() == [[1, 0, 0, -2], [1, 0, -2, -2]] and eo.tolist() == [[0, 0, -2], [0, -2, -2]]
    assert cu["adjacency"].dtype == np.int32 and cu["adjacency"][0, 0].tolist() == [0, 1, 0]      # the input is left alone


# ---- fresh_child, run_switch_sets, assert_same_bytes against a stand-in child
CHILD = textwrap.dedent("""
    import json, os, signal, sys, time
    path = sys.argv[1]
    tag = os.path.basename(path)[:-4]
    open(os.path.join(os.path.dirname(path), tag + ".started"), "w").close()
    how = os.environ.get("STANDIN_" + tag.upper(), "")
    if how == "kill":
        os.kill(os.getpid(), signal.SIGKILL)
    import numpy as np
    if how == "exit3":
        print("it went wrong", file=sys.stderr)
        sys.exit(3)
    if how == "sleep":
        time.sleep(30)
    seen = {k: v for k, v in os.environ.items() if k.startswith("FL_OBS_") or k == "PYTHONPATH"}
    print("RECORD", "b0", "both", json.dumps(dict(mode=3, env=seen)), flush=True)
    a = np.arange(6, dtype=np.float32)
    if how == "flip":
        a[4] = -a[4]
    np.savez(path, **{"b0/both/forest": a, "b0/both/tree": np.zeros(3)})
    if how != "nodone":
        print("DONE", 2, "tensors")
""")
SETS = (("default", {}), ("second", {"FL_OBS_NO_FIX": "1"}), ("third", {"FL_OBS_NO_CF_DIRS": "1"}))


@pytest.fixture
def script(tmp_path):
    path = tmp_path / "standin_child.py"
    path.write_text(CHILD)
    return str(path)


def _started(tmp_path):
    return sorted(f[:-8] for f in os.listdir(tmp_path) if f.endswith(".started"))


def test_three_well_behaved_children(script, tmp_path):
    outs, records = sw.run_switch_sets(script, SETS, tmp_path, 30)
    assert list(outs) == list(records) == ["default", "second", "third"] and _started(tmp_path) == ["default", "second", "third"]
    assert all(set(r) == {("b0", "both")} and r[("b0", "both")]["mode"] == 3 for r in records.values())
    sw.assert_same_bytes(outs, 2)
    with pytest.raises(AssertionError):
        sw.assert_same_bytes(outs, 3)      # (a tensor fewer than the caller counted)


def test_a_flipped_byte_is_found_and_named(script, tmp_path, monkeypatch):
    monkeypatch.setenv("STANDIN_SECOND", "flip")
    outs, _ = sw.run_switch_sets(script, SETS, tmp_path, 30)
    with pytest.raises(AssertionError) as e:
        sw.assert_same_bytes(outs, 2)
    assert "second" in str(e.value) and "b0/both/forest" in str(e.value)
    no_default = {k: outs[k] for k in ("second", "third")}      # no "default": the first tag is the one the others are held to
    with pytest.raises(AssertionError) as e:
        sw.assert_same_bytes(no_default, 2)
    assert "third" in str(e.value) and "b0/both/forest" in str(e.value)


def test_a_child_that_exits_3_ends_the_loop(script, tmp_path, monkeypatch):
    monkeypatch.setenv("STANDIN_SECOND", "exit3")
    with pytest.raises(AssertionError) as e:
        sw.run_switch_sets(script, SETS, tmp_path, 30)
    assert "second: exit status 3" in str(e.value) and "it went wrong" in str(e.value)
    assert _started(tmp_path) == ["default", "second"]


def test_a_child_at_its_time_limit_ends_the_loop(script, tmp_path, monkeypatch):
    monkeypatch.setenv("STANDIN_DEFAULT", "sleep")
    with pytest.raises(pytest.fail.Exception) as e:
        sw.run_switch_sets(script, SETS, tmp_path, 1)
    assert "default: no end after 1 s" in str(e.value) and _started(tmp_path) == ["default"]


def test_a_child_that_ends_on_a_signal_is_remembered(script, tmp_path, monkeypatch):
    monkeypatch.setenv("STANDIN_SECOND", "kill")
    lost = []
    sw.fresh_child(script, [str(tmp_path / "default.npz")], {}, 30, lost=lost)
    assert lost == []
    with pytest.raises(AssertionError, match="exit status -9"):
        sw.fresh_child(script, [str(tmp_path / "second.npz")], {}, 30, tag="second", lost=lost)
    assert lost == [("second", "with exit status -9")]


def test_a_child_without_DONE_fails(script, tmp_path, monkeypatch):
    monkeypatch.setenv("STANDIN_SECOND", "nodone")
    with pytest.raises(AssertionError, match="second"):
        sw.run_switch_sets(script, SETS, tmp_path, 30)
    assert _started(tmp_path) == ["default", "second"]


def test_a_misspelt_switch_is_refused_before_any_child_starts(script, tmp_path):
    """the launcher ignores a name its table does not have: the child would run the default, and a "this switch changes no byte" test pass"""
    with pytest.raises(AssertionError, match="no such switch of the launcher: FL_OBS_NOFIX"):
        sw.run_switch_sets(script, (("typo", {"FL_OBS_NOFIX": "1"}),) + SETS, tmp_path, 30)
    assert _started(tmp_path) == []
    with pytest.raises(AssertionError, match="alone: no such switch of the launcher: FL_OBS_NOFIX, FL_OBS_NO_TAB"):
        sw.fresh_child(script, [str(tmp_path / "alone.npz")], {"FL_OBS_NO_FIX": "1", "FL_OBS_NO_TAB": "1", "FL_OBS_NOFIX": "1"}, 30, tag="alone")
    assert _started(tmp_path) == []
    sw.fresh_child(script, [str(tmp_path / "other.npz")], {"STANDIN_OTHER": "", "FL_OBS_NO_FIX": "1"}, 30)      # (another prefix is the caller's business)
    assert _started(tmp_path) == ["other"]


def test_the_child_sees_its_switches_and_no_others(script, tmp_path, monkeypatch):
    monkeypatch.setenv("FL_OBS_FOO", "1")
    monkeypatch.setenv("FL_OBS_NO_CF_DIRS", "1")
    monkeypatch.setenv("PYTHONPATH", "/somewhere/else")
    _, records = sw.run_switch_sets(script, SETS, tmp_path, 30)
    seen = {tag: r[("b0", "both")]["env"] for tag, r in records.items()}
    assert seen["default"] == {"PYTHONPATH": util.ROOT}
    assert seen["second"] == {"PYTHONPATH": util.ROOT, "FL_OBS_NO_FIX": "1"} and seen["third"] == {"PYTHONPATH": util.ROOT, "FL_OBS_NO_CF_DIRS": "1"}
    lines = sw.fresh_child(script, [str(tmp_path / "alone.npz")], {"FL_OBS_TSHIFT": "3"}, 30)
    assert lines[-1] == "DONE 2 tensors" and json.loads(lines[0].split(None, 3)[3])["env"] == {"PYTHONPATH": util.ROOT, "FL_OBS_TSHIFT": "3"}
