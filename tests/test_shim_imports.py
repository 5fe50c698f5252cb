"""CPU: the opt-in import shim (flatland_marl_amd/shim): the module names the reference's harness imports resolve to the
MI355X library, with the reference's signatures (a stored capture, re-checked against the real reference where it is mounted).
Importing the reference's own eval_env module through the shim needs the reference and runs in the build container only."""
import json
import os
import subprocess
import sys

import pytest

from tests import util

REF = "/root/reference"

DUMP = r'''
import inspect, json, sys
from flatland.envs.rail_env import RailEnv, TrainState
from flatland.envs.rail_env_action import RailEnvActions
from flatland.envs.step_utils.states import TrainState as TS2
from flatland.envs.rail_generators import SparseRailGen, sparse_rail_generator
from flatland.envs.line_generators import SparseLineGen, sparse_line_generator
from flatland.envs.malfunction_generators import MalfunctionParameters, ParamMalfunctionGen, NoMalfunctionGen
from flatland.envs.observations import TreeObsForRailEnv, Node
from flatland.envs.predictions import ShortestPathPredictorForRailEnv
from flatland.envs.persistence import RailEnvPersister
from flatland.core.env_observation_builder import ObservationBuilder
from flatland.core.grid.grid4 import Grid4TransitionsEnum
from flatland.core.grid.grid4_utils import get_new_position
from flatland_cutils import TreeObsForRailEnv as TreeCutils
assert TS2 is TrainState
def params(f):
    return [p for p in inspect.signature(f).parameters if p != "self"]
out = dict(
    railenv_init=params(RailEnv.__init__), railenv_reset=params(RailEnv.reset), railenv_step=params(RailEnv.step),
    railenv_action_required=params(RailEnv.action_required), sparse_rail=params(SparseRailGen.__init__),
    sparse_line=params(SparseLineGen.__init__), malf_fields=list(MalfunctionParameters._fields),
    node_fields=list(Node._fields), treeobs_init=params(TreeObsForRailEnv.__init__),
    predictor_init=params(ShortestPathPredictorForRailEnv.__init__),
    train_state={m.name: int(m.value) for m in TrainState}, actions={m.name: int(m.value) for m in RailEnvActions},
    grid4={m.name: int(m.value) for m in Grid4TransitionsEnum}, new_pos=list(get_new_position((3, 4), 1)),
    obs_builder_methods=sorted(n for n in ("set_env", "reset", "get_many", "get") if hasattr(ObservationBuilder, n)),
    cutils_methods=sorted(n for n in ("set_env", "reset", "get_many", "get_properties") if hasattr(TreeCutils, n)),
    persister=hasattr(RailEnvPersister, "load_new"),
    where=sys.modules["flatland"].__file__)
print("DUMP" + json.dumps(out))
'''


def _run(code, pythonpath):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DUMP")][-1][4:])


def _shim():
    return _run(DUMP, [os.path.join(util.ROOT, "flatland_marl_amd", "shim"), util.ROOT])


def test_harness_imports_resolve_to_the_library():
    d = _shim()
    assert os.path.join("flatland_marl_amd", "shim") in d["where"]
    assert d["railenv_init"][:10] == ["width", "height", "rail_generator", "line_generator", "number_of_agents", "obs_builder_object",
                                     "malfunction_generator_and_process_data", "malfunction_generator", "remove_agents_at_target",
                                     "random_seed"]
    assert d["railenv_reset"] == ["regenerate_rail", "regenerate_schedule", "random_seed"] and d["railenv_step"] == ["action_dict_"]
    assert d["train_state"] == dict(WAITING=0, READY_TO_DEPART=1, MALFUNCTION_OFF_MAP=2, MOVING=3, STOPPED=4, MALFUNCTION=5, DONE=6)
    assert d["cutils_methods"] == ["get_many", "get_properties", "reset", "set_env"] and d["persister"]


def test_install_puts_the_shim_first():
    code = ("import sys; sys.path.insert(0, %r); import flatland_marl_amd.shim as s; s.install(); import flatland, flatland_cutils; "
            "print('DUMP' + __import__('json').dumps(dict(where=flatland.__file__, cutils=flatland_cutils.__file__)))" % util.ROOT)
    d = _run(code, [])
    assert "shim" in d["where"] and "shim" in d["cutils"]


def test_signatures_equal_the_reference():
    """against the reference's signatures as captured by DUMP into tests/golden/reference_signatures.json; where the reference is
    mounted (with oracle/_ref built), that capture is first checked against a fresh DUMP of the reference itself"""
    ref = json.load(open(os.path.join(util.GOLD, "reference_signatures.json")))
    if os.path.isdir(os.path.join(REF, "flatland-rl")) and os.path.exists(os.path.join(util.ROOT, "oracle", "_ref")):
        live = _run(DUMP, [os.path.join(util.ROOT, "oracle", "refharness", "stubs"), os.path.join(REF, "flatland-rl"),
                           os.path.join(util.ROOT, "oracle", "_ref")])
        assert "reference" in live.pop("where")
        assert live == ref
    ours = _shim()
    for k in ("railenv_reset", "railenv_step", "railenv_action_required", "malf_fields", "node_fields", "train_state", "actions", "grid4",
              "new_pos", "obs_builder_methods", "cutils_methods", "treeobs_init", "predictor_init", "persister"):
        assert ours[k] == ref[k], k
    # constructors: the reference's parameters in the reference's order (ours may add keyword-only extras at the end)
    for k in ("railenv_init", "sparse_rail", "sparse_line"):
        assert ours[k][:len(ref[k])] == ref[k], (k, ours[k], ref[k])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "solution")), reason="needs the reference (build container only)")
def test_reference_eval_env_module_imports_unchanged_on_the_shim():
    """solution/eval_env.py:1-8 and the names solution/demo.py:4-12 imports, resolved through the shim (no GPU call is made)"""
    code = ("import eval_env, inspect; from flatland_cutils import TreeObsForRailEnv; "
            "assert eval_env.TreeCutils is TreeObsForRailEnv; "
            "w = eval_env.LocalTestEnvWrapper; "
            "print('DUMP' + __import__('json').dumps(dict(methods=sorted(n for n, _ in inspect.getmembers(w, inspect.isfunction)), "
            "file=eval_env.__file__)))")
    d = _run(code, [os.path.join(util.ROOT, "flatland_marl_amd", "shim"), util.ROOT, os.path.join(REF, "solution")])
    assert d["file"].startswith(REF)
    from flatland_marl_amd.rail_env import LocalTestEnvWrapper
    import inspect
    ours = sorted(n for n, _ in inspect.getmembers(LocalTestEnvWrapper, inspect.isfunction))
    # (`submit` belongs to the redis client of TestEnvWrapper: outside the hot path)
    assert [m for m in d["methods"] if m not in ours and m != "submit"] == [], "methods of the reference's wrapper our counterpart lacks"
