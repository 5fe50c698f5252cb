"""CPU: GlobalObsForRailEnv (flatland/envs/observations.py:535-611).  The numpy restatement (tests/global_obs_np.py) the GPU tests
check the kernel against equals the reference's own outputs (tests/golden/global_*.npz, tools/capture_global_obs.py) on every
sampled step of every fixture; the shim exports the class with the reference's constructor."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from tests.global_obs_np import global_obs, rail_obs

# the episode fixtures (global_states_*.npz are constructed states: tests/test_global_obs_states.py, tests/test_gpu_global_obs_states.py)
FIXTURES = sorted(os.path.basename(f)[len("global_"):-4] for f in glob.glob(os.path.join(util.GOLD, "global_*.npz"))
                  if not os.path.basename(f).startswith("global_states_"))


def test_the_fixtures_cover_what_the_issue_names():
    assert {"cfg0_tall_spfollow", "cfg1_malf20_spfollow", "cfg2_slow_trains", "cfg1_sparse", "cfg3_spfollow_malf100"} <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(name):
    g = util.load("global_" + name)
    fx = util.load(name)
    steps = g["steps"]
    assert g["agents_state"].dtype == np.float64 and g["targets"].dtype == np.float64
    assert np.array_equal(rail_obs(fx["grid"]), g["rail"])
    for k, t in enumerate(steps):
        exp_state = util.golden_state(fx, t - 1) if t > 0 else g["state"][k]
        assert np.array_equal(g["state"][k], exp_state), (name, t)
        r, ast, tgt = global_obs(util.static_of(fx), g["state"][k])
        assert np.array_equal(r, g["rail"])
        assert np.array_equal(ast, g["agents_state"][k]), (name, t)
        assert np.array_equal(tgt, g["targets"][k]), (name, t)


def test_the_goldens_hold_the_cases_that_matter():
    """DONE agents, MALFUNCTION_OFF_MAP, fractional speeds, malfunctions on the map, several agents counted on one start cell"""
    seen = set()
    for name in FIXTURES:
        g = util.load("global_" + name)
        st = g["state"][..., 3]
        seen |= {"done"} if (st == 6).any() else set()
        seen |= {"malf_off_map"} if (st == 2).any() else set()
        ast = g["agents_state"]
        seen |= {"ch4>1"} if (ast[..., 4] > 1).any() else set()
        seen |= {"fractional_speed"} if ((ast[..., 3] > 0) & (ast[..., 3] < 1)).any() else set()
        seen |= {"malf_on_map"} if (ast[..., 2] > 0).any() else set()
    assert seen == {"done", "malf_off_map", "ch4>1", "fractional_speed", "malf_on_map"}, seen


SHIM = r'''
import inspect, sys
from flatland.envs.observations import GlobalObsForRailEnv
import flatland_marl_amd.plugin as plugin
assert issubclass(GlobalObsForRailEnv, plugin.GlobalObsForRailEnv)
print("PARAMS", [p for p in inspect.signature(GlobalObsForRailEnv.__init__).parameters if p != "self"])
b = GlobalObsForRailEnv()
print("EMPTY", b.get_many(None) == {})
'''


def test_shim_exports_global_obs():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(util.ROOT, "flatland_marl_amd", "shim"), util.ROOT]),
               PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", SHIM], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # the reference's constructor takes no arguments (observations.py:553-554)
    assert "PARAMS []" in r.stdout and "EMPTY True" in r.stdout, r.stdout
