"""The fixtures of tools/capture_predictions.py (tests/golden/predictions_*.npz) as a list of groups, for the CPU and the GPU tests:
a group is one map with its agents (a hand-made map, one constructed case, one episode) and S recorded states."""
import glob
import os

import numpy as np

from tests import util

SOURCES = ("handmaps", "states_yard_small", "states_yard_crowd", "states_crossing_small", "states_crossing_crowd", "episodes")
STATIC = ("grid", "init_pos", "init_dir", "target", "speed", "dm", "slot")
KINDS = ("pred", "wp", "len", "dev", "devlen")
_cache = {}


def files():
    return sorted(os.path.basename(f)[len("predictions_"):-4] for f in glob.glob(os.path.join(util.GOLD, "predictions_*.npz")))


def groups(source):
    """[dict(source, name, grid, ..., steps, state [S, A, 12], depths, and per depth D: ("pred", D) ... ("devlen", D), extra)]"""
    if source not in _cache:
        z = np.load(os.path.join(util.GOLD, "predictions_%s.npz" % source))
        out = []
        for name in z["groups"]:
            name = str(name)
            g = {"source": source, "name": name}
            for k in STATIC + ("steps", "state"):
                g[k] = z[name + "/" + k]
            g["depths"] = [int(d) for d in z[name + "/depths"]]
            for D in g["depths"]:
                for k in KINDS:
                    g[(k, D)] = z["%s/%s_d%d" % (name, k, D)]
            g["extra"] = {k: z[name + "/" + k] for k in ("get3", "get0", "getnone", "get3_step") if name + "/" + k in z.files}
            out.append(g)
        _cache[source] = out
    return _cache[source]


def all_groups():
    return [g for s in SOURCES for g in groups(s)]


def static_of(g):
    """a static description BatchedRailEnv loads: the group's map and agents; what the prediction does not read (timetable, malfunction
    parameters, the RNG) is filled in"""
    return util.group_static(g)
