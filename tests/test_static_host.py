"""CPU: the host half of a handle -- what fl_load_env stages and refuses, the rail-cell index space fl_commit derives from it, the owner
election of the shared static tables (csrc/fl_static.h) -- through the library's fl_debug_static_* hook, which runs the functions that
fl_create / fl_load_env / fl_reserve / fl_commit call for their host side on an FlStatic alone.  No GPU, no torch: plain dlopen.  Every
expected value is derived here in numpy, or is the reference's own record in the base_* fixtures (dm_targets, target_slot)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # (the child process of the FL_NO_SHARED_TABLES test)
from flatland_marl_amd import hip_backend as hb  # noqa: E402
from tests import util  # noqa: E402

NONE = 0xFFFF
ARG, CAPACITY = 1, 6
DTYPES = dict(T="i4", mt_pos="i4", mt="u4", malf_thr="u8", malf_min="i4", malf_max="i4", U="i4", R="i4", K="i4", gridx="u4", ridx="u2",
              rgrid="u2", rtype="u1", nbr="u2", rkey="u2", rcell="u4", ut_r="u2", init_pos="i4", target="i4", init_r="u2", target_r="u2",
              srank="u2", earliest="i4", latest="i4", tslot="i4", spk="u4", speed="f8", grid="u2", ut="i4", maxbr="i4", loaded="u1",
              dirty="u1", key="u8", built="u8", tab="i4", need="u1", max_branch="i4", Ucap="i4", Rcap="i4")
STAGED = ("T", "mt_pos", "mt", "malf_thr", "malf_min", "malf_max", "U", "R", "init_pos", "target", "srank", "earliest", "latest", "tslot",
          "spk", "speed", "grid", "ut", "maxbr", "loaded", "dirty", "built")     # what fl_load_env writes


def _lib():
    return hb.bind(ctypes.CDLL(hb.LIB_PATH), ("flatland_hip.h", "debug"))       # plain dlopen: no torch, no GPU


class Static:
    """an FlStatic of the library"""

    def __init__(self, B, A, H, W):
        self.L, self.B, self.A, self.H, self.W = _lib(), B, A, H, W
        self.p = self.L.fl_debug_static_new(B, A, H, W)
        assert self.p

    def __del__(self):
        self.L.fl_debug_static_free(self.p)

    def load(self, b, env, **change):
        """fl_load_env's arguments from a static description; change: raw arguments that replace them (None: a null pointer)"""
        e = dict(env, **change)
        a = dict(grid=np.ascontiguousarray(e["grid"], dtype=np.uint16) if e["grid"] is not None else None,
                 speed=np.ascontiguousarray(e["speed"], dtype=np.float64) if e["speed"] is not None else None,
                 mt_key=np.ascontiguousarray(e["mt_key"], dtype=np.uint32) if e["mt_key"] is not None else None)
        for k in ("init_pos", "init_dir", "target", "earliest", "latest"):
            a[k] = np.ascontiguousarray(e[k], dtype=np.int32) if e[k] is not None else None
        p = lambda k: a[k].ctypes.data if a[k] is not None else None  # noqa: E731
        return self.L.fl_debug_static_load(self.p, b, p("grid"), p("init_pos"), p("init_dir"), p("target"), p("speed"), p("earliest"), p("latest"),
                                           int(e["T"]), e.get("malf_thr", hb.malf_threshold(float(e["malf_rate"]))), int(e["malf_min"]),
                                           int(e["malf_max"]), p("mt_key"), int(e["mt_pos"]))

    def reserve(self, U, R):
        return self.L.fl_debug_static_reserve(self.p, U, R)

    def commit(self):
        return self.L.fl_debug_static_commit(self.p)

    def error(self):
        return self.L.fl_last_error().decode()

    def read(self, name, b=-1):
        n = self.L.fl_debug_static_read(self.p, name.encode(), b, ctypes.byref(ctypes.c_char()), 0)
        assert n >= 0, name
        out = np.zeros(n, dtype=np.uint8)
        assert self.L.fl_debug_static_read(self.p, name.encode(), b, out.ctypes.data, n) == n
        return out.view(DTYPES[name])

    def staged(self, b=-1):
        return {k: self.read(k, b).tobytes() for k in STAGED}


# ---- transitions: bit (3 - d) * 4 + (3 - m) of a cell = "an agent facing d may leave towards m" (N, E, S, W)
BASIC = (0x0000, 0x8020, 0x9220, 0x8421, 0x9621, 0xCC33, 0x5202, 0x2000, 0x4002, 0x1200, 0xC022)    # rail_env_grid.py:28-38


def rot(cell, k):
    """the cell turned by k quarter turns: facing d + k it leaves towards m + k where it left towards m facing d"""
    out = 0
    for d in range(4):
        for m in range(4):
            if (cell >> ((3 - d) * 4 + (3 - m))) & 1:
                out |= 1 << ((3 - (d + k) % 4) * 4 + (3 - (m + k) % 4))
    return out


def road_type(cell):
    """loader.cpp:122-161: the first basic transition that the cell, or else its turn by one, two, three quarters, equals"""
    for k in range(4):
        if rot(cell, k) in BASIC:
            return BASIC.index(rot(cell, k))
    return 0


NS, EW, CROSS, SWITCH = 0x8020, rot(0x8020, 1), 0x8421, 0x9220


def description(grid, agents, speed=None, **kw):
    """agents: rows (row, col, dir, target row, target col)"""
    a = np.array(agents, dtype=np.int32)
    A = len(a)
    d = dict(grid=np.array(grid, dtype=np.uint16), init_pos=a[:, 0:2].copy(), init_dir=a[:, 2].copy(), target=a[:, 3:5].copy(),
             speed=np.array(speed if speed is not None else [1.0] * A, dtype=np.float64), earliest=np.arange(A, dtype=np.int32),
             latest=np.arange(A, dtype=np.int32) + 50, T=100, malf_rate=0.01, malf_min=2, malf_max=9,
             mt_key=np.arange(624, dtype=np.uint32) * 7 + 1, mt_pos=17)
    d.update(kw)
    return d


def wide_env():
    """3 x 5: a line through row 1 crossed by a line through column 2; four agents, two of them to one target"""
    g = np.zeros((3, 5), dtype=np.uint16)
    g[1, :] = EW
    g[0, 2] = g[2, 2] = NS
    g[1, 2] = CROSS
    return description(g, [(1, 0, 1, 1, 4), (0, 2, 2, 2, 2), (1, 4, 3, 1, 0), (1, 1, 1, 1, 4)], speed=[1.0, 0.5, 0.5, 1.0 / 3])


def tall_env():
    """5 x 3: a line through column 1 crossed by a line through row 3.  (3, 0) and (0, 1) both have the key col * W + row = 3"""
    g = np.zeros((5, 3), dtype=np.uint16)
    g[:, 1] = NS
    g[3, 0] = g[3, 2] = EW
    g[3, 1] = CROSS
    return description(g, [(0, 1, 2, 4, 1), (3, 0, 1, 3, 2), (4, 1, 0, 0, 1)], speed=[0.25, 1.0, 0.25])


def derive(env, Rcap, Ucap):
    """the arrays of one env, from its static description"""
    grid = np.asarray(env["grid"], dtype=np.uint16)
    H, W = grid.shape
    flat = grid.ravel()
    cells = np.flatnonzero(flat)
    R = len(cells)
    x = {"R": [R], "grid": flat}
    ridx = np.full(H * W, NONE, dtype=np.uint16)
    ridx[cells] = np.arange(R)
    x["ridx"] = ridx
    x["rcell"] = np.zeros(Rcap, dtype=np.uint32)
    x["rcell"][:R] = cells
    x["rgrid"] = np.zeros(Rcap, dtype=np.uint16)
    x["rgrid"][:R] = flat[cells]
    x["rtype"] = np.array([road_type(int(c)) for c in flat[cells]], dtype=np.uint8)        # (compared up to R)
    framed = np.pad(ridx.reshape(H, W), 1, constant_values=NONE)       # the map's border has no rail
    row, col = cells // W + 1, cells % W + 1
    x["nbr"] = np.full((Rcap, 4), NONE, dtype=np.uint16)
    x["nbr"][:R] = np.stack([framed[row - 1, col], framed[row, col + 1], framed[row + 1, col], framed[row, col - 1]], axis=1)
    rail = framed != NONE
    x["gridx"] = (grid.astype(np.uint32) | rail[:-2, 1:-1] << 16 | rail[1:-1, 2:] << 17 | rail[2:, 1:-1] << 18 | rail[1:-1, :-2] << 19).ravel()
    if H > W:       # the prediction keys col * W + row collide on a tall map: equal keys share one compact key, in ascending order
        keys = (cells % W) * W + cells // W
        uniq = np.unique(keys)
        x["K"] = [len(uniq)]
        x["rkey"] = np.zeros(Rcap, dtype=np.uint16)
        x["rkey"][:R] = np.searchsorted(uniq, keys)
    else:
        x["K"], x["rkey"] = [R], np.zeros(0, dtype=np.uint16)
    ip = np.asarray(env["init_pos"])
    tg = np.asarray(env["target"])
    x["init_pos"], x["target"] = ip[:, 0] * W + ip[:, 1], tg[:, 0] * W + tg[:, 1]
    x["init_r"], x["target_r"] = ridx[x["init_pos"]], ridx[x["target"]]
    ut = []
    for t in x["target"]:       # unique targets in first-seen order (distance_map.py:71-79)
        if t not in ut:
            ut.append(int(t))
    x["U"], x["tslot"] = [len(ut)], [ut.index(t) for t in x["target"]]
    x["ut_r"] = np.zeros(Ucap, dtype=np.uint16)
    x["ut_r"][:len(ut)] = ridx[ut]
    speed = np.asarray(env["speed"], dtype=np.float64)
    x["speed"] = speed
    x["srank"] = [(speed < s).sum() for s in speed]
    x["spk"] = [int(d) | (int(1.0 / s) - 1) << 2 for d, s in zip(env["init_dir"], speed)]
    x["maxbr"] = [max(bin((int(c) >> 4 * d) & 15).count("1") for c in flat for d in range(4))]
    x["earliest"], x["latest"], x["T"], x["mt"], x["mt_pos"] = env["earliest"], env["latest"], [env["T"]], env["mt_key"], [env["mt_pos"]]
    x["malf_thr"], x["malf_min"], x["malf_max"] = [hb.malf_threshold(float(env["malf_rate"]))], [env["malf_min"]], [env["malf_max"]]
    return x, ut


def committed(envs, reserve=None):
    e0 = envs[0]
    s = Static(len(envs), len(e0["init_dir"]), *np.asarray(e0["grid"]).shape)
    if reserve:
        assert s.reserve(*reserve) == 0, s.error()
    for b, e in enumerate(envs):
        assert s.load(b, e) == 0, s.error()
    assert s.commit() == 0, s.error()
    return s


def check_tables(s, envs):
    Rcap, Ucap = int(s.read("Rcap", 0)[0]), int(s.read("Ucap", 0)[0])
    assert Rcap == max(max(np.count_nonzero(e["grid"]) for e in envs), 1)
    for b, e in enumerate(envs):
        x, ut = derive(e, Rcap, Ucap)
        R = x["R"][0]
        for name, want in x.items():
            got = s.read(name, b)
            want = np.asarray(want).ravel().astype(DTYPES[name])
            if name == "rtype":
                got = got[:R]
            assert got.tobytes() == want.tobytes(), (b, name, got, want)
        assert s.read("ut", b)[:len(ut)].tolist() == ut
    return Rcap, Ucap


# ---------------------------------------------------------------------------------------------------------------- rail tables
@pytest.mark.parametrize("cfg", ["base_cfg2", "base_cfg3"])
def test_rail_tables_of_the_base_fixtures_are_the_numpy_derivation_and_the_references_targets(cfg):
    fxs = [util.load(n) for n in util.base_fixtures(cfg)]
    assert len(fxs) >= 3
    envs = [util.static_of(fx) for fx in fxs]
    s = committed(envs)
    Rcap, Ucap = check_tables(s, envs)
    assert Ucap == max(len(fx["dm_targets"]) for fx in fxs) and len({np.count_nonzero(fx["grid"]) for fx in fxs}) > 1    # (envs below the capacity)
    W = s.W
    for b, fx in enumerate(fxs):    # what the reference recorded
        U = len(fx["dm_targets"])
        assert s.read("U", b)[0] == U
        assert s.read("tslot", b).tolist() == fx["target_slot"].tolist()
        assert s.read("ut", b)[:U].tolist() == (fx["dm_targets"][:, 0] * W + fx["dm_targets"][:, 1]).tolist()
        assert s.read("K", b)[0] == s.read("R", b)[0] == np.count_nonzero(fx["grid"]) and s.read("rkey", b).size == 0
    assert s.read("max_branch", 0)[0] == 2


def test_rail_tables_of_a_wide_hand_made_grid():
    e = wide_env()
    s = committed([e])
    assert check_tables(s, [e]) == (7, 3)
    assert s.read("ridx").tolist() == [NONE, NONE, 0, NONE, NONE, 1, 2, 3, 4, 5, NONE, NONE, 6, NONE, NONE]
    assert s.read("nbr").reshape(7, 4).tolist() == [[NONE, NONE, 3, NONE], [NONE, 2, NONE, NONE], [NONE, 3, NONE, 1], [0, 4, 6, 2],
                                                     [NONE, 5, NONE, 3], [NONE, NONE, NONE, 4], [3, NONE, NONE, NONE]]
    assert (s.read("gridx") >> 16).tolist() == [4, 6, 4, 12, 4, 2, 10, 15, 10, 8, 1, 3, 1, 9, 1]      # bit m: rail towards m
    assert s.read("tslot").tolist() == [0, 1, 2, 0] and s.read("ut_r").tolist() == [5, 6, 1]
    assert s.read("init_r").tolist() == [1, 0, 5, 2] and s.read("target_r").tolist() == [5, 6, 1, 5]
    assert s.read("K")[0] == 7 and s.read("rkey").size == 0


def test_rail_tables_of_a_tall_hand_made_grid_share_prediction_keys():
    e = tall_env()
    assert e["grid"][3, 0] and e["grid"][0, 1]          # both have the key col * W + row = 3
    s = committed([e])
    assert check_tables(s, [e]) == (7, 3)
    assert s.read("R")[0] == 7 and s.read("K")[0] == 6            # K < R: two cells share a key
    # rail cells (0,1) (1,1) (2,1) (3,0) (3,1) (3,2) (4,1) -> keys 3 4 5 3 6 9 7
    assert s.read("rkey").tolist() == [0, 1, 2, 0, 3, 5, 4]


def test_road_types_of_every_basic_transition_and_its_rotations():
    assert [road_type(c) for c in BASIC] == list(range(11))
    g = np.zeros((4, 11), dtype=np.uint16)
    for k in range(4):
        g[k] = [rot(c, k) for c in BASIC]
    e = description(g, [(0, 1, 0, 3, 10)])
    s = committed([e])
    got = s.read("rtype")[:40].reshape(4, 10)
    assert got.tolist() == [[road_type(int(c)) for c in row[1:]] for row in g]
    assert got[0].tolist() == list(range(1, 11))
    assert got[1].tolist() == [1, 2, 3, 4, 5, 6, 7, 9, 8, 10]          # (the curves 8 and 9 are quarter turns of each other)


def test_speed_ranks_with_ties_and_speed_counters():
    speed = [0.5, 1.0, 0.5, 1.0 / 3, 1.0 / 64, 1.0, 1.0 / 3]
    g = np.zeros((3, 5), dtype=np.uint16)
    g[1, :] = EW
    e = description(g, [(1, a % 5, a % 4, 1, 4) for a in range(7)], speed=speed)
    s = committed([e])
    assert s.read("srank").tolist() == [3, 5, 3, 1, 0, 5, 1]          # agents with a smaller speed; ties share a rank
    assert (s.read("spk") >> 2).tolist() == [1, 0, 1, 2, 63, 0, 2]      # SpeedCounter.max_count = int(1 / speed) - 1
    assert (s.read("spk") & 3).tolist() == [0, 1, 2, 3, 0, 1, 2]
    assert s.read("speed").tolist() == speed


def test_max_branch_is_the_most_transitions_of_any_cell_and_direction():
    def of(*cells):
        g = np.zeros((3, 5), dtype=np.uint16)
        g[1, :len(cells)] = cells
        s = committed([description(g, [(1, 0, 1, 1, 0)])])
        return int(s.read("max_branch")[0])
    assert of(EW, CROSS, EW) == 1           # a diamond crossing: one way on from every direction
    assert of(EW, CROSS, SWITCH) == 2
    assert of(EW, rot(0xCC33, 1), EW) == 2
    assert of(EW, 0x00E0, SWITCH) == 3      # (no Flatland cell type: three ways on facing south)


def test_max_branch_of_a_batch_is_its_largest_env():
    a, b = wide_env(), wide_env()
    b["grid"] = b["grid"].copy()
    b["grid"][1, 3] = SWITCH
    s = committed([a, b, a])
    assert s.read("maxbr").tolist() == [1, 2, 1] and s.read("max_branch", 0)[0] == 2


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(s, b, env, code, message, **change):
    before = s.staged()
    assert s.load(b, env, **change) == code, (change, s.error())
    assert s.error() == message
    assert s.staged() == before, change         # a refused call leaves every env's staged copy as it was


def loaded_pair():
    s = Static(2, 4, 3, 5)
    e = wide_env()
    for b in range(2):
        assert s.load(b, e) == 0
    return s, e


def test_load_refuses_env_index_null_arguments_rng_position_and_malfunction_range():
    s, e = loaded_pair()
    for b in (-1, 2):
        refused(s, b, e, ARG, "fl_load_env: env index out of range")
    for k in ("grid", "init_pos", "init_dir", "target", "speed", "earliest", "latest", "mt_key"):
        refused(s, 1, e, ARG, "fl_load_env: null argument", **{k: None})
    for pos in (-1, 625):
        refused(s, 1, e, ARG, "fl_load_env: mt_pos out of range", mt_pos=pos)
    assert s.load(1, e, mt_pos=0) == 0 and s.load(1, e, mt_pos=624) == 0
    for lo, hi in ((5, 4), (-1, 4), (0, 60001)):
        refused(s, 1, e, ARG, "fl_load_env: bad malfunction duration range", malf_min=lo, malf_max=hi)
    assert s.load(1, e, malf_min=0, malf_max=60000) == 0 and s.load(1, e, malf_min=7, malf_max=7) == 0


def test_load_refuses_positions_directions_and_cells_without_rail():
    s, e = loaded_pair()

    def agents(i, col, value, key):
        a = e[key].copy()
        if a.ndim == 2:
            a[i, col] = value
        else:
            a[i] = value
        return {key: a}
    for i, change in ((0, agents(0, 0, 3, "init_pos")), (1, agents(1, 0, -1, "init_pos")), (2, agents(2, 1, 5, "init_pos")), (3, agents(3, 1, -1, "init_pos")),
                      (0, agents(0, 0, 3, "target")), (1, agents(1, 0, -1, "target")), (2, agents(2, 1, 5, "target")), (3, agents(3, 1, -1, "target")),
                      (1, agents(1, 0, 4, "init_dir")), (2, agents(2, 0, -1, "init_dir"))):
        refused(s, 1, e, ARG, "fl_load_env: agent %d position/direction out of range" % i, **change)
    for i, change in ((0, agents(0, 0, 0, "init_pos")), (3, agents(3, 0, 2, "target"))):       # (0, 0) and (2, 4) have no rail
        refused(s, 1, e, ARG, "fl_load_env: agent %d starts or ends on a cell without rail" % i, **change)


def test_load_refuses_speeds_outside_the_supported_range():
    s, e = loaded_pair()

    def speed(i, v):
        a = e["speed"].copy()
        a[i] = v
        return a
    for i, v in ((0, 0.0), (2, 1.5), (3, -0.25), (1, float("nan"))):
        refused(s, 1, e, ARG, "fl_load_env: agent %d speed %g not in (0, 1]" % (i, v), speed=speed(i, v))
    refused(s, 1, e, ARG, "fl_load_env: agent 2 speed %g unsupported (max_count 64)" % (1.0 / 65), speed=speed(2, 1.0 / 65))
    assert s.load(1, e, speed=speed(2, 1.0 / 64)) == 0 and s.load(1, e, speed=speed(2, 1.0)) == 0


def test_load_refuses_more_rail_cells_than_u16_rail_states():
    g = np.full((128, 129), EW, dtype=np.uint16)
    g.ravel()[16383:] = 0
    e = description(g, [(0, 0, 1, 0, 1)])
    s = Static(1, 1, 128, 129)
    assert s.load(0, e) == 0 and s.read("R")[0] == 16383
    for n in (16384, 128 * 129):
        g.ravel()[:n] = EW
        refused(s, 0, e, ARG, "fl_load_env: %d rail cells exceed the u16 rail-state / distance range" % n, grid=g)


def test_load_after_a_commit_refuses_an_env_beyond_the_committed_capacities():
    e = wide_env()
    s = committed([e, e])
    g = e["grid"].copy()
    g[0, 0] = NS
    refused(s, 1, e, CAPACITY, "fl_load_env: env 1 has 3 unique targets / 8 rail cells, the batch was committed for 3 / 7 (fl_reserve)", grid=g)
    t = e["target"].copy()
    t[3] = (0, 2)
    refused(s, 0, e, CAPACITY, "fl_load_env: env 0 has 4 unique targets / 7 rail cells, the batch was committed for 3 / 7 (fl_reserve)", target=t)
    g[0, 0], g[1, 0] = 0, 0         # fewer cells, fewer targets: accepted
    assert s.load(1, e, grid=g, init_pos=np.array([(1, 1)] * 4), target=np.array([(1, 4)] * 4)) == 0 and s.commit() == 0
    # with room reserved before the first commit both fit
    s = committed([e, e], reserve=(4, 8))
    assert s.load(0, e, target=t) == 0 and s.load(1, e, grid=e["grid"] | (np.arange(15).reshape(3, 5) == 0) * np.uint16(NS)) == 0
    assert s.commit() == 0 and (s.read("Ucap", 0)[0], s.read("Rcap", 0)[0]) == (4, 8)


def test_reserve_and_commit_refusals():
    s, e = loaded_pair()
    assert s.reserve(-1, 3) == ARG and s.error() == "fl_reserve: bad argument"
    assert s.reserve(3, 16384) == ARG and s.error() == "fl_reserve: at most 16383 rail cells per env (u16 rail states)"
    fresh = Static(2, 4, 3, 5)
    assert fresh.load(0, e) == 0
    assert fresh.commit() == ARG and fresh.error() == "fl_commit: env 1 was never loaded"
    assert s.commit() == 0
    assert s.reserve(3, 7) == ARG and s.error() == "fl_reserve: the capacities are fixed at the first fl_commit"


# ---------------------------------------------------------------------------------------------------------------- owner election
def _rng(b):
    st = np.random.RandomState([b]).get_state()
    return np.array(st[1], dtype=np.uint32), int(st[2])


def shared_batch(which=(0, 1, 0, 1, 0, 1)):
    """the batch of tests/test_gpu_reload.py::test_envs_of_one_map_share_their_static_tables_through_replacements"""
    bases = [util.load("base_cfg2_L%d" % k) for k in range(1, 4)]
    U = max(len(fx["dm_targets"]) for fx in bases)
    R = max(int((fx["grid"] != 0).sum()) for fx in bases)
    envs = [util.static_of(bases[m], *_rng(1700 + b)) for b, m in enumerate(which)]
    return committed(envs, reserve=(U, R)), bases, envs


def owners(s):
    return s.read("tab").tolist(), s.read("need").tolist()


def test_owners_of_the_shared_tables_through_replacements():
    s, bases, envs = shared_batch()
    assert owners(s) == ([0, 1, 0, 1, 0, 1], [1, 1, 0, 0, 0, 0])

    def replace(b, m, k):
        envs[b] = util.static_of(bases[m], *_rng(k))
        assert s.load(b, envs[b]) == 0 and s.commit() == 0
        return owners(s)
    # the owner of map 0's tables gets map 2: env 2 now owns map 0's (never built so far)
    assert replace(0, 2, 1800) == ([0, 1, 2, 1, 2, 1], [1, 0, 1, 0, 0, 0])
    # env 3 joins map 2 (owner: env 0, built): nothing to build
    assert replace(3, 2, 1801) == ([0, 1, 2, 0, 2, 1], [0, 0, 0, 0, 0, 0])
    # the new owner of map 0 leaves too: env 4 is the last one on it, and its slabs were never built
    assert replace(2, 1, 1802) == ([0, 1, 1, 0, 4, 1], [0, 0, 0, 0, 1, 0])
    # the tables of every env are those of its own description all along
    maps = [2, 1, 1, 2, 0, 1]
    check_tables(s, envs)
    key = s.read("key")
    assert all((key[a] == key[b]) == (maps[a] == maps[b]) for a in range(6) for b in range(6))
    assert s.read("built").tolist() == [key[0], key[1], 0, 0, key[4], 0] and not s.read("dirty").any()


def test_a_commit_with_nothing_loaded_since_the_last_one_changes_nothing():
    s = shared_batch()[0]
    names = [n for n in DTYPES if n != "rkey"]
    before = {n: s.read(n).tobytes() for n in names}
    assert s.commit() == 0
    assert {n: s.read(n).tobytes() for n in names} == before


def test_reloading_the_same_content_builds_nothing_another_grid_in_between_does():
    s, bases, _ = shared_batch()
    same = util.static_of(bases[0], *_rng(5))           # the owner's own map again, another RNG stream
    assert s.load(0, same) == 0 and s.read("dirty").tolist() == [1, 0, 0, 0, 0, 0] and s.commit() == 0
    assert owners(s) == ([0, 1, 0, 1, 0, 1], [0] * 6)
    assert s.read("mt", 0).tolist() == _rng(5)[0].tolist()
    assert s.load(0, util.static_of(bases[2])) == 0 and s.load(0, same) == 0 and s.commit() == 0     # whatever its slabs held is stale
    assert owners(s) == ([0, 1, 0, 1, 0, 1], [1, 0, 0, 0, 0, 0])
    # other unique targets on the same grid are other content as well
    other = dict(same, target=same["target"][::-1].copy())
    assert s.load(4, other) == 0 and s.commit() == 0
    assert owners(s) == ([0, 1, 0, 1, 4, 1], [0, 0, 0, 0, 1, 0])


def test_no_shared_tables_switch_makes_every_env_its_own_owner():
    """FL_NO_SHARED_TABLES is read once per process: a child process"""
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, FL_NO_SHARED_TABLES="1"), cwd=os.path.dirname(os.path.abspath(__file__)))
    assert json.loads(out) == [[0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1, 1]]


if __name__ == "__main__":
    print(json.dumps(owners(shared_batch()[0])))
