"""The table of observation-kernel cases: ONE row per runtime-carving kernel k_obs<MODE, VAR>, per split kernel that no other test pins and
per fallback value of a launcher option (ObsOptions of csrc/fl_obs_layout.h and what obs_pick_config of csrc/fl_obs.hip derives from them).
A helper module like tests/tree_lstm_forests.py, not a test: tests/test_obs_kernel_cases.py (CPU) asks the launcher's diagnostic what it
chooses for every row it models and asserts that the table is complete; tests/test_gpu_obs_kernel_cases.py (GPU) runs every row in a fresh
child process against the CPU oracle, bit for bit, and compares BatchedRailEnv.last_obs_launch() with the row.

A row:
  id        the pytest id
  recipe    the maps of the batch (RECIPES: the smallest shapes of the repository at which each path exists) -- B envs over them, each with its
            own RNG stream (workload.replica_rng) and malfunction rate 1 / 200
  call      ("cutils",) = obs_cutils(), ("both", depth) = obs_both(depth, 30), ("tree", depth) = obs_tree(depth, 30)
  handles   index of one of tests/golden/subset_cfg2.npz's handle lists: obs_cutils(handles=...) / obs_tree(depth, 30, handles) (None: every agent)
  max_nodes, pred_depth   the flatland_cutils builder's parameters (31 / 500 unless the row is about them)
  switches  the environment of the child (the launcher reads its switches once per process)
  expect    fields of BatchedRailEnv.last_obs_launch() the launch must report: always mode, var, fix, split, nt, and the option fields the row
            exists for.  mode / var / fix name the kernel: k_obs<mode, var> of launch class fix (0: the runtime carving), split 1: the class's split
            kernel (the class's body for the envs that fit it, the runtime-carving body for the others).

Adding a row: when build.sh gets a unit (a MODE, a class with a split kernel) or ObsOptions a field, add the rows that reach every new kernel and
both values of the field at the smallest recipe that does -- tools/print_obs_config.py and FL_OBS_VERBOSE show what the launcher chooses under a
set of switches without a GPU -- and extend RUNTIME_KERNELS / OPTION_VALUES below; the completeness tests of tests/test_obs_kernel_cases.py fail
until the table reaches them.
"""
import collections
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Row = collections.namedtuple("Row", "id recipe call handles max_nodes pred_depth switches expect")

# what the runtime-carving units of csrc/build.sh (fl_obs_m0 .. fl_obs_m8) instantiate: fl_obs_launch_mode<MODE> of csrc/fl_obs_unit.hip -- VAR 0 / 1 / 2
# of every MODE but k_obs<5, 1> (both builders in rounds of 16 agents never hold the static tables in LDS)
RUNTIME_MODES = tuple(range(9))
RUNTIME_KERNELS = frozenset((m, v) for m in RUNTIME_MODES for v in (0, 1, 2)) - {(5, 1)}
# the split kernels with a runtime-carving second body that no other test pins: (class, split)
SPLIT_KERNELS = frozenset({(2, 1), (4, 1)})
# every launcher option with a fallback, and the values the table must show: field of last_obs_launch() -> values
OPTION_VALUES = {"snext": (0, 1), "nh": (0, 1), "partial": (0, 1), "tmask": (0, 1), "dual": (0, 1), "items": (0, 1), "own_filter": (0, 1), "fb": (0, 1),
                 "bk_room": (0, 1), "wl_head": (0, "head"), "wl_bytes": (0, 8192, 24576), "nt": (256, 512, 1024), "tshift": (1, 3), "compact_t": (0, 1),
                 "tab": (0, 1), "raw": (0, 1), "label": (0, 1)}


def _static(name):
    from flatland_marl_amd import workload as wl
    return wl.load_static(name)


def _golden(name):
    from tests import util
    return util.static_of(util.load(name))


def _levels(test, levels):
    from flatland_marl_amd import workload as wl
    return [wl.generate_level(test, lv) for lv in levels]


# recipe -> (B, steps, the maps).  cfg1: 7 agents / 138 rail cells; cfg2: 20 agents / at most 213; cfg3: 80 agents / at most 231 (rounds of 32
# agents with a tail round of 16); tall: a map taller than wide (compact prediction keys: never the one-pass kernels); threeway: a cell with three ways
# on (DFS-slot node tables); two80: two levels of Test_5's row, 216 and 239 rail cells -- on either side of class 2's 232; cfg5x2: two levels of cfg5's
# row, 2 548 and 3 025 rail cells -- on either side of class 4's 2 816
RECIPES = {
    "cfg1": (4, 36, lambda: [_static("cfg1_uniform")]),
    "cfg2": (6, 32, lambda: [_static(n) for n in ("cfg2_uniform", "base_cfg2_L1", "base_cfg2_L2", "base_cfg2_L3", "base_cfg2_L4", "base_cfg2_L5")]),
    "cfg3": (4, 30, lambda: [_static(n) for n in ("cfg3_uniform", "base_cfg3_L1", "base_cfg3_L2", "base_cfg3_L3")]),
    "tall": (4, 36, lambda: [_golden("cfg0_tall_uniform"), _golden("cfg0_tall_spfollow")]),
    "threeway": (4, 36, lambda: [_golden("threeway_cfg2")]),
    "subset": (4, 36, lambda: [_golden("subset_cfg2")]),
    "two80": (4, 30, lambda: _levels("Test_5", (9, 1))),
    "cfg5x2": (2, 12, lambda: _levels("Test_13", (2, 1))),
}
SPLIT_RCAP = {2: 232, 4: 2816}    # rail cells of the classes with a split row (ObsFixed<k>::dims.Rcap of csrc/fl_obs_layout.h)


def maps_of(recipe):
    return RECIPES[recipe][2]()


def sizes_of(maps):
    """(agents, largest number of rail cells, largest number of unique targets, taller than wide, most ways on of a cell and direction <= 2)"""
    A = len(maps[0]["init_dir"])
    R = max(int((np.asarray(e["grid"]) != 0).sum()) for e in maps)
    U = max(len({tuple(t) for t in np.asarray(e["target"]).tolist()}) for e in maps)
    H, W = np.asarray(maps[0]["grid"]).shape
    return A, R, U, int(H > W)


def handle_lists():
    fx = np.load(os.path.join(GOLD, "subset_cfg2.npz"))
    return [fx["handles_%d" % k].tolist() for k in range(int(fx["n_lists"]))]


def _row(id, recipe, call, switches, kernel, nt=1024, handles=None, max_nodes=31, pred_depth=500, **options):
    mode, var, fix, split = kernel
    return Row(id, recipe, call, handles, max_nodes, pred_depth, dict(switches), dict(options, mode=mode, var=var, fix=fix, split=split, nt=nt))


ALONE, D2, D3 = ("cutils",), ("both", 2), ("both", 3)
NO_FIX = {"FL_OBS_NO_FIX": "1"}
# A runtime choice with the MODE, VAR and threads of class 2 / 4 / 9 takes that class's SPLIT kernel on a GPU (every env of these recipes fits the class: its body
# then builds them all, whatever the row's switches asked for).  The rows about such a choice itself rule the split out; the diagnostic of the CPU test,
# which knows no per-env sizes, never splits.
NO_SPLIT = {"FL_OBS_NO_SPLIT": "1"}
WIDE = {"FL_OBS_ROUND16": "2"}         # envs of at most 32 agents in rounds of 16, two workgroups a CU, whatever the batch
R16 = {"FL_OBS_ROUND16": "1"}          # ... envs of more than 32 agents


def _force(v, **more):
    return dict({"FL_OBS_FORCE": v}, **more)


ROWS = [
    # ---- no switch: the launch classes of the three shapes (the reference point of every row below)
    _row("cfg2-alone", "cfg2", ALONE, {}, (6, 0, 6, 0), compact_t=1, label=0),
    _row("cfg2-d2", "cfg2", D2, {}, (3, 0, 1, 0), dual=1, tab=0, raw=1),
    _row("cfg3-alone", "cfg3", ALONE, {}, (7, 0, 7, 0), fb=1),
    _row("cfg3-d3", "cfg3", D3, {}, (4, 0, 2, 0), fb=1, own_filter=1),
    # ---- the one-pass kernels on the runtime carving: MODE 3 / 4 / 5 (both builders), 6 / 7 / 8 (the flatland_cutils builder alone)
    _row("nofix-cfg2-alone", "cfg2", ALONE, NO_FIX, (6, 0, 0, 0), wl_bytes=24576, items=1, snext=1, partial=1),
    _row("nofix-cfg2-d2", "cfg2", D2, NO_FIX, (3, 0, 0, 0), wl_bytes=24576, nh=1, tmask=1, bk_room=0),
    _row("nofix-cfg3-alone", "cfg3", ALONE, NO_FIX, (7, 0, 0, 0)),
    _row("nofix-cfg3-d2", "cfg3", D2, NO_FIX, (4, 0, 0, 0), tshift=1),
    _row("nofix-wide-cfg2-alone", "cfg2", ALONE, dict(NO_FIX, **WIDE), (8, 0, 0, 0), nt=512),
    _row("nofix-wide-cfg2-d2", "cfg2", D2, dict(NO_FIX, **WIDE), (5, 0, 0, 0), nt=512),
    _row("nofix-r16-cfg3-alone", "cfg3", ALONE, dict(NO_FIX, **R16), (8, 0, 0, 0), nt=512),
    _row("nofix-r16-cfg3-d2", "cfg3", D2, dict(NO_FIX, **R16), (5, 2, 0, 0), nt=512, wl_bytes=0),
    # work lists in HBM scratch (VAR 2) with an LDS head of what the carving leaves
    _row("wl0-cfg2-alone", "cfg2", ALONE, _force("wl=0"), (6, 2, 0, 0), wl_bytes=0, wl_head="head"),
    _row("wl0-cfg2-d2", "cfg2", D2, _force("wl=0"), (3, 2, 0, 0), wl_bytes=0, wl_head="head"),
    _row("wl0-cfg3-d3", "cfg3", D3, _force("wl=0"), (4, 2, 0, 0), wl_bytes=0, wl_head="head"),
    _row("wl0-wide-cfg2-alone", "cfg2", ALONE, _force("wl=0", **WIDE), (8, 2, 0, 0), nt=512, wl_bytes=0),
    _row("wl0-wide-cfg2-d2", "cfg2", D2, _force("wl=0", **WIDE), (5, 2, 0, 0), nt=512, wl_bytes=0),
    _row("wl0-nohead-cfg2-d2", "cfg2", D2, _force("wl=0", FL_OBS_NO_WL_HEAD="1"), (3, 2, 0, 0), wl_bytes=0, wl_head=0),
    _row("wl0-nohead-cfg3-alone", "cfg3", ALONE, _force("wl=0", FL_OBS_NO_WL_HEAD="1"), (7, 2, 0, 0), wl_bytes=0, wl_head=0),
    _row("wl8k-cfg2-d2", "cfg2", D2, _force("wl=8192"), (3, 0, 0, 0), wl_bytes=8192),
    # the env's static tables in LDS (VAR 1)
    _row("tab-cfg2-alone", "cfg2", ALONE, _force("tab=1"), (6, 1, 0, 0), tab=1),
    _row("tab-cfg2-d2", "cfg2", D2, _force("tab=1"), (3, 1, 0, 0), tab=1),
    _row("tab-cfg3-alone", "cfg3", ALONE, _force("tab=1"), (7, 1, 0, 0), tab=1),
    _row("tab-cfg3-d2", "cfg3", D2, _force("tab=1,wl=24576"), (4, 1, 0, 0), tab=1, wl_bytes=24576),
    _row("tab-wide-cfg1-alone", "cfg1", ALONE, _force("tab=1", **WIDE), (8, 1, 0, 0), nt=512, tab=1),
    # both builders in rounds of 16 agents have no kernel with the tables in LDS: the switch leaves them where they are
    # (what is left is the default configuration of these envs: the exact class 5, which FL_OBS_FORCE does not rule out)
    _row("tab-wide-cfg1-d2", "cfg1", D2, _force("tab=1", **WIDE), (5, 0, 5, 0), nt=512, tab=0),
    # ---- the two-stage kernels: MODE 0 (the flatland_cutils builder), 2 (both builders), 1 (the upstream tree alone)
    _row("nomerge-cfg2-alone", "cfg2", ALONE, dict(NO_FIX, FL_OBS_NO_MERGE="1"), (0, 1, 0, 0), tab=1, compact_t=0),
    _row("nomerge-cfg2-d2", "cfg2", D2, dict(NO_FIX, FL_OBS_NO_MERGE="1"), (2, 1, 0, 0), tab=1, dual=1, compact_t=1),
    _row("nomerge-cfg3-d2", "cfg3", D2, dict(NO_FIX, FL_OBS_NO_MERGE="1"), (2, 0, 0, 0), tab=0, wl_bytes=24576),
    _row("nomerge-tab0-cfg2-alone", "cfg2", ALONE, _force("tab=0", FL_OBS_NO_MERGE="1"), (0, 0, 0, 0), tab=0),
    _row("nomerge-wl0-cfg2-alone", "cfg2", ALONE, _force("wl=0", FL_OBS_NO_MERGE="1", **NO_SPLIT), (0, 2, 0, 0), wl_bytes=0),
    _row("nomerge-wl0-cfg2-d2", "cfg2", D2, _force("wl=0", FL_OBS_NO_MERGE="1", **NO_SPLIT), (2, 2, 0, 0), wl_bytes=0),
    _row("tree-cfg2-d2", "cfg2", ("tree", 2), {}, (1, 1, 0, 0), tab=1, dual=0),
    _row("tree-tab0-cfg3-d3", "cfg3", ("tree", 3), _force("tab=0"), (1, 0, 0, 0), tab=0),
    _row("tree-wl0-cfg2-d3", "cfg2", ("tree", 3), _force("wl=0"), (1, 2, 0, 0), wl_bytes=0),
    # ---- the fallback value of every option
    _row("snext0-cfg2-alone", "cfg2", ALONE, _force("snext=0"), (0, 1, 0, 0), snext=0),
    _row("snext0-cfg2-d2", "cfg2", D2, _force("snext=0"), (2, 1, 0, 0), snext=0),
    _row("notmask-cfg2-alone", "cfg2", ALONE, _force("tmask=0,items=0", **NO_SPLIT), (0, 2, 0, 0), tmask=0, items=0),
    _row("notmask-cfg3-d2", "cfg3", D2, _force("tmask=0,items=0", **NO_SPLIT), (2, 2, 0, 0), tmask=0, items=0, dual=0),
    _row("nodual-cfg2-d2", "cfg2", D2, _force("dual=0", **NO_SPLIT), (2, 2, 0, 0), dual=0, items=1),
    _row("nopartial-cfg2-alone", "cfg2", ALONE, {"FL_OBS_NO_MERGE": "1", "FL_OBS_LDS_LIMIT": "90000"}, (0, 0, 0, 0), partial=0, tab=0),
    _row("nonh-cfg2-d2", "cfg2", D2, _force("nh=0"), (3, 0, 0, 0), nh=0),
    _row("lds64k-cfg2-d2", "cfg2", D2, {"FL_OBS_LDS_LIMIT": "65536"}, (2, 2, 0, 0), dual=0, nh=0),
    _row("lds64k-cfg3-alone", "cfg3", ALONE, {"FL_OBS_LDS_LIMIT": "65536"}, (7, 2, 0, 0), items=0),
    _row("lds48k-cfg3-alone", "cfg3", ALONE, {"FL_OBS_LDS_LIMIT": "49152"}, (0, 2, 0, 0), nt=512),
    _row("lds48k-cfg3-d2", "cfg3", D2, {"FL_OBS_LDS_LIMIT": "49152"}, (2, 2, 0, 0), nt=512),
    _row("nt512-cfg2-tree", "cfg2", ("tree", 2), {"FL_OBS_NT": "512"}, (1, 1, 0, 0), nt=512),
    _row("nt256-cfg2-alone", "cfg2", ALONE, {"FL_OBS_NT": "256"}, (0, 1, 0, 0), nt=256),
    _row("nt256-cfg3-d2", "cfg3", D2, {"FL_OBS_NT": "256"}, (2, 1, 0, 0), nt=256),
    _row("nt256-cfg3-tree", "cfg3", ("tree", 2), {"FL_OBS_NT": "256"}, (1, 1, 0, 0), nt=256),
    _row("noown-cfg2-d2", "cfg2", D2, {"FL_OBS_NO_OWN_FILTER": "1"}, (3, 0, 0, 0), own_filter=0, raw=0),
    _row("noown-cfg3-alone", "cfg3", ALONE, {"FL_OBS_NO_OWN_FILTER": "1"}, (7, 0, 0, 0), own_filter=0),
    _row("nofb-cfg3-d3", "cfg3", D3, dict({"FL_OBS_NO_FB": "1"}, **NO_SPLIT), (4, 0, 0, 0), fb=0, bk=0),
    # (the large-map configuration at cfg3's size: exactly class 9's options, and FL_OBS_FORCE leaves the exact classes allowed)
    _row("bk-cfg3-alone", "cfg3", ALONE, _force("wl=0,items=0,dual=0", FL_OBS_NO_MERGE="1"), (0, 2, 9, 0), bk_room=1, bk=1),
    _row("nobk-cfg3-alone", "cfg3", ALONE, _force("wl=0,items=0,dual=0", FL_OBS_NO_MERGE="1", FL_OBS_NO_BK="1", **NO_SPLIT), (0, 2, 0, 0), bk_room=0, bk=0),
    _row("tshift3-cfg2-d2", "cfg2", D2, {"FL_OBS_TSHIFT": "3"}, (3, 0, 0, 0), tshift=3),
    _row("tshift3-cfg3-alone", "cfg3", ALONE, {"FL_OBS_TSHIFT": "3"}, (7, 0, 0, 0), tshift=3),
    _row("nocompact-cfg2-d2", "cfg2", D2, {"FL_OBS_NO_COMPACT": "1"}, (2, 1, 0, 0), compact_t=0),
    _row("nocompact-cfg2-tree3", "cfg2", ("tree", 3), {"FL_OBS_NO_COMPACT": "1"}, (1, 1, 0, 0), compact_t=0),
    # ---- other builder parameters: 64-slot node tables (more than 32 nodes), a predictor horizon of one bucket word
    _row("nodes50-cfg2-alone", "cfg2", ALONE, {}, (0, 1, 0, 0), max_nodes=50),
    _row("pred60-cfg3-d2", "cfg3", D2, {}, (4, 0, 0, 0), pred_depth=60, fb=0),
    # ---- a handle subset: the stand-alone kernels' label path
    _row("subset-tab0-alone", "subset", ALONE, _force("tab=0"), (0, 0, 0, 0), handles=1, label=1),
    _row("subset-wl0-alone", "subset", ALONE, _force("wl=0"), (0, 2, 0, 0), handles=2, label=1),
    _row("subset-tab0-tree", "subset", ("tree", 2), _force("tab=0"), (1, 0, 0, 0), handles=1, label=1),
    _row("subset-wl0-tree", "subset", ("tree", 2), _force("wl=0"), (1, 2, 0, 0), handles=7, label=1),
    # ---- maps the one-pass kernels never take
    _row("tall-alone", "tall", ALONE, {"FL_OBS_NO_BINS": "1"}, (0, 1, 0, 0), compact_t=0),
    _row("tall-d3", "tall", D3, {"FL_OBS_NO_BINS": "1"}, (2, 1, 0, 0), compact_t=1),
    _row("threeway-d2", "threeway", D2, {}, (2, 1, 0, 0), compact_t=0),
    _row("threeway-d3", "threeway", D3, {}, (2, 1, 0, 0), compact_t=0),
    _row("threeway-tree3", "threeway", ("tree", 3), {}, (1, 1, 0, 0), compact_t=0),
    # ---- the split kernels with a runtime-carving body: the class's body for the envs that fit, k_obs<4,0> / k_obs<2,2> for the larger level
    _row("split-two80-d3", "two80", D3, {"FL_OBS_NO_BINS": "1"}, (4, 0, 2, 1)),
    _row("split-cfg5x2-d3", "cfg5x2", D3, {"FL_OBS_NO_BINS": "1"}, (2, 2, 4, 1), snext=0, bk_room=1),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def cpu_modelled(row):
    """the rows fl_debug_obs_config_of[_wide] models: the flatland_cutils builder alone or both builders, 31 nodes, every agent listed"""
    return row.call[0] in ("cutils", "both") and row.max_nodes == 31 and row.handles is None
