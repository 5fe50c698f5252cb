"""GPU: ShortestPathPredictorForRailEnv.get() / get_shortest_paths through every layer -- fl_predict (flatland_marl_amd/csrc/fl_predict.h),
BatchedRailEnv.predictions / MixedBatch.predictions, rail_env.ShortestPathPredictorForRailEnv on this library's RailEnv and
plugin.ShortestPathPredictorForRailEnv on a duck-typed env -- against the reference's own outputs (tests/golden/predictions_*.npz) and,
at depths and sizes no fixture covers, against the numpy restatement that tests/test_predictions.py pins to those fixtures.
Everything is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import predictions_cases as pc
from tests import predictions_np as pn
from tests import util

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 7, 8, 9, 16, 17, 30, 500)      # the edges of an eight-hop walk and of a 32-lane tile of rows, and the limit


def _by_shape(groups):
    shapes = {}
    for g in groups:
        shapes.setdefault(g["grid"].shape + (len(g["slot"]),), []).append(g)
    return shapes


def _check_groups(env, gs, pick=None):
    """every recorded state and depth of the groups gs (env b = group b; pick(result, b) selects env b's slice)"""
    import torch
    pick = pick or (lambda r, b: r[b])
    S = max(len(g["steps"]) for g in gs)
    for s in range(S):
        env.set_state(np.stack([g["state"][min(s, len(g["steps"]) - 1)] for g in gs]))
        for D in sorted({d for g in gs for d in g["depths"]}):
            pred, wp, ln = (x.cpu().numpy() for x in env.predictions(D, paths=True))
            p32 = env.predictions(D, torch.int32).cpu().numpy()
            for b, g in enumerate(gs):
                if D not in g["depths"]:
                    continue
                k = min(s, len(g["steps"]) - 1)
                msg = "%s state %d depth %d" % (g["name"], k, D)
                util.same(pick(pred, b), g[("pred", D)][k], msg + " float64", dtype=True)
                util.same(pick(p32, b), g[("pred", D)][k].astype(np.int32), msg + " int32", dtype=True)
                util.same(pick(wp, b), g[("wp", D)][k], msg + " waypoints", dtype=True)
                util.same(pick(ln, b), g[("len", D)][k], msg + " length", dtype=True)
    env.check()


@pytest.mark.parametrize("source", pc.SOURCES)
def test_fixtures_batched_per_shape(source):
    """the groups of one shape are the envs of one handle: states through fl_set_state, both element kinds and the paths"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    for shape, gs in _by_shape(pc.groups(source)).items():
        env = BatchedRailEnv([pc.static_of(g) for g in gs])
        _check_groups(env, gs)
        env.close()


@pytest.mark.parametrize("source", ("handmaps", "states_crossing_crowd", "episodes"))
def test_fixtures_alone_with_one_env(source):
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    for g in pc.groups(source):
        env = BatchedRailEnv([pc.static_of(g)])
        _check_groups(env, [g])
        env.close()


def test_handmaps_in_one_mixed_batch():
    import torch
    from flatland_marl_amd.hip_backend import MixedBatch
    gs = pc.groups("handmaps")
    mb = MixedBatch([pc.static_of(g) for g in gs])
    assert len(mb.groups) > 1
    for s in (0, 2):
        per = [[] for _ in mb.groups]
        for i, g in enumerate(gs):
            per[mb.where[i][0]].append(g["state"][min(s, len(g["steps"]) - 1)])
        for grp, rows in zip(mb.groups, per):
            grp.set_state(np.stack(rows))
        for D in (8, 30):
            out = mb.predictions(D, paths=True)
            o32 = mb.predictions(D, torch.int32)
            assert len(out) == len(mb.groups)
            for i, g in enumerate(gs):
                k = min(s, len(g["steps"]) - 1)
                pred, wp, ln = mb.pick(i, out)
                util.same(pred.cpu().numpy(), g[("pred", D)][k], "mixed %s depth %d" % (g["name"], D), dtype=True)
                util.same(wp.cpu().numpy(), g[("wp", D)][k], "mixed %s waypoints" % g["name"], dtype=True)
                util.same(ln.cpu().numpy(), g[("len", D)][k], "mixed %s length" % g["name"], dtype=True)
                util.same(mb.pick(i, o32).cpu().numpy(), g[("pred", D)][k].astype(np.int32), "mixed %s int32" % g["name"], dtype=True)
    mb.check()
    mb.close()


def _restated(env, statics, st, b, D, cache):
    key = (b, D)
    if key not in cache:
        if ("dm", b) not in cache:
            cache[("dm", b)] = env.distance_map(b)
        dm, slot = cache[("dm", b)]
        s = statics[b]
        cache[key] = pn.predict(s["grid"], dm, slot, s["init_pos"], s["target"], s["speed"], st[b], D)[:3]
    return cache[key]


def _check_against_restatement(env, statics, envs_checked, depths, msg):
    import torch
    st, _ = env.state()
    cache = {}
    for D in depths:
        pred, wp, ln = (x.cpu().numpy() for x in env.predictions(D, paths=True))
        p32 = env.predictions(D, torch.int32).cpu().numpy()
        for b in envs_checked:
            e_pred, e_wp, e_ln = _restated(env, statics, st, b, D, cache)
            util.same(pred[b], e_pred, "%s env %d depth %d float64" % (msg, b, D), dtype=True)
            util.same(p32[b], e_pred.astype(np.int32), "%s env %d depth %d int32" % (msg, b, D), dtype=True)
            util.same(wp[b], e_wp, "%s env %d depth %d waypoints" % (msg, b, D), dtype=True)
            util.same(ln[b], e_ln, "%s env %d depth %d length" % (msg, b, D), dtype=True)
    return st


@pytest.mark.parametrize("workload,steps", [("cfg1", 25), ("cfg2", 40)])
def test_depths_on_played_envs_sharing_static_tables(workload, steps):
    """replicas over a pool of maps (shared static tables, FlDev::tab), played with the on-device shortest-path stream"""
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs(workload, B=12)
    env = BatchedRailEnv(envs)
    for _ in range(steps):
        env.step_synth(seed, 0, 2, auto_reset=False)
    st = _check_against_restatement(env, envs, (0, 5, 11), DEPTHS, workload)
    assert (st[..., 3] >= 3).any()          # trains on the map
    env.check()
    env.close()


def test_depths_after_replace_env_of_one_replica():
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    bases = [util.load("base_cfg2_L%d" % k) for k in range(1, 8)]
    U = max(len(fx["dm_targets"]) for fx in bases)
    R = max(int((fx["grid"] != 0).sum()) for fx in bases)
    envs = [util.static_of(bases[k], *wl.replica_rng(500 + b)) for b, k in enumerate((0, 0, 1))]   # envs 0 and 1 share one map's tables
    env = BatchedRailEnv(envs, reserve=(U, R))
    for _ in range(20):
        env.step_synth(7, 0, 2)
    _check_against_restatement(env, envs, (0, 1, 2), (8, 30), "before the replacement")
    envs[1] = util.static_of(bases[4], *wl.replica_rng(900))
    env.replace_env(1, envs[1])
    for _ in range(20):
        env.step_synth(7, 0, 2)
    _check_against_restatement(env, envs, (0, 1, 2), (1, 9, 17, 30, 500), "after the replacement")
    env.check()
    env.close()


def test_env_ranges_odd_and_last():
    import torch
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs("cfg1", B=7)
    env = BatchedRailEnv(envs)
    for _ in range(20):
        env.step_synth(seed, 0, 2, auto_reset=False)
    for D in (9, 30):
        full = [x.clone() for x in env.predictions(D, paths=True)]
        f32 = env.predictions(D, torch.int32).clone()
        for rng in (range(1, 4), (3, 6), slice(6, 7), range(0, 7), (5, 7)):
            b0, nb = env._env_range(rng)
            part = env.predictions(D, envs=rng, paths=True)
            assert part[0].shape == (nb, env.A, D + 1, 5)
            for x, y in zip(part, full):
                assert torch.equal(x, y[b0:b0 + nb]), (D, rng)
            assert torch.equal(env.predictions(D, torch.int32, envs=rng), f32[b0:b0 + nb])
    _check_against_restatement(env, envs, range(7), (30,), "cfg1 x 7")
    with pytest.raises(ValueError):
        env.predictions(30, envs=(5, 8))
    with pytest.raises(ValueError):
        env.predictions(30, envs=range(0, 6, 2))
    with pytest.raises(ValueError):
        env.predictions(30, torch.float32)
    with pytest.raises(ValueError):
        env.predictions(501)
    env.check()
    env.close()


def test_1101_one_agent_envs_in_one_launch():
    """more envs than any launch class of the observation kernels; every env its own start, all on the smallest hand-made map"""
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    gs = pc.groups("handmaps")
    g = min(gs, key=lambda x: x["grid"].size)
    A = len(g["slot"])
    statics = []
    for b in range(1101):
        a = b % A
        s = pc.static_of(g)
        for k in ("init_pos", "init_dir", "target", "speed", "earliest", "latest"):
            s[k] = s[k][a:a + 1]
        statics.append(s)
    env = BatchedRailEnv(statics)
    k = len(g["steps"]) - 1
    state = np.stack([g["state"][(b // A) % (k + 1)][b % A:b % A + 1] for b in range(1101)])
    env.set_state(state)
    for D in (9, 30):
        pred, wp, ln = (x.cpu().numpy() for x in env.predictions(D, paths=True))
        p32 = env.predictions(D, torch.int32).cpu().numpy()
        for b in range(1101):
            s = (b // A) % (k + 1)
            util.same(pred[b, 0], g[("pred", D)][s][b % A], "env %d depth %d" % (b, D), dtype=True)
            util.same(p32[b, 0], g[("pred", D)][s][b % A].astype(np.int32), "env %d depth %d int32" % (b, D), dtype=True)
            util.same(wp[b, 0], g[("wp", D)][s][b % A], "env %d waypoints" % b, dtype=True)
            assert ln[b, 0] == g[("len", D)][s][b % A]
    env.check()
    env.close()


@pytest.mark.parametrize("side_stream", (False, True))
def test_guarded_buffers_null_outputs_and_a_side_stream(side_stream):
    """fl_predict through ctypes on buffers with 64 guard elements before and behind the 16-byte aligned output; the outputs start as
    NaN / 0x7f bytes and every element is written; every output NULL in turn"""
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import workload as wl
    envs, seed = wl.make_envs("cfg1", B=3)
    env = hb.BatchedRailEnv(envs)
    for _ in range(15):
        env.step_synth(seed, 0, 2, auto_reset=False)
    env.sync()
    L = hb.lib()
    A, dev = env.A, env.device
    stream = torch.cuda.Stream(device=dev) if side_stream else None
    if side_stream:
        assert L.fl_set_stream(env.h, C.c_void_p(stream.cuda_stream)) == 0
    G = 64
    for D in (1, 8, 17):
        exp = [x.cpu().numpy() for x in hb.BatchedRailEnv.predictions(env, D, paths=True)] if not side_stream else None
        for b0, nb in ((0, 3), (1, 2)):
            n_pred, n_wp, n_len = nb * A * (D + 1) * 5, nb * A * D * 3, nb * A
            for kind, dt in ((0, torch.float64), (1, torch.int32)):
                for skip in (None, "pred", "paths"):
                    pred = torch.full((n_pred + 2 * G,), float("nan") if kind == 0 else 0x7f7f7f7f, dtype=dt, device=dev)
                    wp = torch.full((n_wp + 2 * G,), 0x7f7f7f7f, dtype=torch.int32, device=dev)
                    ln = torch.full((n_len + 2 * G,), 0x7f7f7f7f, dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    ptr = lambda x: C.c_void_p(x.data_ptr() + G * x.element_size())      # noqa: E731  (64 elements: 16-byte aligned)
                    rc = L.fl_predict(env.h, b0, nb, D, kind, None if skip == "pred" else ptr(pred), None if skip == "paths" else ptr(wp),
                                      None if skip == "paths" else ptr(ln))
                    assert rc == 0, L.fl_last_error()
                    assert L.fl_sync(env.h) == 0
                    for x, n, skipped in ((pred, n_pred, skip == "pred"), (wp, n_wp, skip == "paths"), (ln, n_len, skip == "paths")):
                        h = x.cpu().numpy()
                        fill = h[:G]
                        assert (np.isnan(fill).all() if x.dtype == torch.float64 else (fill == 0x7f7f7f7f).all()), "guard before"
                        assert h[:G].tobytes() == h[G + n:].tobytes(), "guard behind"
                        body = h[G:G + n]
                        if skipped:
                            assert body.tobytes() == np.resize(fill, n).tobytes(), "a NULL output was written"
                        elif x.dtype == torch.float64:
                            assert not np.isnan(body).any()
                        else:
                            assert not (body == 0x7f7f7f7f).any()
                    if exp is not None:
                        if skip != "pred":
                            util.same(pred.cpu().numpy()[G:G + n_pred].reshape(nb, A, D + 1, 5), exp[0][b0:b0 + nb].astype(pred.cpu().numpy().dtype), "pred", dtype=True)
                        if skip != "paths":
                            util.same(wp.cpu().numpy()[G:G + n_wp].reshape(nb, A, D, 3), exp[1][b0:b0 + nb], "waypoints", dtype=True)
                            util.same(ln.cpu().numpy()[G:G + n_len].reshape(nb, A), exp[2][b0:b0 + nb], "length", dtype=True)
    if side_stream:
        # the same values as on the handle's usual stream
        st, _ = env.state()
        pred = torch.empty((3, A, 31, 5), dtype=torch.float64, device=dev)
        assert L.fl_predict(env.h, 0, 3, 30, 0, C.c_void_p(pred.data_ptr()), None, None) == 0
        assert L.fl_sync(env.h) == 0
        cache = {}
        for b in range(3):
            util.same(pred[b].cpu().numpy(), _restated(env, envs, st, b, 30, cache)[0], "side stream env %d" % b, dtype=True)
        env.use_torch_stream()
    env.check()
    env.close()


def test_bad_arguments_are_refused_before_a_launch():
    import torch
    from flatland_marl_amd import hip_backend as hb
    fx = util.load("cfg1_sparse")
    env = hb.BatchedRailEnv([util.static_of(fx), util.static_of(fx)])
    L = hb.lib()
    A, D = env.A, 8
    pred = torch.full((2 * A * (D + 1) * 5 + 8,), 7.0, dtype=torch.float64, device=env.device)
    big = torch.full((2 * A * 502 * 5,), 7.0, dtype=torch.float64, device=env.device)
    wp = torch.full((2 * A * 501 * 3,), 7, dtype=torch.int32, device=env.device)
    ln = torch.full((2 * A,), 7, dtype=torch.int32, device=env.device)
    p, pb, w, n = pred.data_ptr(), big.data_ptr(), wp.data_ptr(), ln.data_ptr()
    cases = [(-1, 1, D, 0, p, w, n), (0, 0, D, 0, p, w, n), (1, 2, D, 0, p, w, n), (2, 1, D, 0, p, w, n),       # the range
             (0, 1, 0, 0, pb, w, n), (0, 1, 501, 0, pb, w, n), (0, 1, -3, 0, pb, w, n),                           # the depth
             (0, 1, D, 2, p, w, n), (0, 1, D, -1, p, w, n),                                                       # the element kind
             (0, 2, D, 0, None, None, None),                                                                      # nothing to write
             (0, 1, D, 0, p, w, None), (0, 1, D, 0, p, None, n), (0, 1, D, 0, None, w, None),                     # half a path output
             (0, 1, D, 0, p + 8, w, n), (0, 1, D, 1, p + 4, None, None)]                                          # the alignment
    for b0, nb, depth, kind, *ptrs in cases:
        rc = L.fl_predict(env.h, b0, nb, depth, kind, *[None if q is None else C.c_void_p(q) for q in ptrs])
        assert rc == 1, (b0, nb, depth, kind, rc)          # FL_ERR_ARG
        assert b"fl_predict" in L.fl_last_error()
    torch.cuda.synchronize()
    for x in (pred, big):
        assert bool((x == 7.0).all())
    for x in (wp, ln):
        assert bool((x == 7).all())
    env.check()
    env.close()


def _dicts_equal_fixture(p, g, k, D, A, msg):
    got = p.get()
    assert sorted(got) == list(range(A))
    for h in range(A):
        util.same(got[h], g[("pred", D)][k][h], "%s get() handle %d" % (msg, h), dtype=True)
        n = int(g[("devlen", D)][k][h])
        assert list(p.env.dev_pred_dict[h]) == [tuple(int(q) for q in x) for x in g[("dev", D)][k][h][:n]], (msg, h)
    paths = p.get_shortest_paths(D)
    for h in range(A):
        n = int(g[("len", D)][k][h])
        exp = [((int(r), int(c)), int(d)) for r, c, d in g[("wp", D)][k][h][:n]] if n else None
        assert paths[h] == exp, (msg, h)
        if n:
            assert paths[h][0].position == exp[0][0] and paths[h][0].direction == exp[0][1]


def test_rail_env_facade_on_a_hand_made_map():
    from flatland_marl_amd.rail_env import RailEnv, ShortestPathPredictorForRailEnv, TreeObsUpstream
    g = next(x for x in pc.groups("handmaps") if x["extra"])
    fx = util.load("handmap_" + g["name"])
    p = ShortestPathPredictorForRailEnv(8)
    env = RailEnv.from_static(util.static_of(fx), obs_builder_object=TreeObsUpstream(2, predictor=p))
    env.reset(regenerate_rail=False, regenerate_schedule=False)
    assert p.env is env                                  # (the tree builder's set_env forwards the env)
    A = env.get_num_agents()
    steps = [int(t) for t in g["steps"]]
    for t in range(max(steps) + 1):
        if t:
            env.step({i: int(a) for i, a in enumerate(fx["actions"][t - 1])})
        if t in steps:
            k = steps.index(t)
            util.same(env._batch.state()[0][0], g["state"][k], "%s t=%d state" % (g["name"], t), dtype=True)
            _dicts_equal_fixture(p, g, k, 8, A, "%s t=%d" % (g["name"], t))
            if k == int(g["extra"]["get3_step"]):
                assert sorted(p.get(3)) == g["extra"]["get3"].tolist() == [3]
                assert sorted(p.get(0)) == g["extra"]["get0"].tolist() and sorted(p.get(None)) == g["extra"]["getnone"].tolist()
                util.same(p.get(3)[3], g[("pred", 8)][k][3], "get(3)", dtype=True)
    q = ShortestPathPredictorForRailEnv(30)
    q.set_env(env)
    _dicts_equal_fixture(q, g, steps.index(max(steps)), 30, A, g["name"] + " depth 30")


def test_rail_env_facade_on_an_episode():
    from flatland_marl_amd.rail_env import RailEnv, ShortestPathPredictorForRailEnv
    g = next(x for x in pc.groups("episodes") if x["name"] == "cfg1_malf20_spfollow")
    fx = util.load(g["name"])
    env = RailEnv.from_static(util.static_of(fx))
    env.reset(regenerate_rail=False, regenerate_schedule=False)
    p = ShortestPathPredictorForRailEnv(30)
    p.set_env(env)
    A = env.get_num_agents()
    steps = [int(t) for t in g["steps"]]
    for t, row in enumerate(util.actions_of(fx)[:max(steps)], start=1):
        if t == 1 and 0 in steps:
            _dicts_equal_fixture(p, g, 0, 30, A, g["name"] + " t=0")
        env.step({i: int(a) for i, a in enumerate(row) if a != 255})
        if t in steps:
            _dicts_equal_fixture(p, g, steps.index(t), 30, A, "%s t=%d" % (g["name"], t))


@pytest.mark.parametrize("name", ["cfg2_slow_trains", "cfg0_tall_spfollow"])
def test_plugin_on_a_duck_typed_env(name):
    """the stand-in env object of tests/test_gpu_plugin.py; no reset() of the predictor: the reference's tree builder never calls it"""
    from flatland_marl_amd.plugin import ShortestPathPredictorForRailEnv, TreeObsUpstream
    g = next(x for x in pc.groups("episodes") if x["name"] == name)
    env = util.DuckEnv(util.load(name))
    p = ShortestPathPredictorForRailEnv(10)
    b = TreeObsUpstream(2, p)
    b.set_env(env)
    assert p.env is env
    A = env.get_num_agents()
    for k, t in enumerate(g["steps"]):
        env.goto(int(t))
        _dicts_equal_fixture(p, g, k, 10, A, "%s t=%d" % (name, t))
    assert sorted(p.get(3)) == [3] and sorted(p.get(0)) == list(range(A))
