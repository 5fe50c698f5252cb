"""GPU: the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py through every layer -- fl_action_space and
fl_decision_cells (flatland_marl_amd/csrc/fl_wrappers.h), BatchedRailEnv / MixedBatch, and the wrappers of rail_env over this library's
RailEnv -- against the reference's own outputs (tests/golden/action_space_*.npz).  Everything is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import action_space_np as an
from tests import handmaps, util

pytestmark = pytest.mark.gpu

I32_INF = np.iinfo(np.int32).max


def _as_i32(dist):
    return np.where(np.isinf(dist), I32_INF, dist).astype(np.int32)


def _by_shape(groups):
    shapes = {}
    for g in groups:
        shapes.setdefault(g["grid"].shape + (len(g["slot"]),), []).append(g)
    return shapes


def _poison(env):
    """every cached output buffer of the batch: NaN / 0xFF, so that an element the next call leaves out shows"""
    for t in env._wrap.values():
        t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0x7FFFFFFF if t.element_size() == 4 else 0xFF)


def _check_state(env, gs, s, pick=None, envs=None, cells=True):
    """env b of the batch (or of the range `envs`) holds group gs[b] at its recorded state s: the four outputs in both element kinds,
    and the cells"""
    import torch
    pick = pick or (lambda r, b: r[b])
    for dtype in (torch.float64, torch.int32):
        _poison(env)
        act, dist, cnt = (x.cpu().numpy() for x in env.shortest_path_actions(dtype, envs))
        for b, g in enumerate(gs):
            k = min(s, len(g["steps"]) - 1)
            msg = "%s state %d %s" % (g["name"], k, dtype)
            util.same(pick(act, b), g["sp_action"][k], msg + " actions", dtype=True, bytes=True)
            util.same(pick(dist, b), g["sp_dist"][k] if dtype == torch.float64 else _as_i32(g["sp_dist"][k]), msg + " distances", dtype=True, bytes=True)
            util.same(pick(cnt, b), g["sp_count"][k], msg + " count", dtype=True, bytes=True)
    _poison(env)
    dec = env.on_decision_cell(envs).cpu().numpy()
    for b, g in enumerate(gs):
        util.same(pick(dec, b), g["on_decision"][min(s, len(g["steps"]) - 1)], g["name"] + " on_decision", dtype=True, bytes=True)
    if cells:
        _poison(env)
        cl = env.decision_cells(envs).cpu().numpy()
        for b, g in enumerate(gs):
            H, W = g["cells"].shape
            got = pick(cl, b)
            util.same(got[:H, :W], g["cells"], g["name"] + " cells", dtype=True, bytes=True)
            assert not got[H:].any() and not got[:, W:].any()


def _check_groups(env, gs):
    for s in range(max(len(g["steps"]) for g in gs)):
        env.set_state(np.stack([g["state"][min(s, len(g["steps"]) - 1)] for g in gs]))
        _check_state(env, gs, s, cells=s == 0)
    env.check()


@pytest.mark.parametrize("source", an.SOURCES)
def test_fixtures_batched_per_shape(source):
    """the groups of one shape (A = 4, 5, 8, 24, the episodes' own; the tall map) are the envs of one handle: states through fl_set_state"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    for shape, gs in _by_shape(an.groups(source)).items():
        env = BatchedRailEnv([an.static_of(g) for g in gs])
        _check_groups(env, gs)
        env.close()


@pytest.mark.parametrize("name", ("mesh12", "disconnected"))
def test_one_env_of_one_agent(name):
    """B = 1, A = 1: every agent of a hand-made map alone on it"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    g = next(x for x in an.groups("handmaps") if x["name"] == name)
    for a in range(len(g["slot"])):
        one = dict(g, **{k: g[k][:, a:a + 1] for k in an.KINDS + ("state",)})
        one["slot"] = g["slot"][a:a + 1]
        env = BatchedRailEnv([an.static_of(g, [a])])
        assert (env.B, env.A) == (1, 1)
        _check_groups(env, [one])
        env.close()


def _small_padded():
    """oval, lasso and disconnected (five agents each) on one 8 x 10 canvas"""
    gs = {g["name"]: g for g in an.groups("handmaps")}
    return {n: gs[n] for n in ("oval", "lasso", "disconnected")}, 8, 10


def test_padded_maps_shared_tables_and_ranges():
    """two and more maps padded onto one canvas; replicas that read one table set (tab[b] != b) beside envs with tables of their own;
    ranges with b0 > 0 and nb < B at both ends of the batch"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    maps, H, W = _small_padded()
    order = ("oval", "oval", "lasso", "oval", "disconnected", "lasso", "oval")
    gs = [maps[n] for n in order]
    env = BatchedRailEnv([handmaps.padded(an.static_of(g), H, W) for g in gs])
    B = len(gs)
    for s in (0, 3, 9, 17):
        # (replicas of one map in different states of its episode)
        rows = [g["state"][min(s + 2 * b, len(g["steps"]) - 1)] for b, g in enumerate(gs)]
        env.set_state(np.stack(rows))
        shifted = [dict(g, **{k: g[k][min(s + 2 * b, len(g["steps"]) - 1)][None] for k in an.KINDS}) for b, g in enumerate(gs)]
        for b0, b1 in ((0, B), (0, 1), (1, 3), (2, B - 1), (B - 2, B), (B - 1, B)):
            _check_state(env, shifted[b0:b1], 0, envs=(b0, b1))
        _check_state(env, shifted[3:6], 0, envs=range(3, 6))
        _check_state(env, shifted[1:4], 0, envs=slice(1, 4))
    env.check()
    env.close()


def test_replace_env_with_another_map():
    """decision_cells and on_decision_cell follow a live replace_env: the owner of a shared table set is replaced (its replica becomes
    the owner), then the replica too"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    maps, H, W = _small_padded()
    st = lambda n: handmaps.padded(an.static_of(maps[n]), H, W)      # noqa: E731
    names = ["lasso", "lasso", "oval"]
    env = BatchedRailEnv([st(n) for n in names], reserve=(5, 40))
    for b, n in ((0, "disconnected"), (1, "oval"), (2, "lasso"), (0, "lasso")):
        gs = [maps[x] for x in names]
        s = min(len(g["steps"]) for g in gs) - 1
        env.set_state(np.stack([g["state"][s] for g in gs]))
        _check_state(env, gs, s)
        env.replace_env(b, st(n))
        names[b] = n
    gs = [maps[x] for x in names]
    env.set_state(np.stack([g["state"][5] for g in gs]))
    _check_state(env, gs, 5)
    env.rebuild_distance_maps()
    import torch
    env.rebuild_distance_maps(torch.tensor([1, 0, 1], dtype=torch.uint8, device=env.device))
    _check_state(env, gs, 5)
    env.check()
    env.close()


def test_handmaps_in_one_mixed_batch():
    import torch
    from flatland_marl_amd.hip_backend import MixedBatch
    gs = an.groups("handmaps")
    mb = MixedBatch([an.static_of(g) for g in gs])
    assert len(mb.groups) > 1
    rng = np.random.RandomState(3)
    for s in (0, 4, 11):
        per = [[] for _ in mb.groups]
        for i, g in enumerate(gs):
            per[mb.where[i][0]].append(g["state"][min(s, len(g["steps"]) - 1)])
        for grp, rows in zip(mb.groups, per):
            grp.set_state(np.stack(rows))
        out, o32, dec, cells = mb.shortest_path_actions(), mb.shortest_path_actions(torch.int32), mb.on_decision_cell(), mb.decision_cells()
        reduced = [rng.randint(0, 4, len(g["slot"])).astype(np.uint8) for g in gs]
        tr = mb.reduced_actions(reduced)
        assert len(out) == len(mb.groups)
        for i, g in enumerate(gs):
            k = min(s, len(g["steps"]) - 1)
            act, dist, cnt = (x.cpu().numpy() for x in mb.pick(i, out))
            util.same(act, g["sp_action"][k], "mixed %s actions" % g["name"], dtype=True, bytes=True)
            util.same(dist, g["sp_dist"][k], "mixed %s distances" % g["name"], dtype=True, bytes=True)
            util.same(cnt, g["sp_count"][k], "mixed %s count" % g["name"], dtype=True, bytes=True)
            util.same(mb.pick(i, o32)[1].cpu().numpy(), _as_i32(g["sp_dist"][k]), "mixed %s int32" % g["name"], dtype=True, bytes=True)
            util.same(mb.pick(i, dec).cpu().numpy(), g["on_decision"][k], "mixed %s on_decision" % g["name"], dtype=True, bytes=True)
            util.same(mb.pick(i, cells).cpu().numpy(), g["cells"], "mixed %s cells" % g["name"], dtype=True, bytes=True)
            util.same(mb.pick(i, tr).cpu().numpy(), an.translate(reduced[i], g["sp_action"][k], g["sp_count"][k]), "mixed %s translation" % g["name"], dtype=True, bytes=True)
    mb.check()
    mb.close()


@pytest.mark.parametrize("source", ("handmaps", "states_yard_crowd", "episodes"))
def test_reduced_actions_against_the_recorded_lists(source):
    """every value 0 .. 3 and 255 against every count (2 and 3: mesh12 has the lists of three), and a mixed row"""
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    rng = np.random.RandomState(11)
    counts = set()
    for shape, gs in _by_shape(an.groups(source)).items():
        env = BatchedRailEnv([an.static_of(g) for g in gs])
        B, A = env.B, env.A
        for s in range(0, max(len(g["steps"]) for g in gs), 3):
            ks = [min(s, len(g["steps"]) - 1) for g in gs]
            env.set_state(np.stack([g["state"][k] for g, k in zip(gs, ks)]))
            act = np.stack([g["sp_action"][k] for g, k in zip(gs, ks)])
            cnt = np.stack([g["sp_count"][k] for g, k in zip(gs, ks)])
            counts |= set(cnt.ravel().tolist())
            rows = [np.full((B, A), v, dtype=np.uint8) for v in (0, 1, 2, 3, 255)]
            rows.append(rng.choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), size=(B, A)))
            for n, red in enumerate(rows):
                arg = red if n % 2 else torch.as_tensor(red).to(env.device)      # (a host array and a device tensor)
                _poison(env)
                util.same(env.reduced_actions(arg).cpu().numpy(), an.translate(red, act, cnt), "%s state %d row %d" % (source, s, n), dtype=True, bytes=True)
            if B > 1:
                util.same(env.reduced_actions(rows[-1][1:], envs=(1, B)).cpu().numpy(), an.translate(rows[-1][1:], act[1:], cnt[1:]), "a range", dtype=True, bytes=True)
        for bad in (np.zeros((B, A + 1), dtype=np.uint8), np.zeros((B, A), dtype=np.float32), np.full((B, A), 256),
                    torch.zeros((B, A), dtype=torch.int32, device=env.device), torch.zeros((B, A + 1), dtype=torch.uint8, device=env.device)):
            with pytest.raises(ValueError):
                env.reduced_actions(bad)
        with pytest.raises(ValueError):
            env.shortest_path_actions(torch.float32)
        with pytest.raises(ValueError):
            env.on_decision_cell(envs=(0, B + 1))
        env.check()
        env.close()
    assert counts == ({2, 3} if source == "handmaps" else {2})


def test_step_shortest_path_equals_translate_then_step():
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import workload as wl
    envs, _ = wl.make_envs("cfg1", B=3)
    one, two = hb.BatchedRailEnv(envs), hb.BatchedRailEnv(envs)
    rng = np.random.RandomState(5)
    for t in range(40):
        red = rng.choice(np.array([0, 1, 1, 1, 2, 255], dtype=np.uint8), size=(one.B, one.A))
        r1, d1, a1 = one.step_shortest_path(red, filter_required=bool(t % 2))
        r2, d2, a2 = two.step(two.reduced_actions(red), filter_required=bool(t % 2))
        util.same(one.state()[0], two.state()[0], "state after step %d" % (t + 1), dtype=True, bytes=True)
        util.same(r1.cpu().numpy(), r2.cpu().numpy(), "rewards", dtype=True, bytes=True)
        util.same(d1.cpu().numpy(), d2.cpu().numpy(), "dones", dtype=True, bytes=True)
    st = one.state()[0]
    assert (st[:, :, 3] >= an.MOVING).any(), "no agent ever left"
    for e in (one, two):
        e.check()
        e.close()


def test_guarded_buffers_and_null_outputs():
    """fl_action_space and fl_decision_cells through ctypes on buffers with guard words before and behind every output; the outputs
    start as NaN / 0xFF bytes and every element is written; the optional outputs NULL in turn"""
    import torch
    from flatland_marl_amd import hip_backend as hb
    maps, H, W = _small_padded()
    gs = [maps["oval"], maps["lasso"], maps["oval"]]
    env = hb.BatchedRailEnv([handmaps.padded(an.static_of(g), H, W) for g in gs])
    s = 6
    env.set_state(np.stack([g["state"][s] for g in gs]))
    L, A, dev, G = hb.lib(), env.A, env.device, 16

    def buf(n, dt):
        fill = float("nan") if dt == torch.float64 else 0x7F7F7F7F if dt == torch.int32 else 0xFF
        return torch.full((n + 2 * G,), fill, dtype=dt, device=dev)

    def inner(x, n):
        h = x.cpu().numpy()
        assert h[:G].tobytes() == h[G + n:].tobytes() == np.resize(h[:1], G).tobytes(), "a guard word was written"
        return h[G:G + n], h[:1]

    ptr = lambda x: C.c_void_p(x.data_ptr() + G * x.element_size())      # noqa: E731  (16 elements: 8-byte aligned at the least)
    for b0, nb in ((0, 3), (1, 2), (2, 1)):
        red = np.full((nb, A), 2, dtype=np.uint8)
        red_dev = torch.as_tensor(red).to(dev)
        exp = {k: np.stack([g[k][s] for g in gs[b0:b0 + nb]]) for k in an.KINDS}
        for kind, dt in ((0, torch.float64), (1, torch.int32)):
            for skip in (None, "lists", "dec", "actions"):
                act, dist, cnt, dec, out = buf(nb * A * 3, torch.uint8), buf(nb * A * 3, dt), buf(nb * A, torch.uint8), buf(nb * A, torch.uint8), \
                    buf(nb * A, torch.uint8)
                torch.cuda.synchronize()
                lists = [None] * 3 if skip == "lists" else [ptr(act), ptr(dist), ptr(cnt)]
                rc = L.fl_action_space(env.h, b0, nb, kind, *lists, None if skip == "dec" else ptr(dec),
                                       None if skip == "actions" else C.c_void_p(red_dev.data_ptr()), None if skip == "actions" else ptr(out))
                assert rc == 0, L.fl_last_error()
                assert L.fl_sync(env.h) == 0
                want = {"act": exp["sp_action"].ravel(), "dist": (exp["sp_dist"] if kind == 0 else _as_i32(exp["sp_dist"])).ravel(),
                        "cnt": exp["sp_count"].ravel(), "dec": exp["on_decision"].ravel(),
                        "out": an.translate(red, exp["sp_action"], exp["sp_count"]).ravel()}
                for name, x, skipped in (("act", act, skip == "lists"), ("dist", dist, skip == "lists"), ("cnt", cnt, skip == "lists"),
                                         ("dec", dec, skip == "dec"), ("out", out, skip == "actions")):
                    body, fill = inner(x, len(want[name]))
                    if skipped:
                        assert body.tobytes() == np.resize(fill, len(body)).tobytes(), "a NULL output was written"
                    else:
                        util.same(body, want[name], "%s range (%d, %d) kind %d" % (name, b0, nb, kind), dtype=True, bytes=True)
        cells = buf(nb * H * W, torch.uint8)
        assert L.fl_decision_cells(env.h, b0, nb, ptr(cells)) == 0, L.fl_last_error()
        assert L.fl_sync(env.h) == 0
        body, _ = inner(cells, nb * H * W)
        for b, g in enumerate(gs[b0:b0 + nb]):
            h, w = g["cells"].shape
            util.same(body.reshape(nb, H, W)[b][:h, :w], g["cells"], "cells", dtype=True, bytes=True)
    env.check()
    env.close()


def test_bad_arguments_are_refused_before_a_launch():
    import torch
    from flatland_marl_amd import hip_backend as hb
    fx = util.load("cfg1_sparse")
    env = hb.BatchedRailEnv([util.static_of(fx), util.static_of(fx)])
    L = hb.lib()
    A = env.A
    u8 = lambda n: torch.full((n,), 7, dtype=torch.uint8, device=env.device)      # noqa: E731
    act, cnt, dec, red, out, cells = u8(2 * A * 3), u8(2 * A), u8(2 * A), u8(2 * A), u8(2 * A), u8(2 * env.H * env.W)
    dist = torch.full((2 * A * 3 + 2,), 7.0, dtype=torch.float64, device=env.device)
    a, d, c, e, r, o = (x.data_ptr() for x in (act, dist, cnt, dec, red, out))
    cases = [(-1, 1, 0, a, d, c, e, r, o), (0, 0, 0, a, d, c, e, r, o), (1, 2, 0, a, d, c, e, r, o), (2, 1, 0, a, d, c, e, r, o),     # the range
             (0, 1, 2, a, d, c, e, r, o), (0, 1, -1, a, d, c, e, r, o),                                                              # the element kind
             (0, 2, 0, None, None, None, None, None, None),                                                                          # nothing to write
             (0, 1, 0, a, d, None, e, r, o), (0, 1, 0, a, None, c, e, r, o), (0, 1, 0, None, d, c, e, r, o),                         # part of a list
             (0, 1, 0, a, None, None, e, None, None), (0, 1, 0, None, None, c, None, None, None),
             (0, 1, 0, a, d, c, e, r, None), (0, 1, 0, a, d, c, e, None, o), (0, 1, 0, None, None, None, None, r, None),             # half a translation
             (0, 1, 0, a, d + 4, c, e, r, o), (0, 1, 1, a, d + 2, c, e, r, o)]                                                       # the alignment
    for b0, nb, kind, *ptrs in cases:
        rc = L.fl_action_space(env.h, b0, nb, kind, *[None if q is None else C.c_void_p(q) for q in ptrs])
        assert rc == 1, (b0, nb, kind, ptrs, rc)          # FL_ERR_ARG
        assert b"fl_action_space" in L.fl_last_error()
    for b0, nb, p in ((-1, 1, cells.data_ptr()), (0, 0, cells.data_ptr()), (1, 2, cells.data_ptr()), (2, 1, cells.data_ptr()), (0, 2, None)):
        assert L.fl_decision_cells(env.h, b0, nb, None if p is None else C.c_void_p(p)) == 1
        assert b"fl_decision_cells" in L.fl_last_error()
    h = C.c_void_p()
    assert L.fl_create(1, A, env.H, env.W, 0, C.byref(h)) == 0      # an uncommitted handle
    assert L.fl_action_space(h, 0, 1, 0, *[C.c_void_p(q) for q in (a, d, c, e, r, o)]) == 1
    assert L.fl_decision_cells(h, 0, 1, C.c_void_p(cells.data_ptr())) == 1
    L.fl_destroy(h)
    torch.cuda.synchronize()
    for x in (act, cnt, dec, red, out, cells):
        assert bool((x == 7).all())
    assert bool((dist == 7.0).all())
    env.check()
    env.close()


# ---- the dict level
def test_functions_on_rail_env_replaying_a_hand_made_map():
    """possible_actions_sorted_by_distance (types included: RailEnvActions, numpy float64, the int 0 of the fallback) and
    find_all_cells_where_agent_can_choose (as sets) on this library's RailEnv, also through a wrapper"""
    from flatland_marl_amd import rail_env as re_
    for name in ("mesh12", "crossing_u1"):
        g = next(x for x in an.groups("handmaps") if x["name"] == name)
        fx = util.load("handmap_" + name)
        env = re_.RailEnv.from_static(util.static_of(fx), obs_builder_object=re_.GlobalObsForRailEnv())
        env.reset(regenerate_rail=False, regenerate_schedule=False)
        top = re_.SkipNoChoiceCellsWrapper(re_.ShortestPathActionWrapper(env), False, 1.0)
        sw, nb, dc = re_.find_all_cells_where_agent_can_choose(top)
        exp_sw = {(int(r), int(c)) for r, c in zip(*np.nonzero(g["cells"] & 1))}
        exp_nb = {(int(r), int(c)) for r, c in zip(*np.nonzero(g["cells"] & 2))}
        assert (sw, nb, dc) == (exp_sw, exp_nb, exp_sw | exp_nb) and isinstance(sw, set) and isinstance(dc, set)
        assert (top.switches, top.switches_neighbors, top.decision_cells) == (sw, nb, dc)
        steps = [int(t) for t in g["steps"]]
        fallback = 0
        for t in range(max(steps) + 1):
            if t:
                env.step({i: int(a) for i, a in enumerate(fx["actions"][t - 1])})
            if t not in steps[::4] + steps[-1:]:
                continue
            k = steps.index(t)
            util.same(env._batch.state()[0][0], g["state"][k], "%s t=%d state" % (name, t), dtype=True, bytes=True)
            for h, agent in enumerate(env.agents):
                got = re_.possible_actions_sorted_by_distance(top if h % 2 else env, h)
                n = int(g["sp_count"][k][h])
                assert isinstance(got, list) and len(got) == n and all(isinstance(x, tuple) and len(x) == 2 for x in got)
                assert [int(a) for a, _ in got] == g["sp_action"][k][h][:n].tolist() and all(type(a) is re_.RailEnvActions for a, _ in got)
                if int(g["state"][k][h][3]) in (an.WAITING, an.MALF_OFF, an.DONE):
                    assert all(type(dd) is int and dd == 0 for _, dd in got)
                    fallback += 1
                else:
                    assert all(type(dd) is np.float64 for _, dd in got)
                    assert np.array([dd for _, dd in got]).tobytes() == g["sp_dist"][k][h][:n].tobytes()
                assert top.on_decision_cell(agent) == bool(g["on_decision"][k][h])
                assert top.on_switch(agent) == (agent.position in exp_sw) and top.next_to_switch(agent) == (agent.position in exp_nb)
        assert fallback
        env._batch.close()


@pytest.mark.parametrize("name", sorted(an.WRAPPED))
def test_wrappers_reproduce_the_wrapped_episode(name):
    """SkipNoChoiceCellsWrapper(ShortestPathActionWrapper(env), True, 0.9) over rail_env.RailEnv on the recorded env and reduced-action
    stream: keys, rewards as the same floats, dones, infos, the agents' state and the inner-step counts of every outer step"""
    from flatland_marl_amd import rail_env as re_
    w = an.wrapped_episode(name)
    env = re_.RailEnv.from_static(util.static_of(util.load(an.WRAPPED_STATICS[name])), obs_builder_object=re_.GlobalObsForRailEnv())
    env.reset(regenerate_rail=False, regenerate_schedule=False)
    calls = [0]
    inner_step = env.step

    def counted(action_dict):
        calls[0] += 1
        return inner_step(action_dict)

    env.step = counted
    top = re_.SkipNoChoiceCellsWrapper(re_.ShortestPathActionWrapper(env), True, an.WRAPPED_DISCOUNT)
    assert top.accumulate_skipped_rewards is True and top.discounting == an.WRAPPED_DISCOUNT and top.skipped_rewards == {}
    A = env.get_num_agents()
    for s, row in enumerate(w["reduced"]):
        calls[0] = 0
        o, r, d, i = top.step({h: int(row[h]) for h in range(A)})
        keys = [h for h in range(A) if w["present"][s][h]]
        msg = "outer step %d" % s
        assert sorted(o) == sorted(r) == keys and sorted(k for k in d if k != "__all__") == keys, msg
        assert sorted(i) == ["action_required", "malfunction", "speed", "state"] and all(sorted(i[k]) == keys for k in i), msg
        assert calls[0] == int(w["inner"][s]), msg
        assert np.array([r[h] for h in keys], dtype=np.float64).tobytes() == w["reward"][s][keys].tobytes(), msg
        assert [bool(d[h]) for h in keys] == [bool(v) for v in w["done"][s][keys]] and bool(d["__all__"]) == bool(w["done_all"][s]), msg
        assert [bool(i["action_required"][h]) for h in keys] == [bool(v) for v in w["action_required"][s][keys]], msg
        assert [int(i["malfunction"][h]) for h in keys] == w["malfunction"][s][keys].tolist(), msg
        assert np.array([i["speed"][h] for h in keys], dtype=np.float64).tobytes() == w["speed"][s][keys].tobytes(), msg
        assert [int(i["state"][h]) for h in keys] == w["info_state"][s][keys].tolist(), msg
        util.same(env._batch.state()[0][0], w["state"][s], msg + " state", dtype=True, bytes=True)
    if w["done_all"][-1]:
        with pytest.raises(Exception, match="Episode is done"):
            top.step({0: 1})
    obs, info = top.reset(regenerate_rail=False, regenerate_schedule=False)
    assert sorted(obs) == list(range(A)) and top.decision_cells == top.switches | top.switches_neighbors
    env._batch.close()
