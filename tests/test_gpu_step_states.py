"""GPU parity of k_step (fl_step_body.h) with the REAL RailEnv.step() on constructed states: tests/step_state_cases.py lists them,
tests/golden/step_states_<map>.npz holds what the reference did (oracle/refharness/capture_step_states.py), tests/test_step_states.py (CPU)
asserts that they reach the branches they exist for.  The cases are the envs of a batch: the state is injected (fl_set_state) and after
EVERY step the agent rows, the aux columns the fixture determines (previous state, in_malfunction signal, done), rewards, dones, done_all,
the elapsed steps, the MT19937 key and position, check(), the counters of metrics() and scores() and the per-episode pair of info() are
compared; bit equality (the sums of scores(): see _compare).  Three ways: every case of a static variant in one batch on shared tables,
through fl_step and through the fused fl_step_obs (its observations compared with the oracle's); a sample alone with B = 1; one batch that
mixes the two maps on one canvas."""
import numpy as np
import pytest

from tests import handmaps, step_state_cases as sc, util

pytestmark = pytest.mark.gpu
AUX_COLS = [0, 1, 3]      # previous state, in_malfunction signal, done (the deadlock flag belongs to the observation builder)


def _fx_case(fx, name):
    return {k: fx[name + "/" + k] for k in ("state", "aux", "reward", "done", "done_all", "raised", "elapsed", "mt_key_id", "mt_pos", "log")}


_FX = {}


def _fixture(map_name):
    if map_name not in _FX:
        fx = util.load("step_states_" + map_name)
        _FX[map_name] = (fx["mt_keys"], {c["name"]: _fx_case(fx, c["name"]) for c in sc.CASES if c["map"] == map_name})
    return _FX[map_name]


def _run(cases, how, pad=None, obs=False):
    """the cases (same number of steps, same filter flag) as the envs of one batch; how: "step" | "step_obs"; pad: canvas (H, W)"""
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv, EpisodeDoneError
    from oracle import orc
    K, flt = len(cases[0]["actions"]), cases[0]["filter"]
    assert all(len(c["actions"]) == K and c["filter"] == flt for c in cases)
    statics = [sc.static_of(c["map"], c["variant"], c["rng"]) for c in cases]
    if pad is not None:
        statics = [handmaps.padded(s, *pad) for s in statics]
    fxs = [_fixture(c["map"]) for c in cases]
    f = [fxs[b][1][c["name"]] for b, c in enumerate(cases)]
    B, A = len(cases), 5
    env = BatchedRailEnv(statics)
    env.set_state(np.stack([c["state"] for c in cases]), np.stack([c["aux"] for c in cases]),
                  np.array([c["elapsed"] for c in cases], dtype=np.int32), np.array([c["done_all"] for c in cases], dtype=np.uint8))
    st, el = env.state()
    util.same(st, np.stack([c["state"] for c in cases]), "rows read back after the injection")
    util.same(env.state_aux(), np.stack([c["aux"] for c in cases]), "aux read back after the injection")
    oracles = None
    if obs:
        oracles = [orc.OracleEnv(s) for s in statics]
        for o, c in zip(oracles, cases):
            o.set_state(c["state"], c["aux"], c["elapsed"], c["done_all"])
    metrics = np.zeros(4, dtype=np.int64)
    sums = np.zeros(3, dtype=np.float64)
    pair = np.stack([np.array([1.0, 0.0]) for _ in cases])      # (no finished episode: sum of rewards 0, nobody arrived)
    for k in range(K):
        acts = torch.from_numpy(np.stack([c["actions"][k] for c in cases])).cuda()
        if how == "step":
            out = env.step(acts, filter_required=flt)
        else:
            out = env.step_obs(acts, filter_required=flt)
        rew, done, done_all = (x.cpu().numpy() for x in out[:3])
        st, el = env.state()
        aux = env.state_aux()
        key, pos = env.rng_state()
        for b, c in enumerate(cases):
            w = "%s (%s, env %d of %d) step %d" % (c["name"], how, b, B, k)
            util.same(st[b], f[b]["state"][k], w + " rows")
            util.same(aux[b][:, AUX_COLS], f[b]["aux"][k][:, AUX_COLS], w + " aux")
            util.same(rew[b], f[b]["reward"][k], w + " rewards")
            # (a step on a finished env: the reference raises and leaves its dones, all set by the ending step, as they are)
            util.same(done[b], f[b]["done"][k], w + " dones")
            assert bool(done_all[b]) == bool(f[b]["done_all"][k]), w + " done_all"
            assert el[b] == f[b]["elapsed"][k], w + " elapsed %d vs %d" % (el[b], f[b]["elapsed"][k])
            assert pos[b] == f[b]["mt_pos"][k], w + " mt_pos %d vs %d" % (pos[b], f[b]["mt_pos"][k])
            util.same(key[b], fxs[b][0][f[b]["mt_key_id"][k]], w + " mt_key")
            if not f[b]["raised"][k]:
                metrics[2] += A
                if f[b]["done_all"][k]:
                    R, arrived, T = int(f[b]["reward"][k].sum()), int((f[b]["state"][k][:, 3] == sc.DONE).sum()), int(statics[b]["T"])
                    metrics += (R, arrived, 0, 1)
                    pair[b] = (1.0 + float(R) / (float(T) * float(A)), float(arrived) / float(A))
                    sums += (pair[b][0], pair[b][1], 1.0)
        raising = [b for b in range(B) if f[b]["raised"][k]]
        if raising:
            with pytest.raises(EpisodeDoneError, match="env %d: Episode is done" % raising[0]):
                env.check()
        else:
            env.check()
        util.same(env.metrics().cpu().numpy(), metrics, "%s step %d metrics()" % (how, k))
        util.same(env.info()["scores"].cpu().numpy(), pair, "%s step %d the per-episode pair" % (how, k))
        # scores() adds the envs' terms up in an order of its own: at most B additions of values in [-|R|, 1] per sum, each within
        # half an ulp of the running sum -- B * 2^-53 relative to the sum of the magnitudes; the episode count is exact
        got = env.scores().cpu().numpy()
        assert got[2] == sums[2], "%s step %d scores() episodes" % (how, k)
        tol = B * 2.0 ** -53 * max(1.0, float(np.abs(pair).sum()))
        assert np.all(np.abs(got[:2] - sums[:2]) <= tol), "%s step %d scores() %s vs %s" % (how, k, got, sums)
        if obs:
            o_gpu = out[3]
            forest, attr, adj = (o_gpu[n].cpu().numpy() for n in ("forest", "agent_attr", "adjacency"))
            for b, (o, c) in enumerate(zip(oracles, cases)):
                a = c["actions"][k].copy()
                a[f[b]["log"][k][:, 12] == 1] = sc.ABSENT
                try:
                    o.step(a)
                except RuntimeError:
                    assert f[b]["raised"][k]
                exp = o.obs_cutils(31, 500)
                w = "%s (step_obs) step %d" % (c["name"], k)
                util.same(forest[b], exp["forest"], w + " forest vs oracle")
                util.same(attr[b], exp["attr"], w + " agent_attr vs oracle")
                util.same(adj[b], exp["adjacency"], w + " adjacency vs oracle")
    env.close()


def _groups():
    """(map, variant, filter) -> the cases, each group split by the number of steps (a batch steps in lock-step)"""
    g = {}
    for c in sc.CASES:
        g.setdefault((c["map"], c["variant"], c["filter"]), {}).setdefault(len(c["actions"]), []).append(c)
    return g


GROUPS = _groups()


def test_no_case_is_left_out():
    assert sorted(c["name"] for by_k in GROUPS.values() for cs in by_k.values() for c in cs) == sorted(c["name"] for c in sc.CASES)
    assert len(sc.CASES) >= 150


@pytest.mark.parametrize("how", ["step", "step_obs"])
@pytest.mark.parametrize("group", sorted(GROUPS), ids=lambda g: "%s-%s%s" % (g[0], g[1], "-filter" if g[2] else ""))
def test_every_case_of_a_variant_in_one_batch(group, how):
    for k, cases in sorted(GROUPS[group].items()):
        _run(cases, how, obs=(how == "step_obs"))


def test_a_sample_of_cases_alone():
    """B = 1: every seventh case, and the cases of the rows the recorded episodes never reach"""
    names = {c["name"] for c in sc.CASES[::7]} | {"malfoff_complete_stop", "malfoff_stop_on_occupied", "draw_malfoff_stop", "last_arrives", "T_end_mixed",
                                                    "already_over", "filter_required"}
    for c in sc.CASES:
        if c["name"] in names:
            _run([c], "step")


def test_two_maps_in_one_batch_on_one_canvas():
    """the yard and the crossing padded onto 12 x 12, their two-step cases interleaved: a case's neighbours are of the other map"""
    two = [c for c in sc.CASES if len(c["actions"]) == 2 and not c["filter"]]
    yard, crossing = [c for c in two if c["map"] == "yard"], [c for c in two if c["map"] == "crossing"]
    n = min(len(yard), len(crossing))
    assert n >= 20
    step = len(yard) // n
    mixed = [c for pair in zip(yard[::step][:n], crossing[:n]) for c in pair]
    assert {c["map"] for c in mixed[0::2]} == {"yard"} and {c["map"] for c in mixed[1::2]} == {"crossing"}
    _run(mixed, "step", pad=(12, 12))
