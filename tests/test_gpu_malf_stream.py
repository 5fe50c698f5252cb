"""GPU parity of the step kernel's malfunction draws (fl_step_body.h: speculative rand() at offset 2 * i, serial replay of the agents that
fire, a ring of wcap tempered words, as many twists as the consumed words need) against numpy itself (tests/malf_stream_np.py) and the
CPU oracle, at the edges of the stream: tests/malf_stream_cases.py lists them, tests/test_malf_stream.py asserts that each case reaches
its edge.  After EVERY step the counters, the counts, the MT19937 key and the position are compared; bit equality, no tolerance."""
import numpy as np
import pytest

from tests import malf_stream_cases as mc
from tests import util
from tests.malf_stream_np import rng_of

pytestmark = pytest.mark.gpu


def _advance(env, traces, t, how):
    """step t of the batch through one of the three entry points of fl_launch_step; env b follows traces[b] (action stream b)"""
    import torch
    if how == "synth":
        return env.step_synth(mc.ACT_SEED, 0, 0, auto_reset=False)
    if how == "synth_auto_reset":
        return env.step_synth(mc.ACT_SEED, 0, 0, auto_reset=True)
    if how == "step":
        return env.step(torch.from_numpy(np.stack([tr.actions[t] for tr in traces])).cuda())
    assert how == "step_obs"
    return env.step_obs(None, mc.ACT_SEED, 0, 0)[:3]


def _compare(env, traces, t, out, what):
    rew, done, done_all = (x.cpu().numpy() for x in out)
    st, _ = env.state()
    info = env.info()["malfunction"].cpu().numpy()
    key, pos = env.rng_state()
    for b, tr in enumerate(traces):
        w = f"{what} env {b} step {t}"
        # against numpy
        util.same(st[b][:, 4], tr.malf[t], w + " malfunction_down_counter vs numpy")
        util.same(st[b][:, 5], tr.nmalf[t], w + " num_malfunctions vs numpy")
        util.same(info[b], tr.malf[t], w + " info['malfunction'] vs numpy")
        assert pos[b] == tr.pos[t], f"{w} mt_pos {pos[b]} vs numpy {tr.pos[t]}"
        util.same(key[b], tr.key[t], w + " mt_key vs numpy")
        # against the oracle
        util.same(st[b], tr.state[t], w + " state vs oracle")
        util.same(rew[b], tr.rewards[t], w + " rewards vs oracle")
        util.same(done[b], tr.dones[t], w + " dones vs oracle")
        assert bool(done_all[b]) == bool(tr.done_all[t]), w + " done_all vs oracle"


def _run(traces, how, what, before_step=None, **kw):
    env = util.batched([tr.env for tr in traces], **kw)
    for t in range(len(traces[0].malf)):
        if before_step is not None:
            before_step(env, t)
        _compare(env, traces, t, _advance(env, traces, t, how), what)
    env.check()
    env.close()


# explicit host-made actions for the rings of 256 and 1024 words, the fused step + observation launch for A = 32, the on-device stream else
HOW = {mc.CASE_96_WRAP: "step", mc.CASE_480: "step", mc.CASE_32: "step_obs"}


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_case_matches_numpy_and_oracle_after_every_step(case):
    how = HOW.get(case, "synth")
    _run([mc.trace(case)], how, f"{mc.case_id(case)} ({how})", pred_depth=60)


@pytest.mark.parametrize("how", ["synth", "step"])
def test_other_entry_points_on_the_smallest_wrapping_ring(how):
    """A = 32 (ring of 128 words, wraps in a quarter of the steps) goes through the fused launch above: here through the other two entry
    points, so that one case has seen all three"""
    _run([mc.trace(mc.CASE_32)], how, how, pred_depth=60)


def test_envs_sharing_one_map_with_different_malfunction_parameters():
    """twelve envs on one map (one set of static tables, FlDev::tab), six parameter sets of A = 96 twice with different keys: thresholds,
    duration ranges and streams are per env"""
    traces = [mc.trace(mc.CASES_96[b % 6], seed=mc.CASES_96[b % 6].seed + 100 * (b // 6), stream=b) for b in range(12)]
    assert len({(tr.env["malf_rate"], tr.env["malf_min"], tr.env["malf_max"]) for tr in traces}) == 6
    assert all(np.array_equal(tr.env["grid"], traces[0].env["grid"]) and np.array_equal(tr.env["target"], traces[0].env["target"])
               for tr in traces)
    _run(traces, "synth", "shared map")


@pytest.mark.parametrize("lo,hi", [(0, 4), (3, 3)])
def test_every_loaded_position_at_the_ends_of_a_block(lo, hi):
    """one key, fourteen envs, mt_pos 0, 1, 2, 621, 622, 623, 624 (each twice): the first words of the step are the last of the loaded
    block, the first of the next, or both"""
    positions = [0, 1, 2, 621, 622, 623, 624] * 2
    traces = [mc.trace(mc.Case(7, 1.0, lo, hi, p, 20, 77, None, None), stream=b) for b, p in enumerate(positions)]
    assert all(np.array_equal(tr.env["mt_key"], traces[0].env["mt_key"]) for tr in traces)
    assert sorted({tr.log[0]["pos0"] for tr in traces}) == sorted(set(positions))
    assert sum(r["fires"] for tr in traces for r in tr.log) > 14 * 20 * 7 // 2          # rate 1.0: 63 % of the draws fire
    _run(traces, "synth", f"mt_pos sweep durations {lo}..{hi}")


def test_rng_state_injected_between_steps():
    """fl_set_rng in the middle of a run of the wrapping A = 96 case: a fresh key at position 624 before step 10, another at position 0
    before step 20; the model and the oracle get the same"""
    inject = ((10, 201, 624), (20, 202, 0))
    tr = mc.trace(mc.CASE_96_WRAP, steps=30, inject=inject)
    assert tr.log[10]["pos0"] == 624 and tr.log[20]["pos0"] == 0 and all(r["wraps"] for r in tr.log)

    def before_step(env, t):
        for s, seed, pos in inject:
            if s == t:
                key, p = rng_of(seed, pos)
                env.set_rng_state(key[None], np.array([p], dtype=np.int32))
    _run([tr], "synth", "set_rng_state", before_step=before_step)


def test_auto_reset_clears_the_counters_and_keeps_the_stream():
    """T = 12, auto-reset: the counters and the counts restart with the episode (durations of up to 33 steps outlive it otherwise), the
    generator runs on"""
    tr = mc.trace(mc.CASE_32, steps=40, T=12, auto_reset=True)
    assert tr.episodes >= 3
    ends = np.flatnonzero(tr.done_all)
    # the reset is visible: counters that were still running at the end of an episode are gone one step later
    assert all(tr.malf[e].max() > 1 for e in ends) and all(tr.nmalf[e + 1].max() == 1 for e in ends if e + 1 < 40)
    _run([tr], "synth_auto_reset", "auto reset")
