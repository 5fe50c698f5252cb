"""Cases that drive the step's malfunction draws to the edges of their stream, the env they run on and their reference traces.
A helper module, not a test; numpy and the CPU oracle only.

The env is the one of test_largest_supported_agent_count_matches_oracle: the 30x30 map of cfg2_spfollow, A agents cycling through its
agents' lines, earliest = arange(A) // 4, the MT19937 key of RandomState([seed]) with the position overwritten.

A case is (A, rate, malf_min, malf_max, mt_pos, steps) plus the seed of its key and the condition it exists to reach.  The condition is a
function of the numpy model's per-step log (tests/malf_stream_np.py) and of nothing else; a case that no longer reaches it fails.
"""
import collections
import functools

import numpy as np

from tests import util
from tests.malf_stream_np import MalfStream, rng_of

# why: the condition the case exists to reach, in words (the assertion's message); cond: the same as a predicate on the model's log
Case = collections.namedtuple("Case", "A rate malf_min malf_max mt_pos steps seed why cond")
ACT_SEED = 41          # seed of the synthetic action stream (synth.uniform_actions) of every trace


def _every(log, pred):
    return all(pred(r) for r in log)


def _frac(log, pred):
    return sum(1 for r in log if pred(r)) / float(len(log))


def _total(log, k):
    return sum(int(r[k]) for r in log)


def _ends_at_624(log):          # numpy leaves position 624, not 0, after the last word of a block: the next step starts there
    return any(r["pos0"] == 624 for r in log[1:])


# rate 50: 1 - exp(-50) is 1.0 in double, every agent fires, the last one included
#    A   rate  min    max  pos steps seed
CASES = [
    Case(1, 50.0, 0, 4, 624, 60, 1, "one lane; the first step starts at position 624",
         lambda log: log[0]["starts_at_624"]),
    Case(7, 1.0, 0, 4, 623, 60, 2, "a block boundary between the two words of a rand(), at least 1 twist",
         lambda log: log[0]["pos0"] == 623 and _total(log, "twists") >= 1),
    Case(32, 50.0, 0, 32, 1, 40, 3, "ring of 128 words, span 2^k (acceptance 33/64): wraps in at least 10 % of the steps",
         lambda log: _frac(log, lambda r: r["wraps"]) >= 0.10),
    Case(96, 50.0, 0, 4, 624, 30, 4, "ring of 256 words: wraps in every step; a rejected word is the first of a block",
         lambda log: _every(log, lambda r: r["wraps"]) and _total(log, "rejected_block_start") >= 1),
    Case(96, 0.7, 2, 2, 0, 30, 5, "span 0: no randint word is ever drawn, at least 1000 fires; a step ends exactly at position 624",
         lambda log: _every(log, lambda r: r["extra"] == 0) and _total(log, "fires") >= 1000 and _ends_at_624(log)),
    Case(96, 50.0, 0, 0, 100, 30, 6, "span 0 and every agent fires in every step: all durations are 1",
         lambda log: _every(log, lambda r: r["fires"] == r["A"] and r["min_duration"] == r["max_duration"] == 1 and r["extra"] == 0)),
    Case(96, 50.0, 0, 7, 311, 30, 7, "span 2^k - 1, no rejection: extra equals the number of fires in every step",
         lambda log: _every(log, lambda r: r["extra"] == r["fires"] == r["A"] and r["rejected"] == 0)),
    Case(257, 0.5, 0, 5, 0, 20, 28, "320 lanes; a rejected word is the first of a block",
         lambda log: _total(log, "rejected_block_start") >= 1),
    Case(313, 50.0, 0, 9, 623, 20, 9, "2 * A > 624: at least 2 twists in most steps, wraps in every step",
         lambda log: _frac(log, lambda r: r["twists"] >= 2) > 0.5 and _every(log, lambda r: r["wraps"])),
    Case(313, 0.05, 0, 60000, 624, 40, 10, "the duration cap and a wide mask: a duration above 32768 is drawn",
         lambda log: max(r["max_duration"] for r in log) > 32768),
    Case(480, 50.0, 0, 32, 623, 12, 11, "2 * A + 64 is the ring of 1024 words: wraps and at least 3 twists in every step",
         lambda log: 2 * 480 + 64 == 1024 and _every(log, lambda r: r["wraps"] and r["twists"] >= 3)),
    Case(992, 50.0, 0, 4, 624, 8, 12, "the same with 1024 lanes and a ring of 2048 words: wraps in every step, 6 twists in a step",
         lambda log: 2 * 992 + 64 == 2048 and _every(log, lambda r: r["wraps"] and r["twists"] >= 5) and max(r["twists"] for r in log) == 6),
    Case(992, 0.02, 1, 60000, 620, 12, 13, "sparse fires among 4 blocks: at least 2 twists in every step, the ring never wraps",
         lambda log: _every(log, lambda r: r["twists"] >= 2 and not r["wraps"]) and _total(log, "fires") >= 12),
]
CASE_32, CASE_96_WRAP, CASE_480 = CASES[2], CASES[3], CASES[10]
# the parameter sets of A = 96 that share one map in test_gpu_malf_stream: the four above, one where half of the agents fire and words are
# rejected, and rate 0
CASES_96 = CASES[3:7] + [
    Case(96, 0.7, 0, 4, 622, 30, 14, "some agents fire in every step, the last one among them at least once; the ring wraps",
         lambda log: _every(log, lambda r: 0 < r["fires"] < r["A"]) and _total(log, "fire_last") >= 1 and _total(log, "wraps") >= 1),
    Case(96, 0.0, 0, 4, 624, 30, 15, "rate 0: nothing fires; a step ends exactly at position 624",
         lambda log: _total(log, "fires") == 0 and _ends_at_624(log)),
]


def case_id(c):
    return "A%d-rate%g-dur%d..%d-pos%d" % (c.A, c.rate, c.malf_min, c.malf_max, c.mt_pos)


@functools.lru_cache(maxsize=None)
def _fixture():
    return util.static_of(util.load("cfg2_spfollow"))


def build_env(A, rate, malf_min, malf_max, key, pos, T=None):
    st = _fixture()
    A0 = len(st["init_dir"])
    idx = np.arange(A) % A0
    env = dict(st)
    for k in ("init_pos", "init_dir", "target", "speed", "latest"):
        env[k] = np.ascontiguousarray(np.asarray(st[k])[idx])
    env["earliest"] = (np.arange(A) // 4).astype(np.int32)
    env["malf_rate"], env["malf_min"], env["malf_max"] = float(rate), int(malf_min), int(malf_max)
    env["mt_key"], env["mt_pos"] = np.array(key, dtype=np.uint32), int(pos)
    if T is not None:
        env["T"] = int(T)
    return env


def env_of(case, seed=None, pos=None, T=None):
    key, p = rng_of(case.seed if seed is None else seed, case.mt_pos if pos is None else pos)
    return build_env(case.A, case.rate, case.malf_min, case.malf_max, key, p, T)


Trace = collections.namedtuple("Trace", "env actions state rewards dones done_all okey opos malf nmalf key pos log episodes")


@functools.lru_cache(maxsize=None)
def trace(case, seed=None, pos=None, stream=0, steps=None, T=None, auto_reset=False, inject=()):
    """The oracle and the numpy model stepped side by side with synth.uniform_actions(ACT_SEED, stream, step of the episode); everything
    a test compares afterwards, per step.  inject: ((step, seed, pos), ...) -- both get the key of RandomState([seed]) at position pos
    before that step.  auto_reset: after a step that ends the episode both start fresh agents and the generator runs on.  Computed once
    per argument set and shared; the arrays are read-only."""
    from oracle import orc
    from flatland_marl_amd import synth
    env = env_of(case, seed, pos, T)
    o = orc.OracleEnv(env)
    m = MalfStream(env["mt_key"], env["mt_pos"], case.A, case.rate, case.malf_min, case.malf_max)
    inject = {s: (sd, p) for s, sd, p in inject}
    cols = collections.defaultdict(list)
    tc = episodes = 0
    for t in range(case.steps if steps is None else steps):
        if t in inject:
            key, p = rng_of(*inject[t])
            o.set_rng(key, p)
            m.set_rng(key, p)
        a = synth.uniform_actions(ACT_SEED, stream, tc, case.A)
        r, d, da = o.step(a)
        m.step()
        tc += 1
        ok, op = o.get_rng()
        mk, mp = m.rng()
        for k, v in (("actions", a), ("state", o.state()), ("rewards", r), ("dones", d), ("done_all", da), ("okey", ok), ("opos", op),
                     ("malf", m.malf.copy()), ("nmalf", m.nmalf.copy()), ("key", mk), ("pos", mp)):
            cols[k].append(v)
        if da and auto_reset:
            o = orc.OracleEnv(env)
            o.set_rng(ok, op)
            m.reset()
            tc = 0
            episodes += 1
    arrs = {k: np.stack(v) for k, v in cols.items()}
    for v in arrs.values():
        v.setflags(write=False)
    return Trace(env=env, log=m.log, episodes=episodes, **arrs)


def check_condition(case, log):
    assert case.cond(log), "case %s no longer reaches its condition: %s" % (case_id(case), case.why)
