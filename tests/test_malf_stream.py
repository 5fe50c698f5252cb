"""The C oracle's malfunction draws against numpy itself (tests/malf_stream_np.py) where the stream is hard: many fires a step, long
rejection runs, several MT19937 blocks a step, positions at the ends of a block.  Bit equality throughout.  The same cases then run on
the HIP step kernel in tests/test_gpu_malf_stream.py; the conditions that make them hard are asserted here, from the numpy model alone."""
import numpy as np
import pytest

from tests import malf_stream_cases as mc
from tests.malf_stream_np import MalfStream, random_state, rng_of, wcap_of


def _same_trace(tr, what):
    for t in range(len(tr.malf)):
        np.testing.assert_array_equal(tr.state[t][:, 4], tr.malf[t], err_msg=f"{what} step {t} malfunction_down_counter")
        np.testing.assert_array_equal(tr.state[t][:, 5], tr.nmalf[t], err_msg=f"{what} step {t} num_malfunctions")
        assert tr.opos[t] == tr.pos[t], f"{what} step {t} mt_pos {tr.opos[t]} vs numpy {tr.pos[t]}"
        np.testing.assert_array_equal(tr.okey[t], tr.key[t], err_msg=f"{what} step {t} mt_key")


@pytest.mark.parametrize("case", mc.CASES + mc.CASES_96[4:], ids=mc.case_id)
def test_oracle_malfunctions_match_numpy_and_case_reaches_its_condition(case):
    tr = mc.trace(case)
    assert len(tr.log) == case.steps
    _same_trace(tr, mc.case_id(case))
    mc.check_condition(case, tr.log)


def test_ring_size_of_the_cases_is_what_their_purpose_says():
    assert [wcap_of(A) for A in (1, 7, 32, 96, 257, 313, 480, 992)] == [128, 128, 128, 256, 1024, 1024, 1024, 2048]
    assert 2 * 480 + 64 == wcap_of(480) and 2 * 992 + 64 == wcap_of(992)


@pytest.mark.parametrize("span", [0, 1, 2, 3, 4, 255, 256, 59999])
def test_oracle_randint_matches_numpy(span):
    """One agent, rate 50 (it fires in every step), orc_reset() after every step so that the counter takes every draw: the duration the
    oracle shows is rs.randint(lo, lo + span + 1) + 1 - 1, and its generator stands where numpy's does."""
    from oracle import orc
    lo = 3
    case = mc.Case(1, 50.0, lo, lo + span, 617, 300, 100 + span, None, None)
    env = mc.env_of(case)
    o = orc.OracleEnv(env)
    rs = random_state(env["mt_key"], env["mt_pos"])
    act = np.zeros(1, dtype=np.uint8)
    for t in range(case.steps):
        o.step(act)
        assert rs.rand() < 1.0
        n = int(rs.randint(lo, lo + span + 1)) + 1
        assert o.state()[0, 4] == n - 1, f"span {span} step {t}"
        key, pos = o.get_rng()
        st = rs.get_state()
        assert pos == st[2], f"span {span} step {t} mt_pos"
        np.testing.assert_array_equal(key, st[1], err_msg=f"span {span} step {t} mt_key")
        o.reset()


def test_model_counts_words_and_twists():
    """the model's own bookkeeping on a stream small enough to follow by hand: rate 50, span 0 -> exactly two words an agent"""
    key, pos = rng_of(9, 620)
    m = MalfStream(key, pos, 5, 50.0, 7, 7)
    r = m.step()                                   # words 620 .. 629: one twist, position 6 afterwards
    assert (r["used"], r["extra"], r["twists"], r["fires"], r["fire_last"], r["wraps"]) == (10, 0, 1, 5, 1, False)
    assert m.rng()[1] == 6 and (m.malf == 7).all() and (m.nmalf == 1).all()
    r = m.step()                                   # every counter is busy: the draws happen, nothing is taken
    assert r["twists"] == 0 and m.rng()[1] == 16 and (m.malf == 6).all() and (m.nmalf == 1).all()
    m.reset()
    assert not m.malf.any() and not m.nmalf.any() and m.rng()[1] == 16
    m.set_rng(key, 624)
    r = m.step()
    assert r["starts_at_624"] and r["twists"] == 1 and m.rng()[1] == 10
