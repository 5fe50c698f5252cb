"""The malfunction side of one env, drawn by numpy itself.  A helper module, not a test; numpy only.

MalfStream steps the counters of A agents the way the reference does (malfunction_generators.py:46-53 and
malfunction_handler.py:35-50), one agent after the other on one np.random.RandomState:

    n = rs.randint(malf_min, malf_max + 1) + 1 if rs.rand() < 1 - exp(-rate) else 0
    a counter at 0 becomes n (and num_malfunctions goes up when n > 0); after all agents every positive counter goes down by one

and counts, from numpy alone, what each step did to the stream: the 32-bit words it consumed, how many of them belong to randint, how
often the MT19937 state was regenerated, which words were the first of a fresh block.  The words of a randint are counted by replaying the
draw on a shadow RandomState with bytes(4) (one raw word per call) through numpy's masked rejection.  The shadow follows the real generator
word for word -- it takes the two words of every rand() raw as well -- and has to agree with it in every value and, after the step, in key
and position, so the count is numpy's and not a second implementation's.

Nothing here reads the step kernel or the C oracle: wcap is recomputed from its definition (the power of two at or above 2 * A + 64).
"""
import numpy as np

MT_N = 624


def wcap_of(A):
    w = 1
    while w < 2 * A + 64:
        w <<= 1
    return w


def rng_of(seed, pos=None):
    """(key u32[624], pos) of RandomState([seed]), the position overwritten when one is given"""
    st = np.random.RandomState([seed]).get_state()
    return np.array(st[1], dtype=np.uint32), int(st[2] if pos is None else pos)


def random_state(key, pos):
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", np.asarray(key, dtype=np.uint32), int(pos)))
    return rs


class MalfStream:
    def __init__(self, key, pos, A, rate, malf_min, malf_max):
        self.rs = random_state(key, pos)
        self.shadow = np.random.RandomState(0)
        self.A, self.malf_min, self.malf_max = int(A), int(malf_min), int(malf_max)
        self.p = float(1 - np.exp(-rate)) if rate > 0 else 0.0
        self.span = self.malf_max - self.malf_min
        m = self.span
        for s in (1, 2, 4, 8, 16):
            m |= m >> s
        self.mask = m
        self.wcap = wcap_of(self.A)
        self.malf = np.zeros(self.A, dtype=np.int32)
        self.nmalf = np.zeros(self.A, dtype=np.int32)
        self.log = []          # one dict per step

    def rng(self):
        st = self.rs.get_state()
        return np.array(st[1], dtype=np.uint32), int(st[2])

    def set_rng(self, key, pos):
        self.rs.set_state(("MT19937", np.asarray(key, dtype=np.uint32), int(pos)))

    def reset(self):
        """the episode ended: fresh agents, the generator runs on"""
        self.malf[:] = 0
        self.nmalf[:] = 0

    def _randint(self, pos0, used, rec):
        """rs.randint(malf_min, malf_max + 1), its words counted on the shadow generator; returns (value, words)"""
        v = int(self.rs.randint(self.malf_min, self.malf_max + 1))
        words = 0
        if self.span != 0:
            while True:
                w = int.from_bytes(self.shadow.bytes(4), "little")
                at_block_start = (pos0 + used + words) % MT_N == 0
                words += 1
                rec["randint_block_start"] += at_block_start
                if (w & self.mask) <= self.span:
                    break
                rec["rejected"] += 1
                rec["rejected_block_start"] += at_block_start
            assert self.malf_min + (w & self.mask) == v, "the shadow replay of randint disagrees with numpy in value"
        else:
            assert v == self.malf_min
        return v, words

    def step(self):
        A = self.A
        st0 = self.rs.get_state()
        pos0 = int(st0[2])
        self.shadow.set_state(st0)
        rec = dict(A=A, pos0=pos0, fires=0, fire_last=0, rejected=0, rejected_block_start=0, randint_block_start=0, max_duration=0,
                   min_duration=1 << 30)
        used = 0
        for i in range(A):
            n = 0
            u = self.rs.rand()
            # the shadow draws the same two words raw: were it one word off after a randint, this rand() would differ
            wa, wb = np.frombuffer(self.shadow.bytes(8), dtype="<u4")
            assert u == ((int(wa) >> 5) * 67108864 + (int(wb) >> 6)) / 9007199254740992.0, "the shadow lost numpy's position"
            used += 2
            if u < self.p:
                v, words = self._randint(pos0, used, rec)
                used += words
                n = v + 1
                rec["fires"] += 1
                rec["fire_last"] += i == A - 1
                rec["max_duration"] = max(rec["max_duration"], n)
                rec["min_duration"] = min(rec["min_duration"], n)
            if self.malf[i] == 0:
                self.malf[i] = n
                if n > 0:
                    self.nmalf[i] += 1
        a, b = self.shadow.get_state(), self.rs.get_state()
        assert a[2] == b[2] and np.array_equal(a[1], b[1]), "the shadow replay disagrees with numpy in state"
        self.malf[self.malf > 0] -= 1
        P = pos0 + used
        rec.update(used=used, extra=used - 2 * A, wraps=used > self.wcap, twists=0 if P <= MT_N else (P - 1) // MT_N,
                   starts_at_624=pos0 == MT_N)
        # the position numpy is left at: in (0, 624] once a word was drawn
        assert int(b[2]) == P - rec["twists"] * MT_N
        self.log.append(rec)
        return rec
