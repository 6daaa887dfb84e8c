"""Fate tables and an independent rendering of the device loop's link model (include/hdsm_swarm.h, csrc/link_core.h) for the
tests of hdsm_link_deliver_host (tests/test_links.py) and k_deliver (tests/test_gpu_links.py).

The rendering keeps the WHOLE history of published records (no ring) and states a delivery by arrival time: in link round r the
view of slot k takes the record of the newest round q in [r - D, r] that was not lost, has arrived (q + fate <= r) and is newer
than the one held. The library scans delays newest first over a ring of D + 1 rounds; the two must agree bit for bit."""
import numpy as np

NAN_FRONT = np.frombuffer(np.uint64(0x7ff8000000000000).tobytes(), np.float64)[0]


def crafted_tables(n_rob):
    """name -> int8 [n_rounds][n_rob]; the cases the issue names"""
    t = {}
    a = np.zeros((6, n_rob), np.int8)           # out of order: agent 0's record of round 0 (3 late) lands after that of round 1 (on time)
    a[0, 0], a[1, 0] = 3, 0
    a[2, 1 % n_rob], a[3, 1 % n_rob], a[4, 1 % n_rob] = 2, 1, -1   # ... agent 1's of rounds 2 and 3 land TOGETHER in round 4 (its own is lost): the newer wins
    t["out-of-order"] = a
    b = np.ones((14, n_rob), np.int8)           # latency 1 for everyone (a ring of two); agent 2 dark for 9 rounds, longer than the ring
    b[2:11, 2 % n_rob] = -1
    t["dark-longer-than-ring"] = b
    t["all-lost"] = np.full((3, n_rob), -1, np.int8)
    t["one-round-table"] = np.array([[(k % 3) - 1 for k in range(n_rob)]], np.int8)      # n_rounds = 1: -1, 0, 1 per agent, every round
    c = np.zeros((9, n_rob), np.int8)           # delay 7: the longest ring
    c[:, 0] = 7
    c[4, n_rob - 1] = 7
    t["delay-7"] = c
    return t


def random_table(rng, n_rounds, n_rob, loss, dmax):
    f = rng.integers(0, dmax + 1, size=(n_rounds, n_rob)).astype(np.int8)
    f[rng.random((n_rounds, n_rob)) < loss] = -1
    return f


def random_records(rng, n_slots, n_hor, absent=0.15):
    """published records [n_slots][n_hor+1][9]; some carry the sentinel of an agent without a plan"""
    rec = rng.normal(size=(n_slots, n_hor + 1, 9))
    gone = rng.random(n_slots) < absent
    rec[gone] = 0.0
    rec[gone, 0, 0] = NAN_FRONT
    return rec


class PyLinkView:
    """the independent rendering"""

    def __init__(self, fate, n_slots, n_hor, step_plan, time_aware, plans0, has0):
        self.fate = np.asarray(fate)
        self.n_rounds, self.n_rob = self.fate.shape
        self.D = int(max(0, self.fate.max()))
        self.n_slots, self.N, self.step_plan, self.time_aware = n_slots, n_hor, step_plan, bool(time_aware)
        self.history = []
        self.seen = np.array(plans0, dtype=np.float64, copy=True)
        self.seen_has = np.array(has0, dtype=np.uint8, copy=True)
        self.seen_round = np.full(n_slots, -1, np.int32)
        self.shift = np.zeros(n_slots, np.int32)
        self.counters = np.zeros((n_slots, 4), np.int32)

    def _fate(self, q, k):
        return int(self.fate[q % self.n_rounds, k]) if k < self.n_rob else 0

    def deliver(self, truth):
        r = len(self.history)
        self.history.append(np.array(truth, dtype=np.float64, copy=True))
        for k in range(self.n_slots):
            arrived = [q for q in range(max(0, r - self.D), r + 1)
                       if self._fate(q, k) >= 0 and q + self._fate(q, k) <= r and q > self.seen_round[k]]
            if arrived:
                q = max(arrived)
                self.seen[k] = self.history[q][k]
                self.seen_has[k] = 0 if np.isnan(self.history[q][k, 0, 0]) else 1
                self.seen_round[k] = q
            age = r - int(self.seen_round[k])
            self.shift[k] = min(age * self.step_plan, self.N) if self.time_aware else 0
            self.counters[k] += [1 if arrived else 0, 1 if self._fate(r, k) < 0 else 0, 0, 1]
            self.counters[k, 2] = max(self.counters[k, 2], age)


def same_view(a, b):
    """every array of two views, bit for bit (records with a NaN in front included)"""
    for name in ("seen", "seen_has", "seen_round", "shift", "counters"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), name
