"""Reference of ensemble traces (SRS v1-T): the rows a traced member records.

TEST INFRASTRUCTURE.  Steps the C oracle (tests/oracle_ctypes.py; no failure model) or the
pure-Python SRS v1-F simulator (tests/faults_ref.py; with one) a round at a time and derives
each row from the state, with nothing from the library under test:

  round    R, the rounds completed
  reached  gossip: nodes with c >= 1, or the seed node; push-sum: nodes with the active bit
  alerts   the cumulative counted alerts
  sent     the sender predicate evaluated on the state before each of the rounds 1..R, summed:
           gossip (seed node or c >= 1) and c <= 10, push-sum active; with a failure model: and
           not down in that round
  err_max  push-sum: the largest bit pattern, sign bit cleared, of fl(fl(s / w) - mu) over all P
           nodes, mu = (P - 1) / 2; a pattern above +inf's becomes the quiet NaN
           0x7FF8000000000000.  gossip: 0.0

A row is taken after round R iff R % stride == 0 and R / stride - 1 < capacity (capacity 0:
max_rounds // stride).
"""
from __future__ import annotations

import functools

import numpy as np

from tests.faults_ref import FaultSim
from tests.oracle_ctypes import Oracle

ROW = np.dtype([("round", "<i8"), ("reached", "<u4"), ("alerts", "<u4"), ("sent", "<u8"), ("err_max", "<f8")])
ABS_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
INF_BITS = 0x7FF0000000000000
QNAN_BITS = 0x7FF8000000000000


def err_max_bits(s, w, population):
    """The err_max of a row as its 64-bit pattern."""
    mu = (population - 1) * 0.5
    with np.errstate(all="ignore"):
        e = np.asarray(s, np.float64) / np.asarray(w, np.float64) - mu
    top = int((e.view(np.uint64) & ABS_MASK).max())
    return QNAN_BITS if top > INF_BITS else top


class _Plain:
    """The C oracle behind the few calls the row needs."""

    def __init__(self, n, topo, alg, seed, max_rounds):
        self.o = Oracle(n, topo, alg, seed, max_rounds=max_rounds, threads=1)
        self.alg, self.P, self.seed_node, self.max_rounds = alg, self.o.P, self.o.seed_node, max_rounds

    def step1(self):
        if self.o.alerts_total >= self.o.T or self.o.rounds >= self.max_rounds:
            return False
        return len(self.o.step(1)) == 1

    def rounds(self):
        return self.o.rounds

    def alerts(self):
        return self.o.alerts_total

    def state(self):
        return self.o.state()

    def down(self):
        return np.zeros(self.P, bool)


class _Faulty:
    """tests/faults_ref.py's FaultSim behind the same calls."""

    def __init__(self, n, topo, alg, seed, max_rounds, faults):
        self.f = FaultSim(n, topo, alg, seed, *faults, max_rounds=max_rounds)
        self.alg, self.P, self.seed_node = alg, self.f.P, self.f.seed_node

    def step1(self):
        return len(self.f.step(1)) == 1

    def rounds(self):
        return self.f.round

    def alerts(self):
        return self.f.alerts_total

    def state(self):
        if self.alg == "gossip":
            return {"c": np.array(self.f.c, np.int32)}
        return {"s": np.array(self.f.s, np.float64), "w": np.array(self.f.w, np.float64),
                "flags": np.array(self.f.active, np.uint8)}

    def down(self):
        """Who is down in the round about to run."""
        return np.array([self.f.is_down(i, self.f.round) for i in range(self.P)], bool)


def knows(sim, st):
    """gossip: the node knows the rumour; push-sum: it is active.  (The nodes `reached` counts.)"""
    if sim.alg == "gossip":
        k = st["c"] >= 1
        k[sim.seed_node] = True
        return k
    return (st["flags"] & 1).astype(bool)


def senders(sim, st):
    """The nodes that draw a target in the round about to run."""
    k = knows(sim, st)
    if sim.alg == "gossip":
        k &= st["c"] <= 10
    return k & ~sim.down()


@functools.lru_cache(maxsize=None)
def trace(n, topo, alg, seed, stride=1, capacity=0, max_rounds=400, faults=None):
    """(rows, rounds, alerts, stats) of the member run to its end: rows a read-only structured
    array (ROW); stats the reference's (doomed, down, threshold, lost), None without a failure
    model.  faults: None or (node_fail, msg_drop, fail_round)."""
    sim = _Plain(n, topo, alg, seed, max_rounds) if faults is None else _Faulty(n, topo, alg, seed, max_rounds, faults)
    capacity = capacity or max_rounds // stride
    rows, sent = [], 0
    st = sim.state()
    while True:
        sent += int(senders(sim, st).sum())
        if not sim.step1():
            break
        st = sim.state()
        R = sim.rounds()
        if R % stride == 0 and R // stride - 1 < capacity:
            err = err_max_bits(st["s"], st["w"], sim.P) if alg == "push-sum" else 0
            rows.append((R, int(knows(sim, st).sum()), sim.alerts(), sent, np.array([err], np.uint64).view(np.float64)[0]))
    out = np.array(rows, ROW) if rows else np.zeros(0, ROW)
    out.setflags(write=False)
    return out, sim.rounds(), sim.alerts(), (None if faults is None else sim.f.stats())


def assert_rows_equal(got, want, what=""):
    """Every field for equality; err_max by its bits (a NaN must be the canonical one)."""
    assert len(got) == len(want), f"{what}: {len(got)} rows, reference {len(want)}"
    for k in ("round", "reached", "alerts", "sent"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert not len(bad), f"{what}: {k} differs first at row {bad[0]}: {got[k][bad[0]]} != {want[k][bad[0]]}"
    g, w = got["err_max"].view(np.uint64), want["err_max"].view(np.uint64)
    bad = np.nonzero(g != w)[0]
    assert not len(bad), f"{what}: err_max differs first at row {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"
