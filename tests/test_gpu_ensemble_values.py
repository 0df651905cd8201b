"""GPU: ensembles over caller-supplied values and weights (gp_ensemble_create_values, SRS v1-V)
against the pure-Python reference tests/values_ref.py, bit-exact on s, w, the flags, the member
records, the failure statistics and the trace rows.

All four topologies at n = 27, 64, 125 and 216 and at one size with two node slots a thread
(gp_ensemble_shape.hpp: 1024 < P <= 2048), each plain, with a failure model and traced, stepped
by 1, by 7 and to the end.  With x_i = i and mean = (P - 1) / 2 a values ensemble equals a plain
one byte for byte; duplicate seeds give duplicate members.
"""
import functools

import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, Faults, Trace, Values
from gossipprotocol_amd import _lib as L
from oracle.srs_py import resolve
from tests import summary_ref, trace_ref
from tests import values_ref as V
from tests.test_gpu_values import values_a, values_b

pytestmark = pytest.mark.gpu

TOPOS = ("line", "full", "3D", "Imp3D")
FAULTS = (0.1, 0.05, 3)
SEEDS = (3, 4, 3)  # a duplicate: members 0 and 2 must agree in everything
MEAN = 7.3         # supplied, not the data's: the errors are measured against what the caller says
# (n, max_rounds): the small sizes, and two node slots a thread with a cap the reference can afford
SIZES = [(27, 400), (64, 400), (125, 400), (216, 300)]
TWO_SLOTS = {"line": (1100, 40), "full": (1100, 25), "3D": (1331, 40), "Imp3D": (1331, 40)}
CASES = [(t, n, cap) for t in TOPOS for n, cap in SIZES] + [(t,) + TWO_SLOTS[t] for t in TOPOS]


def data(P, n):
    return (values_a if n % 2 == 0 else values_b)(P)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def ref_sim(topo, n, cap, seed, faults):
    P = resolve(n, topo)[0]
    x, w = data(P, n)
    return V.ValueSim(n, topo, x, w, seed, MEAN, *(faults or (0.0, 0.0, 0)), max_rounds=cap)


@functools.lru_cache(maxsize=None)
def ref_run(topo, n, cap, seed, faults):
    """The reference stepped 1, 7 and to the end: the three states, then (rounds, alerts, status, stats)."""
    sim = ref_sim(topo, n, cap, seed, faults)
    states = []
    for k in (1, 7, cap):
        sim.step(k)
        states.append((sim.round, sim.state()))
    return states, (sim.round, sim.alerts_total, sim.status, sim.stats())


def make(topo, n, cap, faults=None, trace=None):
    P = resolve(n, topo)[0]
    x, w = data(P, n)
    return Ensemble(n, topo, "push-sum", SEEDS, cap, faults=None if faults is None else Faults(*faults),
                    trace=trace, values=Values(x, w, mean=MEAN))


def assert_members(e, topo, n, cap, faults, step):
    for m, seed in enumerate(SEEDS):
        states, _ = ref_run(topo, n, cap, seed, faults)
        rounds, want = states[step]
        got = e.state(m)
        assert e.members()[m].rounds == rounds
        for f in ("s", "w"):
            bad = np.nonzero(got[f].view(np.uint64) != want[f].view(np.uint64))[0]
            assert not len(bad), f"{topo} n={n} member {m} round {rounds}: {f}[{bad[0]}] = {got[f][bad[0]]!r}, reference {want[f][bad[0]]!r}"
        assert np.array_equal(got["flags"], want["flags"]), f"{topo} n={n} member {m} round {rounds}: flags"


@pytest.mark.parametrize("variant", ["plain", "faults", "traced"])
@pytest.mark.parametrize("topo,n,cap", CASES, ids=lambda v: str(v))
def test_members_match_the_reference(topo, n, cap, variant):
    faults = FAULTS if variant == "faults" else None
    e = make(topo, n, cap, faults, Trace(1) if variant == "traced" else None)
    for step, k in enumerate((1, 7, None)):
        if k is None:
            e.run()
        else:
            e.step(k)
        assert_members(e, topo, n, cap, faults, step)
    stats = e.fault_stats()
    sums = e.summary(0.5)
    for m, seed in enumerate(SEEDS):
        states, (rounds, alerts, status, fstats) = ref_run(topo, n, cap, seed, faults)
        final = states[2][1]
        rec = e.members()[m]
        assert (rec.seed, rec.rounds, rec.converged, rec.status) == (seed, rounds, alerts, status)
        if faults:
            assert (stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost) == fstats
        if variant == "plain":  # the summary measures against the supplied mean
            ref = V.ref_summary(final, 0, e.population, rounds, rec.seed_node, 0.5, MEAN)
            summary_ref.assert_exact(sums[m], ref, f"{topo} n={n} member {m}")
        if variant == "traced":
            rows, r_rounds, r_alerts, _ = V.trace_rows(ref_sim(topo, n, cap, seed, None))
            assert (r_rounds, r_alerts) == (rounds, alerts)
            trace_ref.assert_rows_equal(e.trace(m), rows, f"{topo} n={n} member {m}")
    # duplicate seeds give duplicate members
    a, b = e.state(0), e.state(2)
    assert all(np.array_equal(raw(a[f]), raw(b[f])) for f in ("s", "w", "flags"))
    if variant == "traced":
        assert e.trace(0).tobytes() == e.trace(2).tobytes()
    e.close()


@pytest.mark.parametrize("topo", TOPOS)
def test_ids_as_values_equal_a_plain_ensemble(topo):
    n, cap = 125, 300
    P = resolve(n, topo)[0]
    kw = dict(faults=Faults(*FAULTS), trace=Trace(2))
    vals = Values(np.arange(P, dtype=np.float64), np.ones(P), mean=(P - 1) / 2)
    for k in (0, 1):
        v = Ensemble(n, topo, "push-sum", SEEDS, cap, values=vals if k == 0 else Values(np.arange(P, dtype=np.float64)), **kw)
        p = Ensemble(n, topo, "push-sum", SEEDS, cap, **kw)
        assert v.values.mean == (P - 1) / 2
        for step in (0, 5, None):
            for e in (v, p):
                e.run() if step is None else e.step(step)
            for m in range(len(SEEDS)):
                a, b = v.state(m), p.state(m)
                assert all(np.array_equal(raw(a[f]), raw(b[f])) for f in ("c", "s", "w", "flags"))
                assert v.trace(m).tobytes() == p.trace(m).tobytes()
            assert [summary_ref.raw(s) for s in v.summary()] == [summary_ref.raw(s) for s in p.summary()]
            assert [bytes(x) for x in v.members()] == [bytes(x) for x in p.members()]
            assert [bytes(x) for x in v.fault_stats()] == [bytes(x) for x in p.fault_stats()]
        v.close()
        p.close()


def test_inadmissible_values_are_refused():
    x, w = values_b(125)
    for bad_id, (bx, bw), word in ((17, (-0.0, 1.0), "finite"), (124, (1.0, 2.0 ** 33), "2^-32, 2^32"), (0, (2.0 ** 32, 1.0), "below")):
        x2, w2 = x.copy(), w.copy()
        x2[bad_id], w2[bad_id] = bx, bw
        with pytest.raises(L.GossipError) as ei:
            Ensemble(125, "3D", "push-sum", SEEDS, 100, values=Values(x2, w2, mean=1.0))
        assert ei.value.code == -1 and f"node {bad_id} " in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(L.GossipError) as ei:
        Ensemble(125, "3D", "gossip", SEEDS, 100, values=Values(x, w))
    assert "gossip" in str(ei.value)
