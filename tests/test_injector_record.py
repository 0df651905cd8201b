"""CPU tests of the injector record: the oracle's accessor to the injector's list against the list
oracle/srs_py.py keeps, round by round at small sizes, and the committed runs of
tests/golden/runs_injector.json against the coverage conditions their generator asserted
(tests/golden/make_golden_injector.py, tests/injector_record.py)."""
import numpy as np
import pytest

from oracle import srs_py
from tests import injector_record as rec
from tests.oracle_ctypes import Oracle


@pytest.mark.parametrize("n,topo", [(200, "line"), (64, "3D"), (125, "Imp3D")])
def test_injector_accessor_matches_python_list(n, topo):
    """After every round to convergence: or_injector_listed over the whole list, a prefix, a
    middle range, single ids at both ends and ranges that reach past T equals the count from
    PySim.live; |L| equals len(PySim.live) and T minus the removals so far, where a removal is
    recomputed here from the round-start state (the pick k = U_INJECT(|L|) was converged)."""
    seed = 3
    o, p = Oracle(n, topo, "gossip", seed), srs_py.PySim(n, topo, "gossip", seed)
    T = o.T
    ranges = [(0, T), (0, T // 3), (T // 3, T // 2), (0, 1), (T - 1, 1), (T - 1, 5), (T, 7), (T // 2, 10 * T), (5, 0)]
    removals = 0
    assert o.injector_live == T == len(p.live)
    while o.alerts_total < T:
        assert o.rounds < 20000, "the oracle did not converge"
        c0 = o.state()["c"]
        pick = p.live[srs_py.uniform(seed, srs_py.STREAM_INJECT, 0, o.rounds, len(p.live))] if p.live else None
        removals += int(pick is not None and c0[pick] >= 11)
        assert o.step(1) == p.step(1)
        assert o.injector_live == len(p.live) == T - removals
        live = np.asarray(p.live, np.int64)
        for first, count in ranges:
            want = int(np.count_nonzero((live >= first) & (live < first + count)))
            assert o.injector_listed(first, count) == want, (o.rounds, first, count)
    assert p.done and removals > 0 and list(o.state()["c"]) == p.c
    assert o.injector_listed(-1, 3) == -1 and o.injector_listed(0, -1) == -1
    o.close()


@pytest.mark.parametrize("n,topo,alg", [(50, "full", "gossip"), (64, "3D", "push-sum"), (50, "line", "push-sum")])
def test_injector_accessor_without_injector(n, topo, alg):
    o = Oracle(n, topo, alg, 3)
    o.step(5)
    assert o.injector_live == -1 and o.injector_listed(0, n) == -1
    o.close()


@pytest.mark.parametrize("name", list(rec.CASES))
def test_recorded_run_meets_its_coverage_conditions(name):
    """The committed record: the case is the one named in injector_record.CASES, it has
    ceil(rounds / 2048) segments, its cumulative alerts never decrease and end at the threshold,
    the list only shrinks, and the coverage conditions hold (check_coverage: converged; line:
    chunk 1 empty with at least 20 000 rounds to run; 3D / Imp3D: chunk 1 down by at least 3000 of
    3385 before the last segment, below 32 at a segment end before the last, |L| < 64 at the end)."""
    case = rec.load()[name]
    n, topo, seed = rec.CASES[name]
    assert (case["num_nodes"], case["topology"], case["algorithm"], case["seed"]) == (n, topo, "gossip", seed)
    P, T, _ = srs_py.resolve(n, topo)
    assert (case["population"], case["threshold"], case["segment"]) == (P, T, rec.SEG)
    nseg = -(-case["rounds"] // rec.SEG)
    assert all(len(case[k]) == nseg for k in rec.FIELDS)
    cum = case["alerts_cum"]
    assert all(a <= b for a, b in zip(cum, cum[1:])) and cum[0] >= 0 and cum[-1] == T == case["alerts_total"]
    assert cum[-2] < T, "the run had converged before its last segment"
    for k in range(2):
        col = [row[k] for row in case["listed"]]
        assert all(a >= b for a, b in zip(col, col[1:])) and col[0] <= min(rec.INJ_CHUNK, T - k * rec.INJ_CHUNK)
    assert all(len(h) == 64 for k in ("alerts_sha256", "c_sha256", "flags_sha256") for h in case[k])
    assert case["oracle_seconds"] > 0
    rec.check_coverage(name, case)
