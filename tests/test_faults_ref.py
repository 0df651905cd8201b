"""CPU: the pure-Python SRS v1-F reference (tests/faults_ref.py) -- with no faults it is
SRS v1 round for round (PySim and the C oracle), and its failure model obeys the rules
of SURVEY.md B.5: threshold conversion, the seed node never fails, T_f, mass."""
import math

import numpy as np
import pytest

from oracle.srs_py import PySim
from tests.faults_ref import DOWN, FaultSim, draw_x, threshold, STREAM_FAULT_NODE
from tests.oracle_ctypes import Oracle

SHAPES = [("line", 9), ("full", 12), ("3D", 8), ("Imp3D", 27)]
ALGS = ("gossip", "push-sum")
SEEDS = (1, 2, 2**63 + 3)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("topo,n", SHAPES)
def test_zero_faults_equal_pysim_and_the_c_oracle(topo, n, alg):
    for seed in SEEDS:
        ref = FaultSim(n, topo, alg, seed, max_rounds=5000)  # (line push-sum needs ~1000 rounds even at P = 10)
        py = PySim(n, topo, alg, seed)
        orc = Oracle(n, topo, alg, seed, threads=1)
        assert (ref.doomed, ref.threshold, ref.seed_node) == (0, ref.T, py.seed_node)
        for r in range(5000):
            a, b, c = ref.step(1), py.step(1), orc.step(1)
            assert a == b == c, (topo, alg, seed, r)
            if not a:
                break
            st = orc.state()
            assert ref.flags() == py.flags() == list(st["flags"]), (topo, alg, seed, r)
            if alg == "gossip":
                assert ref.c == py.c == list(st["c"])
            else:
                for mine, theirs, k in ((ref.s, py.s, "s"), (ref.w, py.w, "w")):
                    assert mine == theirs
                    assert np.array_equal(np.array(mine).view(np.uint64), st[k].view(np.uint64))
        assert ref.status == 0 and ref.round == py.round == orc.rounds, (topo, alg, seed)
        assert ref.stats() == (0, 0, ref.T, 0)
        orc.close()


def test_threshold_conversion():
    assert threshold(0.0) == 0
    assert threshold(2.0 ** -32) == 1
    assert threshold(0.5) == 2 ** 31
    assert threshold(1.0) == 2 ** 32  # always: every 32-bit word is below it
    assert threshold(0.25) == 2 ** 30 and threshold(0.1) == math.floor(0.1 * 2 ** 32)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            threshold(bad)


def test_event_iff_word_below_threshold():
    # p = 2^-32 fires only on the word 0; the doomed set follows the draw, not a float compare
    sim = FaultSim(64, "full", "gossip", 1, node_fail=0.5)
    for i in range(sim.P):
        x = draw_x(1, STREAM_FAULT_NODE, i, 0)
        assert sim.D[i] == (i != sim.seed_node and x < 2 ** 31)


@pytest.mark.parametrize("topo,n", SHAPES + [("line", 1), ("full", 64)])
def test_seed_node_never_fails_and_threshold(topo, n):
    for seed in SEEDS:
        for p in (0.25, 0.9, 1.0):
            sim = FaultSim(n, topo, "gossip", seed, node_fail=p)
            assert not sim.D[sim.seed_node]
            assert sim.doomed == sum(sim.D)
            assert sim.threshold == max(1, sim.T - sim.doomed)
            if p == 1.0:
                assert sim.doomed == sim.P - 1 and sim.threshold == 1


def test_down_follows_fail_round():
    sim = FaultSim(27, "Imp3D", "push-sum", 2, node_fail=0.5, fail_round=5, max_rounds=8)
    assert sim.doomed >= 1 and sim.down == 0 and not any(f & DOWN for f in sim.flags())
    sim.step(4)
    assert sim.down == 0 and sim.lost == 0  # nothing is lost before anybody is down
    sim.step(1)
    assert sim.down == sim.doomed
    assert [bool(f & DOWN) for f in sim.flags()] == sim.D


@pytest.mark.parametrize("topo,n", SHAPES)
def test_pushsum_mass(topo, n):
    # no faults: the pairwise halving conserves the sums up to rounding
    sim = FaultSim(n, topo, "push-sum", 1, max_rounds=5000)
    S, W = math.fsum(sim.s), math.fsum(sim.w)
    while not sim.done:
        sim.step(1)
        assert abs(math.fsum(sim.s) - S) <= 1e-9 * S and abs(math.fsum(sim.w) - W) <= 1e-9 * W
    # faults: mass only ever leaves.  Halving is exact, every addition of a fold rounds by at most
    # 2^-53 of its result, and a round makes fewer than P additions: slack = P * 2^-52 of the sum.
    for kw in (dict(node_fail=0.25), dict(msg_drop=0.25), dict(node_fail=0.2, msg_drop=0.1, fail_round=5)):
        sim = FaultSim(n, topo, "push-sum", 1, max_rounds=120, **kw)
        last, lost = math.fsum(sim.w), 0
        while not sim.done:
            sim.step(1)
            now = math.fsum(sim.w)
            slack = last * sim.P * 2.0 ** -52
            assert now <= last + slack
            assert now >= last - slack or sim.lost > lost  # only a lost message takes weight along
            last, lost = now, sim.lost


def test_all_messages_dropped():
    g = FaultSim(9, "line", "gossip", 1, msg_drop=1.0, max_rounds=400).run()
    assert g.status == 0 and g.lost > 0  # the injector is never dropped
    f = FaultSim(12, "full", "gossip", 1, msg_drop=1.0, max_rounds=50).run()
    assert (f.status, f.round, f.alerts_total) == (1, 50, 0) and f.lost == 50
    p = FaultSim(8, "3D", "push-sum", 1, msg_drop=1.0, max_rounds=50).run()
    assert (p.status, p.round, p.lost) == (1, 50, 50) and sum(p.active) == 1
