"""GPU: the ensemble kernels at their node-slot and workgroup-size edges -- every member
bit-identical to the reference (the C oracle; tests/faults_ref.py and tests/trace_ref.py for the
failure and traced variants): raw 64-bit patterns of s and w, flags, c, the records, the fault
stats, the trace rows.

ens_kernel picks k_ens_pushsum<TOPO, NPT, ...> with NPT = 1, 2, 4, 8 node slots per thread and
ens_threads a workgroup of whole waves (gp_ensemble_shape.hpp; tests/ensemble_shape_ref.py mirrors
both, tests/test_ensemble_shape.py holds the mirror against the header).  The other ensemble modules
run n <= 1000 (NPT 1), line n = 1100 (NPT 2) and each pair's cap (NPT 8).  Here:

  line, full n = 1023, 1024, 2047, 2048, 4095, 4096   P = n + 1: NPT 1 | 2, 2 | 4, 4 | 8; the second
                                                      of each pair in 576 threads, last slot partly filled
  3D, Imp3D n = 11^3, 13^3, 16^3, 17^3                 NPT 2 (704 threads), 4 (576), 4 (1024: every slot
                                                      full), 8 (640)
  line gossip n = 2047, 2048, 2049                    injector bitmap of 64, 64, 65 words: one word per
                                                      lane of wave 0, the last one of 31 bits; then two
                                                      words per lane, lanes 33..63 empty

Every case asserts from the reference's state alone that it is not vacuous: at the final compare
every slot q < npt (gossip: every pass of the strided loops) holds a touched node (push-sum: active
bit; gossip: c >= 1), and for 3D / Imp3D push-sum both ends of a lattice edge across every slot
boundary are touched.  ROUNDS is the smallest multiple of 64 at which the oracle meets that for
every seed, found on the CPU: 64 everywhere but three line gossip sizes.  Because that is so few
rounds, every pair but two also runs to convergence (the oracle converges at all of them within
MAX_ROUNDS, the slowest member after 12 567 rounds): the injector's removal path with its shrinking
live count runs there.  3D push-sum runs to convergence at g = 11, 13 only (the oracle needs 4 to 5 s
a member at g = 16, 17); line push-sum not at all (hundreds of thousands of rounds).

Line push-sum: activity spreads about +-250 nodes in 512 rounds, so coverage comes from seeds, not
rounds.  LINE_PS_SEEDS holds, per size, the smallest seed for either end of the line and for every
slot boundary b = q * threads such that after 512 rounds the oracle has the end node, or both b - 1
and b, active.  All seeds of a size are members of one ensemble.

Failure and traced variants, parameters (0.2, 0.1, 5), 64 rounds (200 for line gossip): the doomed
bitmap at P % 64 = 1, 21, 51 with several slots, two words per injector lane (line gossip n = 2049),
a doomed bitmap of 69 words (3D gossip n = 2197).  With a fifth of a line's nodes down, activity
stays between the two nearest down nodes: none of LINE_PS_SEEDS' members reaches a slot boundary
under the failure model, so FAULT_LINE_SEEDS holds the two smallest seeds whose seed node sits on
boundary 4032 of n = 4096 and whose reference run has both 4031 and 4032 active after 64 rounds.
"""
import functools

import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, Faults
from gossipprotocol_amd import _lib as L
from oracle.srs_py import resolve
from tests import ensemble_shape_ref as sh
from tests import trace_ref
from tests.faults_ref import FaultSim
from tests.test_gpu_ensemble import (MAX_ROUNDS, SEEDS, assert_member_final, assert_member_live, make_oracle,
                                     oracle_final)
from tests.test_gpu_ensemble_faults import assert_member, snapshot
from tests.test_gpu_ensemble_trace import check

pytestmark = pytest.mark.gpu

LINE_SIZES = (1023, 1024, 2047, 2048, 4095, 4096)
CUBE_SIZES = (11 ** 3, 13 ** 3, 16 ** 3, 17 ** 3)
# rounds of the lock-step cases: 64 but for (found on the CPU with the oracle, see the module docstring)
ROUNDS = {("line", "gossip", 1024): 128, ("line", "gossip", 2048): 128, ("line", "gossip", 4096): 128}
# line push-sum: seeds for (node 0, every slot boundary in ascending order, node P - 1)
LINE_PS_ROUNDS = 512
LINE_PS_SEEDS = {1023: (7, 2),
                 1024: (7, 4, 2),
                 1100: (7, 4, 2),
                 2047: (8, 9, 3),
                 2048: (8, 1, 4, 2, 3),
                 4095: (8, 1, 18, 2, 28),
                 4096: (8, 7, 1, 15, 9, 4, 2, 3, 28),
                 8191: (8, 42, 1, 15, 41, 9, 11, 20, 28)}
FAULT_PARAMS = (0.2, 0.1, 5)
FAULT_LINE_SEEDS = (91, 172)  # seed nodes 4031 and 4033, either side of boundary 4032


# ---------------------------------------------------------------- coverage, from the reference's state
def touched(st, alg):
    return (st["flags"] & 1).astype(bool) if alg == "push-sum" else np.asarray(st["c"]) >= 1


def slots_touched(t, alg, P):
    thr = sh.threads(alg, P)
    return [bool(t[q * thr:(q + 1) * thr].any()) for q in range(sh.slots(alg, P))]


def boundary_crossed(t, b, g, P):
    """Both ends of a lattice edge (i, i + d), i < b <= i + d, touched: d = 1 in a row, g in a plane, g * g."""
    for d in (1, g, g * g):
        i = np.arange(max(0, b - d), b)
        i = i[i + d < P]
        if d == 1:
            i = i[i % g != g - 1]
        elif d == g:
            i = i[(i // g) % g != g - 1]
        if (t[i] & t[i + d]).any():
            return True
    return False


def assert_covered(st, topo, alg, n, what):
    P, _, g = resolve(n, topo)
    t = touched(st, alg)
    assert all(slots_touched(t, alg, P)), f"{what}: a slot without a touched node {slots_touched(t, alg, P)}"
    if alg == "push-sum" and topo in ("3D", "Imp3D"):
        for b in sh.boundaries(alg, P):
            assert boundary_crossed(t, b, g, P), f"{what}: nothing across slot boundary {b}"


# ---------------------------------------------------------------- plain kernels, lock-step with the oracle
def lock_step_cases():
    for topo in ("line", "full", "3D", "Imp3D"):
        for alg in ("gossip", "push-sum"):
            if (topo, alg) != ("line", "push-sum"):  # (test_line_push_sum_reaches_every_slot_boundary)
                for n in (LINE_SIZES if topo in ("line", "full") else CUBE_SIZES):
                    yield topo, alg, n


def lock_step(n, topo, alg, seeds, rounds):
    """Two chunks of rounds / 2 with a full compare of every member after each; returns the oracles' states."""
    orcs = [make_oracle(n, topo, alg, s) for s in seeds]
    with Ensemble(n, topo, alg, list(seeds), max_rounds=MAX_ROUNDS) as ens:
        assert ens.population == orcs[0].P
        for _ in range(2):
            running = ens.step(rounds // 2)
            for o in orcs:
                o.step(rounds // 2)
            assert running == sum(o.alerts_total < o.T for o in orcs)
            recs = ens.members()
            for m, o in enumerate(orcs):
                assert_member_live(ens, m, recs[m], o, alg, f"{topo} {alg} n={n} seed={seeds[m]} round {o.rounds}")
    states = [o.state() for o in orcs]
    for o in orcs:
        o.close()
    return states


@pytest.mark.parametrize("topo,alg,n", list(lock_step_cases()))
def test_lock_step_with_the_oracle(topo, alg, n):
    states = lock_step(n, topo, alg, SEEDS, ROUNDS.get((topo, alg, n), 64))
    for seed, st in zip(SEEDS, states):
        assert_covered(st, topo, alg, n, f"{topo} {alg} n={n} seed={seed}")


# ---------------------------------------------------------------- plain kernels, to convergence
def convergence_cases():
    for topo, alg in (("full", "gossip"), ("full", "push-sum"), ("Imp3D", "gossip"), ("Imp3D", "push-sum"),
                      ("3D", "gossip"), ("line", "gossip")):
        for n in (LINE_SIZES if topo in ("line", "full") else CUBE_SIZES):
            yield topo, alg, n
    yield "line", "gossip", 2049  # 65 injector words: two per lane of wave 0
    yield "3D", "push-sum", 11 ** 3
    yield "3D", "push-sum", 13 ** 3


@pytest.mark.parametrize("topo,alg,n", list(convergence_cases()))
def test_to_convergence(topo, alg, n):
    with Ensemble(n, topo, alg, SEEDS, max_rounds=MAX_ROUNDS) as ens:
        recs = ens.run()
        assert ens.step(1) == 0
        for m, seed in enumerate(SEEDS):
            want = oracle_final(n, topo, alg, seed)
            assert want[3] == L.GP_STATUS_CONVERGED  # (the oracle converges within MAX_ROUNDS)
            assert_covered(want[4], topo, alg, n, f"{topo} {alg} n={n} seed={seed}")
            assert_member_final(ens, m, recs[m], n, topo, alg, seed)


# ---------------------------------------------------------------- line push-sum: a seed per slot boundary and end
@pytest.mark.parametrize("n", sorted(LINE_PS_SEEDS))
def test_line_push_sum_reaches_every_slot_boundary(n):
    P, seeds = n + 1, LINE_PS_SEEDS[n]
    targets = [0] + sh.boundaries("push-sum", P) + [P - 1]
    assert len(seeds) == len(targets) == sh.npt(P) + 1
    states = lock_step(n, "line", "push-sum", seeds, LINE_PS_ROUNDS)
    covered = np.zeros(P, bool)
    for seed, b, st in zip(seeds, targets, states):
        t = touched(st, "push-sum")
        covered |= t
        if b in (0, P - 1):
            assert t[b], f"n={n} seed={seed}: end node {b} not active"
        else:
            assert t[b - 1] and t[b], f"n={n} seed={seed}: nodes {b - 1}, {b} not both active"
    assert all(slots_touched(covered, "push-sum", P))


# ---------------------------------------------------------------- failure and traced variants
# topology, algorithm, n, rounds, seeds
FAULT_SHAPES = [("3D", "push-sum", 13 ** 3, 64, (1, 2)),      # NPT 4, 576 threads, P % 64 = 21
                ("Imp3D", "push-sum", 11 ** 3, 64, (1, 2)),   # NPT 2, 704 threads
                ("full", "push-sum", 2048, 64, (1, 2)),       # NPT 4, 576 threads, P % 64 = 1
                ("line", "push-sum", 4096, 64, FAULT_LINE_SEEDS),  # NPT 8, 576 threads, P % 64 = 1
                ("line", "gossip", 2049, 200, (1, 2)),        # 65 injector words, three passes
                ("3D", "gossip", 13 ** 3, 64, (1, 2))]        # three passes, doomed bitmap of 69 words
FAULT_IDS = [f"{t}-{a}-{n}" for t, a, n, _, _ in FAULT_SHAPES]
TRACE_SHAPES = [s for s in FAULT_SHAPES if s[:3] in (("Imp3D", "push-sum", 11 ** 3), ("3D", "push-sum", 13 ** 3))]


@functools.lru_cache(maxsize=None)
def fault_ref(n, topo, alg, seed, rounds):
    """The failure reference run to its end, once: (snapshot, slots that hold a doomed node, active nodes)."""
    sim = FaultSim(n, topo, alg, seed, *FAULT_PARAMS, max_rounds=rounds).run()
    slots = frozenset(sh.slot_of(i, alg, sim.P) for i in range(sim.P) if sim.D[i])
    active = tuple(sim.active) if alg == "push-sum" else None
    return snapshot(sim), slots, active


def assert_faults_bite(topo, alg, n, rounds, seeds):
    """Every member dooms nodes in at least two slots and loses a message; the line members cross a boundary."""
    for seed in seeds:
        (_, _, _, _, _, stats), slots, active = fault_ref(n, topo, alg, seed, rounds)
        assert stats[0] >= 1 and stats[3] >= 1 and len(slots) >= 2, (seed, stats, slots)
        if (topo, alg) == ("line", "push-sum"):
            b = 4032
            assert b in sh.boundaries(alg, n + 1) and active[b - 1] and active[b], seed


@pytest.mark.parametrize("topo,alg,n,rounds,seeds", FAULT_SHAPES, ids=FAULT_IDS)
def test_failure_variant(topo, alg, n, rounds, seeds):
    assert_faults_bite(topo, alg, n, rounds, seeds)
    with Ensemble(n, topo, alg, list(seeds), max_rounds=rounds, faults=Faults(*FAULT_PARAMS)) as ens:
        recs = ens.run()
        assert ens.step(1) == 0
        stats = ens.fault_stats()
        for m, seed in enumerate(seeds):
            assert recs[m].seed == seed
            assert_member(ens, m, recs[m], stats[m], fault_ref(n, topo, alg, seed, rounds)[0], alg,
                          f"{topo} {alg} n={n} {FAULT_PARAMS} seed={seed}")


@pytest.mark.parametrize("topo,alg,n,rounds,seeds", FAULT_SHAPES, ids=FAULT_IDS)
def test_failure_and_trace_variant(topo, alg, n, rounds, seeds):
    # rows against trace_ref; members, state, stats and summary against the failure variant of the same arguments
    assert_faults_bite(topo, alg, n, rounds, seeds)
    got, want = check(n, topo, alg, seeds, rounds, faults=FAULT_PARAMS)
    for m, seed in enumerate(seeds):
        assert want[m][3] == fault_ref(n, topo, alg, seed, rounds)[0][5]
        assert len(got[m]) == want[m][1] >= 1


@pytest.mark.parametrize("topo,alg,n,rounds,seeds", TRACE_SHAPES, ids=[f"{t}-{a}-{n}" for t, a, n, _, _ in TRACE_SHAPES])
def test_trace_variant_without_faults(topo, alg, n, rounds, seeds):
    assert sorted(sh.npt(resolve(s[2], s[0])[0]) for s in TRACE_SHAPES) == [2, 4]
    got, want = check(n, topo, alg, seeds, rounds)
    for m in range(len(seeds)):
        assert len(got[m]) == rounds
        assert got[m]["reached"][-1] > 1 and got[m]["sent"][-1] > rounds
    for seed in seeds:  # the oracle's state after the same rounds: every slot touched
        o = make_oracle(n, topo, alg, seed)
        o.step(rounds)
        assert_covered(o.state(), topo, alg, n, f"{topo} {alg} n={n} seed={seed}")
        o.close()
