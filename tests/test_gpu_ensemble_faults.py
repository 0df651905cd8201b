"""GPU: ensembles with a failure model (gp_ensemble_create_faults, gp_ensemble_faults.hip) --
every member bit-identical to the pure-Python SRS v1-F reference (tests/faults_ref.py):
rounds, counted alerts, seed node, status, c or the raw bits of s and w, the flags with
bit 4 (down), and the four gp_fault_stats fields.

Shapes: line / full n = 1, 2 (P = 2, 3), 31, 32 (P = 32, 33: the doomed bitmap's word edge),
64 (one node past a wave); 3D / Imp3D n = 8, 27, 28 (g = 2, 3, 4); line push-sum n = 1100
(two node slots per thread); the failure caps (eight slots per thread, strided gossip loops) for
a few rounds.  Parameter sets (node_fail, msg_drop, fail_round): crashes only,
drops only, both with the crash inside the run, everybody but the seed node down, every
message dropped.  Every reference run is capped at 400 rounds (300 at n = 1100): a member
that has not converged by then ends at max_rounds on both sides.  The one exception is gossip
fed by the injector alone (every message dropped), which must still converge and needs about
12 T rounds of one delivery each: 767 at P = 64 and 65, so those three shapes (line n = 64,
3D / Imp3D n = 28) get 1000 rounds in that one parameter set (the reference is cheap there,
0.5 s a member); P <= 33 converges within 400.
"""
import functools

import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, Faults, ensemble_max_nodes
from gossipprotocol_amd import _lib as L
from tests.faults_ref import FaultSim
from tests.oracle_ctypes import Oracle

pytestmark = pytest.mark.gpu

TOPOS = ("line", "full", "3D", "Imp3D")
ALGS = ("gossip", "push-sum")
PAIRS = [(t, a) for t in TOPOS for a in ALGS]
SEEDS = (1, 2, 2**63 + 3)  # (the high seed word reaches the Philox key)
PARAMS = [(0.25, 0.0, 0), (0.0, 0.25, 0), (0.2, 0.1, 5), (1.0, 0.0, 0), (0.0, 1.0, 0)]
# Where none of SEEDS dooms a node (node_fail > 0) or loses a message, one more seed that
# does: the smallest such seed >= 3, found with the reference on the CPU.  Key: (topology, n,
# algorithm, index into PARAMS).
EXTRA_SEEDS = {(topo, n, alg, k): 4  # (P = 2, 3: one or two nodes that may fail, none does under SEEDS)
               for topo in ("line", "full") for n in (1, 2) for alg in ALGS for k in (0, 2)}


def shapes():
    for topo, alg in PAIRS:
        for n in ([1, 2, 31, 32, 64] if topo in ("line", "full") else [8, 27, 28]):
            yield topo, alg, n, 400
    yield "line", "push-sum", 1100, 300


def seeds_of(topo, alg, n, k):
    extra = EXTRA_SEEDS.get((topo, n, alg, k))
    return SEEDS + ((extra,) if extra is not None else ())


@functools.lru_cache(maxsize=None)
def ref_final(n, topo, alg, seed, params, max_rounds):
    """The reference run to its end, computed once: (rounds, alerts, seed_node, status, state, stats)."""
    nf, md, fr = params
    sim = FaultSim(n, topo, alg, seed, node_fail=nf, msg_drop=md, fail_round=fr, max_rounds=max_rounds).run()
    return snapshot(sim)


def snapshot(sim):
    st = {"flags": np.array(sim.flags(), np.uint8)}
    if sim.algorithm == "gossip":
        st["c"] = np.array(sim.c, np.int32)
    else:
        st["s"], st["w"] = np.array(sim.s, np.float64), np.array(sim.w, np.float64)
    for v in st.values():
        v.setflags(write=False)
    return sim.round, sim.alerts_total, sim.seed_node, sim.status, st, sim.stats()


def assert_state(got, want, alg, what):
    if alg == "gossip":
        assert np.array_equal(got["c"], want["c"]), f"{what}: c differs"
    else:
        for k in ("s", "w"):  # raw 64-bit patterns
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), f"{what}: {k} differs"
    assert np.array_equal(got["flags"], want["flags"]), f"{what}: flags differ"


def assert_member(ens, m, rec, fs, want, alg, what):
    rounds, alerts, seed_node, status, st, stats = want
    print(what, "gpu", (rec.rounds, rec.converged, rec.seed_node, rec.status),
          (fs.doomed, fs.down, fs.threshold, fs.lost), "ref", (rounds, alerts, seed_node, status), stats)
    assert (rec.rounds, rec.converged, rec.seed_node, rec.status) == (rounds, alerts, seed_node, status), what
    assert (fs.doomed, fs.down, fs.threshold, fs.lost) == stats, what
    assert_state(ens.state(m), st, alg, what)


# ---------------------------------------------------------------- parity with the reference
@pytest.mark.parametrize("k", range(len(PARAMS)))
@pytest.mark.parametrize("topo,alg,n,max_rounds", list(shapes()))
def test_parity_with_the_reference(topo, alg, n, max_rounds, k):
    nf, md, fr = PARAMS[k]
    seeds = seeds_of(topo, alg, n, k)
    if k == 4 and alg == "gossip" and topo != "full" and n in (64, 28):
        max_rounds = 1000  # the injector alone needs ~12 T rounds: 767 at P = 64, 65; the smaller shapes fit in 400
    want = [ref_final(n, topo, alg, s, PARAMS[k], max_rounds) for s in seeds]
    # not vacuous: the case dooms a node / loses a message in at least one member
    if nf > 0:
        assert any(w[5][0] >= 1 for w in want), "no member has a doomed node"
    assert any(w[5][3] >= 1 for w in want), "no member loses a message"
    if k == 4:  # every message dropped: only the injector still delivers
        for w in want:
            if alg == "gossip" and topo != "full":
                assert w[3] == L.GP_STATUS_CONVERGED
            else:
                assert (w[0], w[3]) == (max_rounds, L.GP_STATUS_MAX_ROUNDS)
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=Faults(nf, md, fr)) as ens:
        recs = ens.run()
        assert ens.step(1) == 0
        stats = ens.fault_stats()
        for m, seed in enumerate(seeds):
            assert recs[m].seed == seed
            assert_member(ens, m, recs[m], stats[m], want[m], alg, f"{topo} {alg} n={n} {PARAMS[k]} seed={seed}")


# ---------------------------------------------------------------- no faults: the C oracle
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_zero_faults_equal_the_c_oracle(topo, alg):
    n = 64 if topo in ("line", "full") else 27
    with Ensemble(n, topo, alg, SEEDS, max_rounds=200_000, faults=Faults()) as ens:
        recs = ens.run()
        stats = ens.fault_stats()
        for m, seed in enumerate(SEEDS):
            o = Oracle(n, topo, alg, seed, max_rounds=200_000, threads=1)
            o.run(max_rounds=200_000)
            what = f"{topo} {alg} n={n} seed={seed}"
            assert (recs[m].rounds, recs[m].converged, recs[m].seed_node, recs[m].status) == \
                (o.rounds, o.alerts_total, o.seed_node, L.GP_STATUS_CONVERGED), what
            assert_state(ens.state(m), o.state(), alg, what)
            assert (stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost) == (0, 0, o.T, 0), what
            o.close()


# ---------------------------------------------------------------- stepping: the failure round inside a later launch
@pytest.mark.parametrize("topo,alg,n", [("Imp3D", "push-sum", 27), ("line", "gossip", 31), ("full", "push-sum", 32),
                                        ("3D", "gossip", 28)])
def test_stepping_equals_one_run(topo, alg, n):
    params, max_rounds = (0.2, 0.1, 5), 200
    sims = [FaultSim(n, topo, alg, s, *params, max_rounds=max_rounds) for s in SEEDS]
    with Ensemble(n, topo, alg, SEEDS, max_rounds=max_rounds, faults=Faults(*params)) as ens:
        steps = 0
        while not all(s.done for s in sims):
            k = 3 if steps == 0 else (1, 7)[steps % 2]  # rounds 0-2, then round 5 inside a launch of 7
            steps += 1
            running = ens.step(k)
            for s in sims:
                s.step(k)
            assert running == sum(not s.done for s in sims)
            recs, stats = ens.members(), ens.fault_stats()
            for m, s in enumerate(sims):
                assert_member(ens, m, recs[m], stats[m], snapshot(s), alg, f"{topo} {alg} seed={SEEDS[m]} step {steps}")
        assert any(s.doomed >= 1 for s in sims) and any(s.lost >= 1 for s in sims)
        for m, seed in enumerate(SEEDS):  # ... and equal to one run()
            assert snapshot(sims[m])[:4] == ref_final(n, topo, alg, seed, params, max_rounds)[:4]
    with Ensemble(n, topo, alg, SEEDS, max_rounds=max_rounds, faults=Faults(*params)) as ens:
        recs = ens.run()
        stats = ens.fault_stats()
        for m, s in enumerate(sims):
            assert_member(ens, m, recs[m], stats[m], snapshot(s), alg, f"{topo} {alg} seed={SEEDS[m]} one run")


# ---------------------------------------------------------------- many members, duplicate seeds
def test_300_members_with_duplicate_seeds():
    n, topo, alg, params, max_rounds = 27, "Imp3D", "push-sum", (0.2, 0.1, 5), 200
    seeds = [1 + (m % 150) for m in range(300)]
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=Faults(*params)) as ens:
        recs = ens.run()
        stats = ens.fault_stats()
        key = lambda m: (recs[m].seed, recs[m].rounds, recs[m].converged, recs[m].seed_node, recs[m].status,
                         stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost)
        for m in range(150):
            assert key(m) == key(m + 150), m
        for m in (0, 7, 149):
            assert_state(ens.state(m), ens.state(m + 150), alg, f"duplicate of seed {seeds[m]}")
            assert_member(ens, m, recs[m], stats[m], ref_final(n, topo, alg, seeds[m], params, max_rounds), alg,
                          f"member {m}")
        assert len({key(m)[1:] for m in range(150)}) > 1, "the members should differ"


# ---------------------------------------------------------------- a plain ensemble knows no faults
@pytest.mark.parametrize("alg", ALGS)
def test_plain_ensemble_has_no_down_bit_and_zero_stats(alg):
    with Ensemble(27, "Imp3D", alg, SEEDS, max_rounds=200_000) as ens:
        ens.run()
        T = 27
        for m, fs in enumerate(ens.fault_stats()):
            assert (fs.doomed, fs.down, fs.threshold, fs.lost) == (0, 0, T, 0)
            assert not (ens.state(m)["flags"] & L.GP_STATE_DOWN).any()


# ---------------------------------------------------------------- at the failure cap (eight node slots per thread)
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_zero_faults_at_the_failure_cap(topo, alg):
    n = ensemble_max_nodes(topo, alg, faults=True)
    orc = Oracle(n, topo, alg, 1, max_rounds=200_000, threads=1)
    with Ensemble(n, topo, alg, [1], max_rounds=200_000, faults=Faults()) as ens:
        assert ens.population == orc.P
        for _ in range(2):
            running = ens.step(256)
            orc.step(256)
            assert running == (0 if orc.alerts_total >= orc.T else 1)
            rec = ens.members()[0]
            what = f"{topo} {alg} n={n} round {orc.rounds}"
            assert (rec.rounds, rec.converged, rec.seed_node) == (orc.rounds, orc.alerts_total, orc.seed_node), what
            assert_state(ens.state(0), orc.state(), alg, what)
    orc.close()


@pytest.mark.parametrize("topo,alg", [(t, a) for t, a in PAIRS if t != "full"])
def test_faults_at_the_failure_cap(topo, alg):
    # a few rounds only: the reference walks all P nodes every round, but few are active yet
    n, params, max_rounds, seeds = ensemble_max_nodes(topo, alg, faults=True), (0.25, 0.1, 3), 16, (1, 2)
    want = [ref_final(n, topo, alg, s, params, max_rounds) for s in seeds]
    assert all(w[5][0] >= 1000 for w in want) and any(w[5][3] >= 1 for w in want)
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=Faults(*params)) as ens:
        recs = ens.run()
        stats = ens.fault_stats()
        for m, seed in enumerate(seeds):
            assert_member(ens, m, recs[m], stats[m], want[m], alg, f"{topo} {alg} n={n} seed={seed}")


@pytest.mark.parametrize("alg", ALGS)
def test_everybody_down_at_the_full_cap(alg):
    # full topology at its cap, where the reference's neighbour lists would not fit: with every node but
    # the seed node down the run is known in closed form -- the seed node sends into the void every round
    n, R = ensemble_max_nodes("full", alg, faults=True), 20
    with Ensemble(n, "full", alg, [1, 2], max_rounds=R, faults=Faults(node_fail=1.0)) as ens:
        P = ens.population
        recs = ens.run()
        stats = ens.fault_stats()
        for m in range(2):
            sn = recs[m].seed_node
            assert (recs[m].rounds, recs[m].converged, recs[m].status) == (R, 0, L.GP_STATUS_MAX_ROUNDS)
            assert (stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost) == (P - 1, P - 1, 1, R)
            st = ens.state(m)
            flags = np.full(P, L.GP_STATE_DOWN | (0 if alg == "gossip" else 1 << 2), np.uint8)
            flags[sn] = 1 if alg == "gossip" else 1 | (1 << 2)
            assert np.array_equal(st["flags"], flags)
            if alg == "gossip":
                assert not st["c"].any()
            else:
                s, w = np.arange(P, dtype=np.float64), np.ones(P)
                s[sn], w[sn] = sn * 2.0 ** -R, 2.0 ** -R
                assert np.array_equal(st["s"], s) and np.array_equal(st["w"], w)
