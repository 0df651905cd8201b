"""GPU: ensemble runs (gp_ensemble_*, gp_ensemble.hip) -- every member bit-identical to
the CPU oracle run with the same (n, topology, algorithm, seed).

Shapes: line / full n = 1, 2, 64 (P = 2, 3, 65: degree-1 ends, one node past a wave) and
line push-sum n = 63; 3D / Imp3D n = 8, 27, 28 (g = 2 all corners, g = 3 one interior node,
g = 4 after rounding up); n = 1000 for every pair; the population cap of every pair (the
kernels with several node slots per thread); 600 members (more than the workgroups resident
at once).  The oracle converges at all of them within MAX_ROUNDS.
"""
import functools

import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, ensemble_max_nodes
from gossipprotocol_amd import _lib as L
from tests.oracle_ctypes import Oracle

pytestmark = pytest.mark.gpu

TOPOS = ("line", "full", "3D", "Imp3D")
ALGS = ("gossip", "push-sum")
PAIRS = [(t, a) for t in TOPOS for a in ALGS]
SEEDS = [1, 2, 2**63 + 3]  # (the high seed word reaches the Philox key)
MAX_ROUNDS = 200_000


def make_oracle(n, topo, alg, seed, max_rounds=MAX_ROUNDS):
    return Oracle(n, topo, alg, seed, max_rounds=max_rounds, threads=1)


@functools.lru_cache(maxsize=None)
def oracle_final(n, topo, alg, seed, max_rounds=MAX_ROUNDS):
    """The oracle run to its end: (rounds, alerts, seed_node, status, state); computed once."""
    o = make_oracle(n, topo, alg, seed, max_rounds)
    o.run(max_rounds=max_rounds)
    st = o.state()
    for v in st.values():
        v.setflags(write=False)
    status = L.GP_STATUS_CONVERGED if o.alerts_total >= o.T else L.GP_STATUS_MAX_ROUNDS
    out = (o.rounds, o.alerts_total, o.seed_node, status, st)
    o.close()
    return out


def assert_state(got, want, alg, what):
    if alg == "gossip":
        assert np.array_equal(got["c"], want["c"]), f"{what}: c differs"
    else:
        for k in ("s", "w"):  # raw 64-bit patterns
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), f"{what}: {k} differs"
    assert np.array_equal(got["flags"], want["flags"]), f"{what}: flags differ"


def assert_member_final(ens, m, rec, n, topo, alg, seed, max_rounds=MAX_ROUNDS):
    rounds, alerts, seed_node, status, st = oracle_final(n, topo, alg, seed, max_rounds)
    what = f"{topo} {alg} n={n} seed={seed}"
    assert rec.seed == seed, what
    assert (rec.rounds, rec.converged, rec.seed_node, rec.status) == (rounds, alerts, seed_node, status), what
    assert_state(ens.state(m), st, alg, what)


def assert_member_live(ens, m, rec, orc, alg, what):
    assert (rec.rounds, rec.converged, rec.seed_node) == (orc.rounds, orc.alerts_total, orc.seed_node), what
    assert_state(ens.state(m), orc.state(), alg, what)


# ---------------------------------------------------------------- parity to convergence
def parity_cases():
    for topo, alg in PAIRS:
        sizes = [1, 2, 64] if topo in ("line", "full") else [8, 27, 28]
        if (topo, alg) == ("line", "push-sum"):
            sizes.append(63)
        for n in sizes + [1000]:
            yield topo, alg, n


@pytest.mark.parametrize("topo,alg,n", list(parity_cases()))
def test_parity_to_convergence(topo, alg, n):
    with Ensemble(n, topo, alg, SEEDS, max_rounds=MAX_ROUNDS) as ens:
        recs = ens.run()
        assert ens.step(1) == 0
        for m, seed in enumerate(SEEDS):
            assert recs[m].status == L.GP_STATUS_CONVERGED
            assert_member_final(ens, m, recs[m], n, topo, alg, seed)


# ---------------------------------------------------------------- at the cap
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_at_the_cap(topo, alg):
    n = ensemble_max_nodes(topo, alg)
    orc = make_oracle(n, topo, alg, 1)
    with Ensemble(n, topo, alg, [1], max_rounds=MAX_ROUNDS) as ens:
        assert ens.population == orc.P
        for _ in range(2):
            running = ens.step(256)
            orc.step(256)
            assert running == (0 if orc.alerts_total >= orc.T else 1)
            assert_member_live(ens, 0, ens.members()[0], orc, alg, f"{topo} {alg} n={n} round {orc.rounds}")
    orc.close()


# ---------------------------------------------------------------- stepping and resume
@pytest.mark.parametrize("topo,alg", [("3D", "push-sum"), ("Imp3D", "gossip")])
def test_stepping_and_resume(topo, alg):
    n, seeds = 27, [1, 2, 3]
    orcs = [make_oracle(n, topo, alg, s) for s in seeds]
    with Ensemble(n, topo, alg, seeds, max_rounds=MAX_ROUNDS) as ens:
        for m, o in enumerate(orcs):  # before the first round
            assert_member_live(ens, m, ens.members()[m], o, alg, f"{topo} {alg} seed={seeds[m]} at start")
        steps = 0
        while any(o.alerts_total < o.T for o in orcs):
            k = (1, 7, 64)[steps % 3]
            steps += 1
            assert steps < 10_000
            running = ens.step(k)
            for o in orcs:
                o.step(k)  # (a finished oracle stays where it is)
            assert running == sum(o.alerts_total < o.T for o in orcs)
            recs = ens.members()
            for m, o in enumerate(orcs):
                assert_member_live(ens, m, recs[m], o, alg, f"{topo} {alg} seed={seeds[m]} after step {steps}")
                want = L.GP_STATUS_CONVERGED if o.alerts_total >= o.T else L.GP_STATUS_RUNNING
                assert recs[m].status == want
        assert len({o.rounds for o in orcs}) > 1, "the members should finish in different rounds"
    for o in orcs:
        o.close()


# ---------------------------------------------------------------- more members than resident workgroups
def test_more_members_than_resident_workgroups():
    n, topo, alg = 27, "3D", "push-sum"
    seeds = list(range(1, 601))
    with Ensemble(n, topo, alg, seeds, max_rounds=MAX_ROUNDS) as ens:
        recs = ens.run()
        for m, seed in enumerate(seeds):
            rounds, alerts, _, _, _ = oracle_final(n, topo, alg, seed)
            assert (recs[m].rounds, recs[m].converged) == (rounds, alerts), seed
        for m in (0, 255, 256, 599):
            assert_member_final(ens, m, recs[m], n, topo, alg, seeds[m])


# ---------------------------------------------------------------- order and duplicates
def test_order_and_duplicates():
    n, topo, alg = 27, "Imp3D", "push-sum"
    seeds = [5, 1, 5]
    with Ensemble(n, topo, alg, seeds, max_rounds=MAX_ROUNDS) as ens:
        ens.run()
        recs = ens.members()
        assert [r.seed for r in recs] == seeds
        assert_member_final(ens, 1, recs[1], n, topo, alg, 1)
        assert_member_final(ens, 0, recs[0], n, topo, alg, 5)
        a, b = ens.state(0), ens.state(2)
        assert_state(a, b, alg, "duplicate seeds")
        assert (recs[0].rounds, recs[0].converged, recs[0].seed_node, recs[0].status) == \
            (recs[2].rounds, recs[2].converged, recs[2].seed_node, recs[2].status)


# ---------------------------------------------------------------- cap on rounds
@pytest.mark.parametrize("topo,alg", [("3D", "push-sum"), ("line", "gossip")])
def test_cap_on_rounds(topo, alg):
    n = 27
    rounds = {s: oracle_final(n, topo, alg, s)[0] for s in (1, 2, 3, 4)}
    slow = max(rounds, key=rounds.get)
    fast = min(rounds, key=rounds.get)
    assert rounds[fast] < rounds[slow]
    cap = rounds[slow] - 1
    with Ensemble(n, topo, alg, [slow, fast], max_rounds=cap) as ens:
        recs = ens.run()
        assert recs[0].status == L.GP_STATUS_MAX_ROUNDS and recs[0].rounds == cap
        assert_member_final(ens, 0, recs[0], n, topo, alg, slow, max_rounds=cap)
        assert recs[1].status == L.GP_STATUS_CONVERGED
        assert_member_final(ens, 1, recs[1], n, topo, alg, fast, max_rounds=cap)
        assert ens.step(5) == 0  # finished members are not run again
        again = ens.members()
        assert (again[0].rounds, again[1].rounds) == (recs[0].rounds, recs[1].rounds)
        assert_member_final(ens, 0, again[0], n, topo, alg, slow, max_rounds=cap)
