"""GPU: ensembles over a caller-supplied graph (gp_ensemble_create_graph, SRS v1-G, DESIGN.md
section 14), bit-exact on c, the raw bits of s and w, the flags, rounds, alerts, seed node and status.

Against the built-in kernels: gossip on Graph.lattice3d(g) is the "3D" ensemble member for member,
on Graph.imp3d(4, seed) the "Imp3D" member of that seed (tests/test_graph_ref.py shows why).
Against the pure-Python reference tests/graph_ref.py, both algorithms, at the shapes where the
kernels can go wrong: P = 2; ring(P, 2) at the bitmap-word and wave edges 33, 64, 65; ring(1025, 4),
the first population with two node slots, the second holding one node (gossip) or 449 (push-sum),
with seeds whose seed node sits at a slot edge; star(65) (in-degree 64 against 1); a directed cycle
(in-list != out-list); self-loops and duplicates; the largest entry count that fits at P = 64; two
components (push-sum ends at max_rounds).  Then launch splitting, the failure / trace / values
variants on a small world, and the summary.
"""
import functools

import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, Faults, Graph, Trace, Values, ensemble_graph_lds_bytes
from oracle.srs_py import STREAM_START, uniform
from tests import graph_ref, summary_ref, trace_ref
from tests import values_ref as V
from tests.ensemble_shape_ref import ENS_LDS_MAX, boundaries
from tests.graph_ref import GraphSim

pytestmark = pytest.mark.gpu

ALGS = ("gossip", "push-sum")
CONVERGED, MAX_ROUNDS = 0, 1
HIGH = (9 << 32) | 4  # a seed with the high word set


def slot_edge_seeds(P, near, count=1):
    """The first seeds whose seed node U_START(P) lies within 20 ids of `near`."""
    out, s = [], 1
    while len(out) < count:
        if abs(uniform(s, STREAM_START, 0, 0, P) - near) <= 20:
            out.append(s)
        s += 1
    return out


def cycle(n):
    return Graph.from_edges(n, [(i, (i + 1) % n) for i in range(n)], directed=True)


def loops12():
    """12 nodes on a ring, plus a self-loop at 3, a duplicated out-edge 5 -> 6 and a one-way chord."""
    e = [(i, (i + 1) % 12) for i in range(12)] + [((i + 1) % 12, i) for i in range(12)]
    return Graph.from_edges(12, e + [(3, 3), (5, 6), (5, 6), (9, 2)], directed=True)


def two_components():
    e = [(i, (i + 1) % 5) for i in range(5)] + [(5 + i, 5 + (i + 1) % 7) for i in range(7)]
    return Graph.from_edges(12, e)


# name -> (graph of the algorithm, max_rounds, seeds)
CASES = {
    "p2": (lambda alg: Graph.from_edges(2, [(0, 1)]), 600, (1, 2, HIGH)),
    "ring33": (lambda alg: Graph.ring(33, 2), 600, (1, HIGH)),
    "ring64": (lambda alg: Graph.ring(64, 2), 600, (1, HIGH)),
    "ring65": (lambda alg: Graph.ring(65, 2), 600, (1, HIGH)),
    # gossip: pass 1 of the strided loops is node 1024 alone; push-sum: slot 1 starts at node 576:
    # a seed that starts next to either, and one with the high word set
    "ring1025": (lambda alg: Graph.ring(1025, 4), 60,
                 (slot_edge_seeds(1025, 1024)[0], slot_edge_seeds(1025, boundaries("push-sum", 1025)[0])[0], HIGH)),
    "star65": (lambda alg: Graph.star(65), 600, (1, HIGH)),
    "cycle40": (lambda alg: cycle(40), 600, (1, HIGH)),
    "loops12": (lambda alg: loops12(), 600, (1, 2, HIGH)),
    "fullest64": (lambda alg: Graph(*graph_ref.fullest_graph(64, alg)), 300, (1, HIGH)),
    "two_components": (lambda alg: two_components(), 150, (1, 2, HIGH)),
}


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def graph_of(name, alg):
    return CASES[name][0](alg)


@functools.lru_cache(maxsize=None)
def ref_run(name, alg, seed, faults=None, values=False):
    g, cap = graph_of(name, alg), CASES[name][1]
    x, w = data(g.num_nodes) if values else (None, None)
    sim = GraphSim(g, alg, seed, *(faults or (0.0, 0.0, 0)), max_rounds=cap, x=x, w=w, mean=MEAN if values else None)
    return sim.run()


def assert_member(e, m, sim, what):
    rec, got, want = e.members()[m], e.state(m), sim.state()
    assert (rec.seed, rec.rounds, rec.converged, rec.seed_node, rec.status) == \
        (sim.seed, sim.round, sim.alerts_total, sim.seed_node, sim.status), what
    assert np.array_equal(got["c"], want["c"]), f"{what}: c"
    for f in ("s", "w"):
        bad = np.nonzero(got[f].view(np.uint64) != want[f].view(np.uint64))[0]
        assert not len(bad), f"{what}: {f}[{bad[0]}] = {got[f][bad[0]]!r}, reference {want[f][bad[0]]!r}"
    assert np.array_equal(got["flags"], want["flags"]), f"{what}: flags"


# ---- against the built-in kernels --------------------------------------------------------------
@pytest.mark.parametrize("g", (3, 4))
def test_lattice3d_gossip_equals_the_3d_ensemble(g):
    seeds = list(range(1, 16)) + [HIGH]
    with Ensemble.on_graph(Graph.lattice3d(g), "gossip", seeds, 5000) as a, Ensemble(g ** 3, "3D", "gossip", seeds, 5000) as b:
        ra, rb = a.run(), b.run()
        for m in range(16):
            assert [getattr(ra[m], k) for k in ("seed", "rounds", "converged", "seed_node", "status")] == \
                   [getattr(rb[m], k) for k in ("seed", "rounds", "converged", "seed_node", "status")]
            sa, sb = a.state(m), b.state(m)
            assert all(np.array_equal(raw(sa[k]), raw(sb[k])) for k in ("c", "s", "w", "flags")), m
            assert ra[m].status == CONVERGED


@pytest.mark.parametrize("seed", (1, 6, HIGH))
def test_imp3d_gossip_equals_the_imp3d_member_of_that_seed(seed):
    with Ensemble.on_graph(Graph.imp3d(4, seed), "gossip", [seed], 5000) as a, Ensemble(64, "Imp3D", "gossip", [seed], 5000) as b:
        (ra,), (rb,) = a.run(), b.run()
        assert (ra.rounds, ra.converged, ra.seed_node, ra.status) == (rb.rounds, rb.converged, rb.seed_node, rb.status)
        assert np.array_equal(a.state(0)["c"], b.state(0)["c"]) and np.array_equal(a.state(0)["flags"], b.state(0)["flags"])


# ---- against the reference, at the shapes where the kernels can go wrong -----------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_members_match_the_reference(name, alg):
    g, cap, seeds = graph_of(name, alg), CASES[name][1], CASES[name][2]
    with Ensemble.on_graph(g, alg, seeds, cap) as e:
        e.run()
        for m, seed in enumerate(seeds):
            assert_member(e, m, ref_run(name, alg, seed), f"{name} {alg} seed {seed}")


def test_what_the_cases_are_about():
    """From the reference alone: the cases reach what they are named for."""
    for alg in ALGS:
        assert ensemble_graph_lds_bytes(graph_of("fullest64", alg), alg) == ENS_LDS_MAX
        for seed in CASES["two_components"][2]:
            sim = ref_run("two_components", alg, seed)
            assert sim.status == (CONVERGED if alg == "gossip" else MAX_ROUNDS)
    # ring1025: activity on both sides of the slot edge within the 60 rounds
    b = boundaries("push-sum", 1025)[0]
    sim = ref_run("ring1025", "push-sum", CASES["ring1025"][2][1])
    assert b == 576 and any(sim.active[:b]) and any(sim.active[b:]) and sim.round == 60
    sim = ref_run("ring1025", "gossip", CASES["ring1025"][2][0])
    assert sim.c[1024] > 0 and sim.round == 60
    assert graph_ref.in_lists(graph_of("cycle40", "gossip"))[0] == [39] and list(graph_of("cycle40", "gossip").neighbors(0)) == [1]
    assert len(graph_ref.in_lists(graph_of("star65", "gossip"))[0]) == 64


# ---- launch splitting --------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_split_launches_equal_one_run(alg):
    g, seeds = Graph.watts_strogatz(128, 4, 0.2, 11), (1, 2, HIGH)
    with Ensemble.on_graph(g, alg, seeds, 2000, trace=Trace(2)) as a, Ensemble.on_graph(g, alg, seeds, 2000, trace=Trace(2)) as b:
        a.step(3)
        assert [r.rounds for r in a.members()] == [3, 3, 3]
        a.step(5)
        ra, rb = a.run(), b.run()  # (the adjacency is staged again at every launch)
        for m in range(3):
            assert (ra[m].rounds, ra[m].converged, ra[m].status) == (rb[m].rounds, rb[m].converged, rb[m].status)
            assert all(np.array_equal(raw(a.state(m)[k]), raw(b.state(m)[k])) for k in ("c", "s", "w", "flags"))
            assert a.trace(m).tobytes() == b.trace(m).tobytes()


# ---- variants on a small world -----------------------------------------------------------------
WS_SEEDS = (3, HIGH)
FAULTS = (0.1, 0.05, 5)
MEAN = 7.3  # supplied, not the data's


def data(P):
    """Admissible values and weights with no structure in the ids."""
    rs = np.random.RandomState(5)
    return tuple((rs.random_sample(P) * 100.0 + 1.0).tolist()), tuple((rs.random_sample(P) * 3.0 + 0.5).tolist())


CASES["ws128"] = (lambda alg: Graph.watts_strogatz(128, 4, 0.2, 11), 500, WS_SEEDS)


def ws_ensemble(alg, faults=None, trace=None, values=False):
    g = graph_of("ws128", alg)
    x, w = data(128)
    return Ensemble.on_graph(g, alg, WS_SEEDS, 500, faults=None if faults is None else Faults(*faults), trace=trace,
                             values=Values(x, w, mean=MEAN) if values else None)


@pytest.mark.parametrize("alg", ALGS)
def test_faults_match_the_reference(alg):
    with ws_ensemble(alg, FAULTS) as e:
        e.run()
        stats = e.fault_stats()
        for m, seed in enumerate(WS_SEEDS):
            sim = ref_run("ws128", alg, seed, FAULTS)
            assert_member(e, m, sim, f"faults {alg} seed {seed}")
            assert (stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost) == sim.stats()
            assert sim.doomed > 0 and sim.lost > 0


@pytest.mark.parametrize("alg", ALGS)
def test_trace_rows_match_the_reference(alg):
    with ws_ensemble(alg, trace=Trace(1)) as e:
        e.run()
        for m, seed in enumerate(WS_SEEDS):
            rows, rounds, alerts, _ = graph_ref.trace_rows(GraphSim(graph_of("ws128", alg), alg, seed, max_rounds=500))
            assert (e.members()[m].rounds, e.members()[m].converged) == (rounds, alerts)
            trace_ref.assert_rows_equal(e.trace(m), rows, f"trace {alg} seed {seed}")
            assert_member(e, m, ref_run("ws128", alg, seed), f"traced {alg} seed {seed}")


def test_values_match_the_reference():
    with ws_ensemble("push-sum", values=True) as e:
        e.run()
        for m, seed in enumerate(WS_SEEDS):
            sim = ref_run("ws128", "push-sum", seed, None, True)
            assert_member(e, m, sim, f"values seed {seed}")
            ref = V.ref_summary(sim.state(), 0, 128, sim.round, sim.seed_node, 0.5, MEAN)
            summary_ref.assert_exact(e.summary(0.5)[m], ref, f"values seed {seed}")


def test_faults_trace_and_values_together():
    with ws_ensemble("push-sum", FAULTS, Trace(3), True) as e:
        e.run()
        stats = e.fault_stats()
        x, w = data(128)
        for m, seed in enumerate(WS_SEEDS):
            sim = ref_run("ws128", "push-sum", seed, FAULTS, True)
            assert_member(e, m, sim, f"all three seed {seed}")
            assert (stats[m].doomed, stats[m].down, stats[m].threshold, stats[m].lost) == sim.stats()
            fresh = GraphSim(graph_of("ws128", "push-sum"), "push-sum", seed, *FAULTS, max_rounds=500, x=x, w=w, mean=MEAN)
            rows, rounds, alerts, _ = graph_ref.trace_rows(fresh, 3)
            assert (rounds, alerts) == (sim.round, sim.alerts_total)
            trace_ref.assert_rows_equal(e.trace(m), rows, f"all three seed {seed}")


@pytest.mark.parametrize("alg", ALGS)
def test_zero_rates_are_the_plain_graph_ensemble(alg):
    with ws_ensemble(alg) as plain, ws_ensemble(alg, (0.0, 0.0, 0), Trace(1)) as other:
        rp, ro = plain.run(), other.run()
        for m in range(len(WS_SEEDS)):
            assert (rp[m].rounds, rp[m].converged, rp[m].seed_node, rp[m].status) == \
                   (ro[m].rounds, ro[m].converged, ro[m].seed_node, ro[m].status)
            assert all(np.array_equal(raw(plain.state(m)[k]), raw(other.state(m)[k])) for k in ("c", "s", "w", "flags"))
        assert [s.lost for s in other.fault_stats()] == [0, 0]


# ---- summary -----------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_summary_equals_the_reference_on_the_read_back_state(alg):
    with ws_ensemble(alg) as e:
        e.step(20)
        for when in ("after 20 rounds", "at the end"):
            sums = e.summary(0.5)
            for m, rec in enumerate(e.members()):
                ref = summary_ref.ref_summary(e.state(m), 0, 128, rec.rounds, ALGS.index(alg), rec.seed_node, 0.5)
                summary_ref.assert_matches(sums[m], ref, f"{alg} member {m} {when}")  # (mean: (P - 1) / 2)
            e.run()
