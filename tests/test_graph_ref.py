"""CPU: the pure-Python SRS v1-G (tests/graph_ref.py) and the Graph constructors.

With the reference's own neighbour lists handed over as a graph, v1-G must be v1: gossip on
Graph.lattice3d(g) is oracle/srs_py.py's 3D run, on Graph.imp3d(g, seed) its Imp3D run of that seed
(same draws: the pick is nb(i)[U(deg i)] either way, and the injector runs over the same list).
Push-sum differs by design (v1 folds lattice messages in slot order, v1-G all by sender id) and is
held to what it must conserve instead.
"""
import math

import numpy as np
import pytest

from gossipprotocol_amd import Graph
from oracle.srs_py import PySim, build_neighbours
from tests.graph_ref import GraphSim

CONVERGED, MAX_ROUNDS = 0, 1


def lists(G):
    return [[int(t) for t in G.neighbors(i)] for i in range(G.num_nodes)]


@pytest.mark.parametrize("g", (3, 4))
@pytest.mark.parametrize("seed", (1, 7))
def test_lattice3d_gossip_is_the_3d_run(g, seed):
    G = Graph.lattice3d(g)
    assert lists(G) == build_neighbours(g ** 3, g, "3D", seed)[0]
    ref, sim = PySim(g ** 3, "3D", "gossip", seed), GraphSim(G, "gossip", seed, max_rounds=5000)
    want = ref.step(5000)
    assert sim.step(5000) == want and sim.round == ref.round and sim.c == ref.c
    assert sim.seed_node == ref.seed_node and sim.status == CONVERGED


@pytest.mark.parametrize("seed", (1, 2, (5 << 32) | 9))
def test_imp3d_gossip_is_the_imp3d_run_of_that_seed(seed):
    G = Graph.imp3d(4, seed)
    assert lists(G) == build_neighbours(64, 4, "Imp3D", seed)[0]
    ref, sim = PySim(64, "Imp3D", "gossip", seed), GraphSim(G, "gossip", seed, max_rounds=5000)
    want = ref.step(5000)
    assert sim.step(5000) == want and sim.c == ref.c


def test_pushsum_conserves_mass_on_a_ring():
    sim = GraphSim(Graph.ring(33, 2), "push-sum", 3, max_rounds=300)
    s0, w0 = math.fsum(sim.s), math.fsum(sim.w)
    for _ in range(300):
        if not sim.step(1):
            break
        # halving is exact and every half arrives: the sums move by rounding only
        assert abs(math.fsum(sim.s) - s0) <= 1e-9 * s0 and abs(math.fsum(sim.w) - w0) <= 1e-9 * w0
    assert sim.round > 10 and all(sim.active)


def two_components():
    """Two directed triangles with no edge between them."""
    return Graph.from_edges(6, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)], directed=True)


def test_two_components_pushsum_ends_at_max_rounds():
    sim = GraphSim(two_components(), "push-sum", 1, max_rounds=200).run()
    assert sim.status == MAX_ROUNDS and sim.round == 200
    other = [i for i in range(6) if i // 3 != sim.seed_node // 3]
    assert not any(sim.active[i] for i in other) and all(sim.s[i] == float(i) and sim.w[i] == 1.0 for i in other)


def test_two_components_gossip_converges_through_the_injector():
    sim = GraphSim(two_components(), "gossip", 1, max_rounds=5000).run()
    assert sim.status == CONVERGED and sim.alerts_total == 6 and min(sim.c) >= 11


def test_self_loop_and_duplicates():
    G = Graph.from_edges(3, [(0, 0), (0, 1), (0, 1), (1, 2), (2, 0)], directed=True)
    assert lists(G) == [[0, 1, 1], [2], [0]]
    sim = GraphSim(G, "push-sum", 4, max_rounds=50).run()
    assert abs(math.fsum(sim.s) - 3.0) < 1e-12 and abs(math.fsum(sim.w) - 3.0) < 1e-12


def test_constructors():
    assert lists(Graph.ring(5, 2)) == [[4, 1], [0, 2], [1, 3], [2, 4], [3, 0]]
    assert lists(Graph.ring(6, 4))[0] == [5, 1, 4, 2]
    assert lists(Graph.star(4)) == [[1, 2, 3], [0], [0], [0]]
    assert lists(Graph.torus(3, 3))[4] == [3, 5, 1, 7] and lists(Graph.torus(3, 3))[0] == [2, 1, 6, 3]
    assert lists(Graph.from_edges(3, [(0, 1), (2, 1), (1, 1)])) == [[1], [0, 2, 1], [1]]
    G = Graph.ring(8, 2)
    assert (G.num_nodes, G.num_edges) == (8, 16) and G.indptr.dtype == np.int64 and G.indices.dtype == np.uint32
    with pytest.raises(ValueError):
        Graph.ring(4, 4)
    with pytest.raises(ValueError):
        Graph.from_edges(3, [(0, 3)])


def test_watts_strogatz_is_deterministic_undirected_and_keeps_its_edge_count():
    a, b = Graph.watts_strogatz(128, 4, 0.2, 5), Graph.watts_strogatz(128, 4, 0.2, 5)
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert not np.array_equal(a.indices, Graph.watts_strogatz(128, 4, 0.2, 6).indices)
    L = lists(a)
    assert a.num_edges == 128 * 4 and all(i in L[t] and t != i for i in range(128) for t in L[i])
    assert all(x == sorted(set(x)) for x in L)
    assert lists(Graph.watts_strogatz(16, 4, 0.0, 1)) == [sorted(x) for x in lists(Graph.ring(16, 4))]
    assert lists(a) != [sorted(x) for x in lists(Graph.ring(128, 4))]
