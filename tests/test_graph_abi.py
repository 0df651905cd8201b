"""CPU: the C-ABI of ensembles over a caller-supplied graph (SRS v1-G).

No GPU: the symbols, the struct, the host-side admissibility check through the size query (every
rule refused with its node and its words), GP_GRAPH refused by every entry point that existed
before it, and the LDS image against its Python restatement (tests/graph_ref.py), at the largest
graph that fits and one entry beyond it.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gossipprotocol_amd import TOPOLOGIES, Ensemble, Graph, ensemble_graph_lds_bytes
from gossipprotocol_amd import _lib as L
from tests import graph_ref
from tests.ensemble_shape_ref import ENS_LDS_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(f, t) for f in (False, True) for t in (False, True)]
ALGS = ("gossip", "push-sum")


def test_symbols_and_constants():
    lib = C.CDLL(L.LIB_PATH)
    bound = {n for n, _, _ in L.SIGNATURES}
    for n in ("gp_ensemble_create_graph", "gp_ensemble_graph_lds_bytes"):
        assert hasattr(lib, n) and n in bound
    assert L.GP_GRAPH == 4 and TOPOLOGIES == ("line", "full", "3D", "Imp3D")


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(gp_graph), offsetof(gp_graph, indices),'
                   'offsetof(gp_graph, num_nodes), offsetof(gp_graph, num_edges), offsetof(gp_graph, reserved), GP_GRAPH);'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    G = L.GpGraph
    assert got == [C.sizeof(G), G.indices.offset, G.num_nodes.offset, G.num_edges.offset, G.reserved.offset, L.GP_GRAPH]


def refusal(graph, alg="gossip"):
    with pytest.raises(L.GossipError) as e:
        ensemble_graph_lds_bytes(graph, alg)
    assert e.value.code == -1
    return str(e.value)


def triangle():
    return Graph([0, 2, 3, 5], [1, 2, 2, 0, 1])


@pytest.mark.parametrize("edit,words", [
    (lambda g: g.indptr.__setitem__(0, 1), "node 0: indptr[0] must be 0"),
    (lambda g: g.indptr.__setitem__(2, 1), "node 1: indptr decreases"),
    (lambda g: g.indptr.__setitem__(3, 4), "node 2: indptr[P] = 4 must be num_edges 5"),
    (lambda g: g.indptr.__setitem__(2, 2), "node 1: degree 0"),
    (lambda g: g.indices.__setitem__(2, 3), "node 1: neighbour index 3 is not below num_nodes 3"),
])
def test_every_rule_is_refused_with_its_node(edit, words):
    g = triangle()
    assert ensemble_graph_lds_bytes(g, "gossip") > 0
    edit(g)
    assert words in refusal(g) and words in refusal(g, "push-sum")


def test_indptr_beyond_the_indices_is_refused():
    g = Graph([0, 2, 3, 9], [1, 2, 2, 0, 1])  # indptr[P] != E, and past the array
    assert "node 2: indptr[3] = 9 exceeds num_edges 5" in refusal(g)


def test_the_lowest_node_and_its_first_rule_are_named():
    g = triangle()
    g.indices[0] = 7
    g.indptr[2] = 2
    assert "node 0: neighbour index 7" in refusal(g)


def test_population_limits():
    assert "num_nodes 1 outside [2, 8192]" in refusal(Graph([0, 1], [0]))
    assert "num_nodes 8193 outside [2, 8192]" in refusal(Graph.ring(8193, 2))
    assert ensemble_graph_lds_bytes(Graph.ring(8192, 2), "gossip") > 0
    assert ensemble_graph_lds_bytes(Graph([0, 1, 2], [1, 0]), "push-sum") > 0  # P = 2, one edge each way


def test_unknown_algorithm_and_null_graph():
    lib = L.lib()
    g = triangle()
    from gossipprotocol_amd.sim import _gp_graph
    assert lib.gp_ensemble_graph_lds_bytes(C.byref(_gp_graph(g)), 2, 0, 0) == -1
    assert b"unknown algorithm" in lib.gp_last_error()
    assert lib.gp_ensemble_graph_lds_bytes(None, 0, 0, 0) == -1
    bad = _gp_graph(g)
    bad.reserved = 1
    assert lib.gp_ensemble_graph_lds_bytes(C.byref(bad), 0, 0, 0) == -1 and b"reserved" in lib.gp_last_error()


def test_gp_graph_is_refused_by_every_earlier_entry_point():
    lib = L.lib()
    P, T, g = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.gp_resolve(100, L.GP_GRAPH, C.byref(P), C.byref(T), C.byref(g)) == -1
    assert b"unknown topology id 4" in lib.gp_last_error()
    for name in (b"graph", b"Graph", b"GRAPH", b"4"):
        assert lib.gp_parse_topology(name) == -1
    for alg in (0, 1):
        assert lib.gp_ensemble_max_nodes(L.GP_GRAPH, alg) == -1
        assert lib.gp_ensemble_faults_max_nodes(L.GP_GRAPH, alg) == -1
        assert lib.gp_ensemble_trace_max_nodes(L.GP_GRAPH, alg, 0) == -1
        assert b"unknown topology id 4" in lib.gp_last_error()
    cfg = L.GpConfig()
    cfg.num_nodes, cfg.topology, cfg.algorithm, cfg.num_gpus, cfg.max_rounds = 100, L.GP_GRAPH, 1, 1, 100
    h = C.c_void_p()
    assert lib.gp_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    seeds = (C.c_uint64 * 1)(1)
    f, t = L.GpFaults(0.0, 0.0, 0, 0), L.GpTraceCfg(1, 0)
    x = (C.c_double * 100)(*range(100))
    v = L.GpValues(x, None, 100, 49.5, 0)
    for rc in (lib.gp_ensemble_create(C.byref(cfg), seeds, 1, C.byref(h)),
               lib.gp_ensemble_create_faults(C.byref(cfg), C.byref(f), seeds, 1, C.byref(h)),
               lib.gp_ensemble_create_traced(C.byref(cfg), None, C.byref(t), seeds, 1, C.byref(h)),
               lib.gp_ensemble_create_values(C.byref(cfg), C.byref(v), None, None, seeds, 1, C.byref(h))):
        assert rc == -1 and not h.value
        assert b"unknown topology id 4" in lib.gp_last_error()


def create(graph, alg="gossip", num_nodes=None, topology=L.GP_GRAPH, values=None, faults=None):
    """gp_ensemble_create_graph, expected to be refused before any device is touched."""
    from gossipprotocol_amd.sim import _gp_graph
    lib = L.lib()
    cfg = L.GpConfig()
    cfg.num_nodes = graph.num_nodes if num_nodes is None else num_nodes
    cfg.topology, cfg.algorithm, cfg.num_gpus, cfg.max_rounds = topology, ALGS.index(alg), 1, 100
    h = C.c_void_p()
    seeds = (C.c_uint64 * 1)(1)
    rc = lib.gp_ensemble_create_graph(C.byref(cfg), C.byref(_gp_graph(graph)) if graph is not None else None,
                                      None if values is None else C.byref(values),
                                      None if faults is None else C.byref(faults), None, seeds, 1, C.byref(h))
    assert not h.value or rc == 0
    if h.value:
        lib.gp_ensemble_destroy(h)
    return rc, lib.gp_last_error().decode()


def test_create_graph_refusals():
    g = triangle()
    rc, msg = create(g, num_nodes=4)
    assert rc == -1 and "cfg.num_nodes 4 is not the graph's num_nodes 3" in msg
    rc, msg = create(g, topology=L.GP_3D)
    assert rc == -1 and "cfg.topology must be GP_GRAPH" in msg
    bad = triangle()
    bad.indptr[2] = 2
    rc, msg = create(bad)
    assert rc == -1 and "node 1: degree 0" in msg
    x = (C.c_double * 3)(1.0, 2.0, 3.0)
    rc, msg = create(g, "gossip", values=L.GpValues(x, None, 3, 2.0, 0))
    assert rc == -1 and "gossip has no values" in msg
    rc, msg = create(g, "push-sum", values=L.GpValues(x, None, 4, 2.0, 0))
    assert rc == -1 and "count 4 is not the population 3" in msg
    rc, msg = create(g, faults=L.GpFaults(1.5, 0.0, 0, 0))
    assert rc == -1 and "node_fail must be in [0, 1]" in msg
    lib = L.lib()
    cfg = L.GpConfig()
    assert lib.gp_ensemble_create_graph(C.byref(cfg), None, None, None, None, None, 0, C.byref(C.c_void_p())) == -1
    assert b"graph is null" in lib.gp_last_error()
    with pytest.raises(L.GossipError, match="degree 0"):
        Ensemble.on_graph(bad, "gossip", [1], 100)


GRAPHS = {"ring(33, 2)": lambda: Graph.ring(33, 2), "star(65)": lambda: Graph.star(65),
          "cycle(40)": lambda: Graph.from_edges(40, [(i, (i + 1) % 40) for i in range(40)], directed=True),
          "ws(128, 4)": lambda: Graph.watts_strogatz(128, 4, 0.2, 3), "imp3d(4)": lambda: Graph.imp3d(4, 1),
          "loops": lambda: Graph.from_edges(4, [(0, 3), (0, 0), (0, 3), (0, 1), (1, 1), (1, 1), (2, 0), (2, 3), (2, 0),
                                                (3, 2)], directed=True),
          "ring(1000, 16)": lambda: Graph.ring(1000, 16)}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_size_query_equals_the_restatement(name):
    g = GRAPHS[name]()
    for alg in ALGS:
        for f, t in VARIANTS:
            assert ensemble_graph_lds_bytes(g, alg, f, t) == graph_ref.graph_lds_bytes(g, alg, f, t), (alg, f, t)
    # the in-list is deduplicated and the variants add what they add for the built-in topologies
    if name == "loops":
        assert g.num_edges == 10 and sum(len(a) for a in graph_ref.in_lists(g)) == 7


def test_condition_of_the_issue_degree_16_at_1000_nodes():
    for alg in ALGS:
        for f, t in VARIANTS:
            assert graph_ref.lds_bytes(alg, 1000, 16000, 16000, f, t) <= ENS_LDS_MAX
    assert ensemble_graph_lds_bytes(Graph.ring(1000, 16), "push-sum", True, True) == \
        graph_ref.lds_bytes("push-sum", 1000, 16000, 16000, True, True)


def fullest(P, alg, f, t):
    """A graph on P nodes with the most out-entries whose image fits: every node lists its successor
    on the ring (so the in-CSR has P entries whatever follows), and node 0 lists it again and again."""
    def size(extra):
        return graph_ref.lds_bytes(alg, P, P + extra, P, f, t)
    extra = 0
    while size(extra + 1) <= ENS_LDS_MAX:
        extra += 4096 if size(extra + 4096) <= ENS_LDS_MAX else 1
    lists = [[(i + 1) % P] for i in range(P)]
    lists[0] += [1] * extra
    return Graph._from_lists(lists), extra


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("f,t", VARIANTS)
def test_largest_graph_that_fits_and_one_entry_more(alg, f, t):
    g, extra = fullest(64, alg, f, t)
    got = ensemble_graph_lds_bytes(g, alg, f, t)
    # (every array is padded to 8 bytes and the budget is a multiple of 8: the fullest image fills it)
    assert got == graph_ref.graph_lds_bytes(g, alg, f, t) == ENS_LDS_MAX
    lists = [list(g.neighbors(i)) for i in range(64)]
    lists[0].append(1)  # one more entry
    big = Graph._from_lists(lists)
    assert big.num_edges == g.num_edges + 1 == 64 + extra + 1
    with pytest.raises(L.GossipError) as e:
        ensemble_graph_lds_bytes(big, alg, f, t)
    need = graph_ref.graph_lds_bytes(big, alg, f, t)
    assert need == ENS_LDS_MAX + 8 and f"takes {need} bytes" in str(e.value)


def test_graph_class():
    g = Graph([0, 2, 3, 5], np.array([1, 2, 2, 0, 1], np.int16))
    assert (g.num_nodes, g.num_edges) == (3, 5) and list(g.neighbors(2)) == [0, 1]
    assert g.indptr.dtype == np.int64 and g.indices.dtype == np.uint32
