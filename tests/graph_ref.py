"""Pure-Python SRS v1-G: gossip and push-sum over a caller-supplied graph.

TEST INFRASTRUCTURE: the one definition of the graph semantics outside the kernels
(gp_ensemble_kernels.hpp, TOPO == GRAPH); tests compare the GPU with it bit for bit, and
tools/graph_ensemble.py --backend ref runs through it.  GraphSim is tests/faults_ref.py's FaultSim
(itself a mirror of oracle/srs_py.py's PySim) with the neighbour lists given instead of built:
P = T = the graph's nodes, nlat = 0 everywhere (so push-sum folds every message by ascending sender
id), the injector on.  Rounds, failure model, flags and stats are inherited, so faults come for
free; values replace the initial (s, w) as tests/values_ref.py's ValueSim does; trace_rows() and
ref_summary() are that module's, which take any simulator with this interface.
Loops are pure Python: keep P x rounds below ~1e5.
"""
from __future__ import annotations

import numpy as np

from oracle.srs_py import STREAM_START, uniform
from tests import values_ref
from tests.faults_ref import FaultSim, draw_x, threshold, STREAM_FAULT_NODE


def in_lists(graph):
    """The transposed graph, senders ascending and each once: what the push-sum kernel walks."""
    indptr, indices = np.asarray(graph.indptr), np.asarray(graph.indices)
    inl = [set() for _ in range(graph.num_nodes)]
    for i in range(graph.num_nodes):
        for t in indices[indptr[i]:indptr[i + 1]]:
            inl[int(t)].add(i)
    return [sorted(a) for a in inl]


def lds_bytes(alg, P, e_out, e_in, faults=False, trace=False):
    """Restatement of ens_graph_lds_bytes (gp_ensemble_shape.hpp), after tests/ensemble_shape_ref.py:
    header; gossip c, inc, live bitmap / push-sum hs, hw, tgt; doomed bitmap; trace block; out-CSR
    (u32 offsets, u16 ids); push-sum: in-CSR.  Every array padded to 8 bytes."""
    from tests.ensemble_shape_ref import ENS_LDS_HDR, ENS_LDS_TRACE, up8

    words = up8(4 * ((P + 31) // 32))
    b = ENS_LDS_HDR
    b += 2 * up8(4 * P) + words if alg == "gossip" else 16 * P + up8(2 * P)
    b += words if faults else 0
    b += ENS_LDS_TRACE if trace else 0
    b += up8(4 * (P + 1)) + up8(2 * e_out)
    if alg != "gossip":
        b += up8(4 * (P + 1)) + up8(2 * e_in)
    return b


def graph_lds_bytes(graph, alg, faults=False, trace=False):
    return lds_bytes(alg, graph.num_nodes, graph.num_edges, sum(len(a) for a in in_lists(graph)), faults, trace)


def fullest_graph(P, alg, faults=False, trace=False, seed=1):
    """(indptr, indices) of a graph on P nodes at the largest entry count whose image fits: every node
    lists every node (itself included, so the in-CSR has its P * P entries whatever follows), then
    duplicates, dealt round-robin over the nodes with targets from numpy.random.RandomState(seed),
    until one more entry would not fit."""
    from tests.ensemble_shape_ref import ENS_LDS_MAX

    extra = 0
    while lds_bytes(alg, P, P * P + extra + 1, P * P, faults, trace) <= ENS_LDS_MAX:
        extra += 1024 if lds_bytes(alg, P, P * P + extra + 1024, P * P, faults, trace) <= ENS_LDS_MAX else 1
    tg = np.random.RandomState(seed).randint(0, P, extra)
    lists = [list(range(P)) + [int(t) for t in tg[i::P]] for i in range(P)]
    indptr = np.concatenate(([0], np.cumsum([len(a) for a in lists]))).astype(np.int64)
    return indptr, np.concatenate(lists).astype(np.uint32)


class GraphSim(FaultSim):
    """FaultSim (no faults by default) on `graph` (anything with indptr / indices / num_nodes)."""

    def __init__(self, graph, algorithm, seed=1, node_fail=0.0, msg_drop=0.0, fail_round=0, max_rounds=400, x=None,
                 w=None, mean=None):
        if fail_round < 0:
            raise ValueError(fail_round)
        P = int(graph.num_nodes)
        indptr, indices = np.asarray(graph.indptr), np.asarray(graph.indices)
        self.topology, self.algorithm, self.seed = "graph", algorithm, seed
        self.P, self.T, self.g = P, P, 0  # v1-G: no extra actor
        self.nbrs = [[int(t) for t in indices[indptr[i]:indptr[i + 1]]] for i in range(P)]  # v1-G: given
        self.nlat = [0] * P  # v1-G: no lattice slots, every message folds by ascending sender id
        assert P >= 2 and all(len(a) >= 1 and max(a) < P for a in self.nbrs)
        self.seed_node = uniform(seed, STREAM_START, 0, 0, self.T)
        self.round = 0
        self.alerts_total = 0
        self.alerts = []
        self.max_rounds = max_rounds
        self.q_node, self.q_drop, self.fail_round = threshold(node_fail), threshold(msg_drop), fail_round
        self.D = [i != self.seed_node and draw_x(seed, STREAM_FAULT_NODE, i, 0) < self.q_node for i in range(P)]
        self.doomed = sum(self.D)
        self.threshold = max(1, self.T - self.doomed)
        self.lost = 0
        self.mean = (P - 1) * 0.5
        if algorithm == "gossip":
            assert x is None and w is None
            self.c = [0] * P
            self.live = list(range(self.T))  # v1-G: the injector runs, L = {0..T-1}
        else:
            self.s = [float(i) for i in range(P)]
            self.w = [1.0] * P
            self.cnt = [1] * P
            self.conv = [False] * P
            self.active = [False] * P
            self.active[self.seed_node] = True
            if x is not None:  # v1-V
                assert len(x) == P and (w is None or len(w) == P) and not values_ref.first_offender(x, w)
                self.s = [float(v) for v in x]
                if w is not None:
                    self.w = [float(v) for v in w]
                self.mean = values_ref.default_mean(x, w) if mean is None else float(mean)

    def state(self):
        z = np.zeros(self.P)
        if self.algorithm == "gossip":
            return {"c": np.array(self.c, np.int32), "s": z, "w": z.copy(), "flags": np.array(self.flags(), np.uint8)}
        return {"c": np.zeros(self.P, np.int32), "s": np.array(self.s, np.float64), "w": np.array(self.w, np.float64),
                "flags": np.array(self.flags(), np.uint8)}


def trace_rows(sim, stride=1, capacity=0):
    """The rows a traced member on the graph records, from a fresh GraphSim run to its end
    (tests/trace_ref.py's loop, the one definition of a row).  Returns (rows, rounds, alerts, stats)."""
    from tests import trace_ref

    if sim.algorithm == "push-sum":
        return values_ref.trace_rows(sim, stride, capacity)
    saved = trace_ref.FaultSim
    trace_ref.FaultSim = lambda *a, **k: sim
    try:
        return trace_ref.trace.__wrapped__(0, "graph", "gossip", sim.seed, stride, capacity, sim.max_rounds, (0.0, 0.0, 0))
    finally:
        trace_ref.FaultSim = saved
