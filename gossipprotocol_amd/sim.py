"""Host-side mirror of the reference's entry point over the C-ABI.

The reference's only interface to the hot path is ``main`` in
/root/reference/Project2/Program.fs (Program.fs:31-283): parse
``num_nodes topology algorithm`` (Program.fs:32-34), build actors and topology
(Program.fs:169-261), start the seed (Program.fs:193-205), wait for the
scheduler's ``nodes`` alerts (Program.fs:41-61).  :class:`Simulation` exposes
the same steps -- create / run -- plus round stepping and state readback for
tests.  Every call goes to libgossip_hip.so; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib as L
from .graph import Graph

TOPOLOGIES = ("line", "full", "3D", "Imp3D")
ALGORITHMS = ("gossip", "push-sum")


def parse_topology(name: str) -> int:
    """Case-sensitive like Program.fs:180,209,238; 'imp3D' accepted as an alias."""
    return L.check(L.lib().gp_parse_topology(name.encode()))


def parse_algorithm(name: str) -> int:
    return L.check(L.lib().gp_parse_algorithm(name.encode()))


def resolve(num_nodes: int, topology: str):
    """(P, T, g) -- population, alert threshold, grid edge (Program.fs:170-171,53,239-240)."""
    P, T, g = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(L.lib().gp_resolve(num_nodes, parse_topology(topology), C.byref(P), C.byref(T), C.byref(g)))
    return P.value, T.value, g.value


def default_mean(x, w=None) -> float:
    """The default mu of a value run: math.fsum(x) / math.fsum(w), or math.fsum(x) / len(x) without
    weights -- the correctly rounded sums, one division."""
    return math.fsum(x) / (math.fsum(w) if w is not None else len(x))


def _f64(a):
    """A contiguous float64 copy-or-view of `a` and its ctypes pointer."""
    arr = np.ascontiguousarray(a, np.float64)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_double))


class Simulation:
    """One simulated network on one MI355X (handle over gp_sim)."""

    def __init__(self, num_nodes: int, topology: str, algorithm: str, seed: int = 1,
                 max_rounds: int = 0, device: int = 0, kernel_timing: bool = False,
                 rank: int = 0, world: int = 1, dist=None, virtual_ranks: int = 1, experimental: bool = False,
                 rendezvous: str | None = None, rendezvous_timeout_ms: int = 600000):
        """world > 1: this process is rank `rank` of a one-process-per-GPU run
        (RCCL; rank 0's RCCL id is shared once, through `dist` -- a
        torch.distributed group -- or through the file `rendezvous`
        (gp_rendezvous_id; gossipprotocol_amd.launch sets GOSSIP_RDV)).  virtual_ranks > 1: that many slabs in this process on `device`,
        exchanging through device copies (the multi-GPU path on one GPU).
        experimental: use the experiments build (kernel variants selected by
        GP_* environment variables; tests and tools only)."""
        self._L = L.lib(experimental)
        cfg = L.GpConfig()
        cfg.num_nodes = num_nodes
        cfg.topology = parse_topology(topology)
        cfg.algorithm = parse_algorithm(algorithm)
        cfg.seed = seed
        cfg.num_gpus = max(1, virtual_ranks)
        cfg.device = device
        cfg.max_rounds = max_rounds
        cfg.flags = (L.GP_FLAG_KERNEL_TIMING if kernel_timing else 0) | \
            (L.GP_FLAG_VIRTUAL_RANKS if virtual_ranks > 1 else 0)
        self.topology, self.algorithm = topology, algorithm
        h = C.c_void_p()
        if world > 1 or (world == 1 and dist is not None and experimental and os.environ.get("GP_FORCE_RCCL") == "1"):
            # one process per GPU: rank 0 makes the RCCL id, the caller's process
            # group (gloo is enough) broadcasts it, every rank joins its slab
            uid = C.create_string_buffer(128)
            if dist is None and rendezvous:
                self._chk(self._L.gp_rendezvous_id(rank, rendezvous.encode(), rendezvous_timeout_ms, uid))
            elif dist is None:
                raise ValueError("world > 1 needs a torch.distributed group or a rendezvous path to share the RCCL id")
            else:
                if rank == 0:
                    self._chk(self._L.gp_get_unique_id(uid))
                box = [uid.raw if rank == 0 else None]
                dist.broadcast_object_list(box, src=0)
                uid = C.create_string_buffer(box[0], 128)
            from .launch import stdout_to_stderr
            with stdout_to_stderr():  # (RCCL's version line)
                rc = self._L.gp_create_rank(C.byref(cfg), rank, world, uid, C.byref(h))
            self._chk(rc)
        else:
            self._chk(self._L.gp_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def _chk(self, rc):
        return L.check(rc, self._L)

    # -- lifecycle -------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.gp_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    # -- the hot path ----------------------------------------------------
    def step(self, nrounds: int):
        """Run up to nrounds synchronous rounds; returns the per-round alert counts."""
        buf = (C.c_int64 * max(1, nrounds))()
        n = self._chk(self._L.gp_step(self._h, nrounds, buf))
        return [buf[i] for i in range(n)]

    def run(self) -> L.GpResult:
        """Run to convergence (or max_rounds): the reference's whole propagation."""
        res = L.GpResult()
        self._chk(self._L.gp_run(self._h, C.byref(res)))
        return res

    def sync(self):
        self._chk(self._L.gp_sync(self._h))

    # -- caller-supplied data (SRS v1-V) -------------
    def set_values(self, x, w=None, first: int = 0, mean: float | None = None):
        """Push-sum over your data: node first + k starts from s = x[k], w = w[k] (all 1 without
        `w`) instead of s = id, w = 1 (gp_set_values).  Before the first round only; may be called
        repeatedly to load a large network in chunks, each call all or nothing.  Entries must be
        admissible (include/gossip_hip.h: non-negative, finite, weights in [2^-32, 2^32], x = 0 or
        >= 2^-64, x / w < 2^32); shift negative data first.  `mean` sets mu, what the summary's
        error fields are measured against; mean=None with first == 0 and len(x) == P computes
        :func:`default_mean`, otherwise the mean is left alone (see :meth:`set_mean`)."""
        xa, xp = _f64(x)
        wa, wp = (None, None) if w is None else _f64(w)
        if wa is not None and len(wa) != len(xa):
            raise ValueError(f"{len(xa)} values but {len(wa)} weights")
        self._chk(self._L.gp_set_values(self._h, first, len(xa), xp, wp))
        if mean is None and first == 0 and len(xa) == self.population:
            mean = default_mean(xa.tolist(), None if wa is None else wa.tolist())
        if mean is not None:
            self.set_mean(mean)

    def set_mean(self, mu: float):
        """mu of the summaries (gp_set_mean): finite, >= 0, < 2^32.  Every rank of a multi-process
        run sets the same value."""
        self._chk(self._L.gp_set_mean(self._h, float(mu)))

    # -- inspection ------------------------------------------------------
    def info(self) -> L.GpInfo:
        out = L.GpInfo()
        self._chk(self._L.gp_get_info(self._h, C.byref(out)))
        return out

    @property
    def population(self):
        return self.info().population

    @property
    def local_population(self):
        """Nodes owned by this handle (its slab; all P for a single GPU)."""
        return self.info().slab_count

    @property
    def threshold(self):
        return self.info().threshold

    @property
    def seed_node(self):
        return self.info().seed_node

    @property
    def rounds(self):
        return self.info().rounds

    @property
    def alerts_total(self):
        return self.info().alerts_total

    def neighbors(self, node: int):
        deg = self._chk(self._L.gp_neighbors(self._h, node, None, 0))
        out = (C.c_int64 * max(1, deg))()
        self._chk(self._L.gp_neighbors(self._h, node, out, deg))
        return [out[k] for k in range(deg)]

    def state(self, first: int = 0, count: int | None = None):
        count = self.population - first if count is None else count
        c = np.zeros(count, np.int32)
        s = np.zeros(count, np.float64)
        w = np.zeros(count, np.float64)
        f = np.zeros(count, np.uint8)
        self._chk(self._L.gp_read_state(self._h, first, count, c.ctypes.data, s.ctypes.data,
                                      w.ctypes.data, f.ctypes.data))
        return {"c": c, "s": s, "w": w, "flags": f}

    def summary(self, tol: float = 1e-10, scope: str = "local") -> L.GpSummary:
        """What the run has computed so far, reduced on the device (gp_summary_take): counts of
        active / converged nodes, gossip's counter histogram, push-sum's estimate range, largest
        error, nodes within `tol` of the true average and the conserved sums.  scope "local":
        the ids this handle owns; "global" (every rank of a multi-process run calls it): the
        whole network.  Leaves the run untouched."""
        scopes = {"local": L.GP_SCOPE_LOCAL, "global": L.GP_SCOPE_GLOBAL}
        if scope not in scopes:
            raise ValueError(f"scope must be 'local' or 'global' (got {scope!r})")
        out = L.GpSummary()
        self._chk(self._L.gp_summary_take(self._h, tol, scopes[scope], C.byref(out)))
        return out

    def kernel_stats(self, reset: bool = False):
        ms, n = C.c_double(), C.c_int64()
        name = C.create_string_buffer(128)
        self._chk(self._L.gp_kernel_stats(self._h, C.byref(ms), C.byref(n), name, 128, int(reset)))
        return ms.value, n.value, name.value.decode()

    def alg_bytes_per_node(self) -> float:
        return self._L.gp_alg_bytes_per_node(self._h)


def ensemble_max_nodes(topology: str, algorithm: str, faults: bool = False, trace: bool = False) -> int:
    """Largest num_nodes an :class:`Ensemble` accepts for the pair (host only); faults=True:
    the cap of an ensemble with a failure model; trace=True: of one that records a trace."""
    if trace:
        return L.check(L.lib().gp_ensemble_trace_max_nodes(parse_topology(topology), parse_algorithm(algorithm),
                                                           int(bool(faults))))
    f = L.lib().gp_ensemble_faults_max_nodes if faults else L.lib().gp_ensemble_max_nodes
    return L.check(f(parse_topology(topology), parse_algorithm(algorithm)))


def _gp_graph(graph: Graph) -> "L.GpGraph":
    """The gp_graph over a :class:`Graph`'s arrays (which the Graph keeps alive)."""
    return L.GpGraph(graph.indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                     graph.indices.ctypes.data_as(C.POINTER(C.c_uint32)), graph.num_nodes, graph.num_edges, 0)


def ensemble_graph_lds_bytes(graph: Graph, algorithm: str, faults: bool = False, trace: bool = False) -> int:
    """The LDS image in bytes of one member of ``Ensemble.on_graph(graph, algorithm, ...)`` (host
    only; gp_ensemble_graph_lds_bytes).  Raises :class:`GossipError` for an inadmissible graph, one
    whose image exceeds what a member may take included; the message names the node and the rule,
    or the bytes."""
    return L.check(L.lib().gp_ensemble_graph_lds_bytes(C.byref(_gp_graph(graph)), parse_algorithm(algorithm),
                                                       int(bool(faults)), int(bool(trace))))


class Faults:
    """Failure model of an :class:`Ensemble` (gp_faults; SRS v1-F): every
    node but the seed node is doomed with probability ``node_fail`` and down -- silent, deaf,
    frozen -- from round ``fail_round`` on; every node-to-node message is lost with
    probability ``msg_drop``."""

    def __init__(self, node_fail: float = 0.0, msg_drop: float = 0.0, fail_round: int = 0):
        self.node_fail, self.msg_drop, self.fail_round = float(node_fail), float(msg_drop), int(fail_round)

    def __repr__(self):
        return f"Faults(node_fail={self.node_fail}, msg_drop={self.msg_drop}, fail_round={self.fail_round})"


class Trace:
    """Trace parameters of an :class:`Ensemble` (gp_trace_cfg; SRS v1-T): a
    member that has just completed round R records a row iff R is a multiple of ``stride`` and it
    has recorded fewer than ``capacity`` rows; capacity 0 keeps every row up to max_rounds."""

    def __init__(self, stride: int = 1, capacity: int = 0):
        self.stride, self.capacity = int(stride), int(capacity)

    def __repr__(self):
        return f"Trace(stride={self.stride}, capacity={self.capacity})"


class Values:
    """The data every member of an :class:`Ensemble` starts from (gp_values; SRS v1-V, DESIGN.md
    section 13): node i holds s = x[i], w = w[i] (all 1 without `w`); ``mean`` is mu, what the
    summaries' and the trace's errors are measured against (default: :func:`default_mean`)."""

    def __init__(self, x, w=None, mean: float | None = None):
        self.x = np.ascontiguousarray(x, np.float64)
        self.w = None if w is None else np.ascontiguousarray(w, np.float64)
        if self.w is not None and len(self.w) != len(self.x):
            raise ValueError(f"{len(self.x)} values but {len(self.w)} weights")
        self.mean = float(default_mean(self.x.tolist(), None if self.w is None else self.w.tolist())
                          if mean is None else mean)

    def __repr__(self):
        return f"Values({len(self.x)} values, {'weighted' if self.w is not None else 'unweighted'}, mean={self.mean!r})"


# one row of a trace (gp_trace_row)
TRACE_DTYPE = np.dtype([("round", "<i8"), ("reached", "<u4"), ("alerts", "<u4"), ("sent", "<u8"), ("err_max", "<f8")])


class Ensemble:
    """Many small networks at once on one MI355X, one per seed (handle over
    gp_ensemble): the regime of the reference's published curves, n = 100..1000
    (README.md, Report.pdf).  Each member is one workgroup with its state in LDS and
    is bit-identical to ``Simulation(num_nodes, topology, algorithm, seed)``.  With
    ``faults=Faults(...)`` nodes crash and messages get lost (gp_ensemble_create_faults); with
    ``trace=Trace(...)`` every member records its spread curve inside the kernel
    (gp_ensemble_create_traced), read with :meth:`trace`; with ``values=Values(...)`` every
    push-sum member averages your data instead of the node ids (gp_ensemble_create_values).  The
    three compose."""

    def __init__(self, num_nodes: int, topology: str, algorithm: str, seeds, max_rounds: int, device: int = 0,
                 faults: "Faults | None" = None, trace: "Trace | None" = None, values: "Values | None" = None):
        self._L = L.lib()
        self.seeds = [int(s) for s in seeds]
        cfg = L.GpConfig()
        cfg.num_nodes = num_nodes
        cfg.topology = parse_topology(topology)
        cfg.algorithm = parse_algorithm(algorithm)
        cfg.num_gpus = 1
        cfg.device = device
        cfg.max_rounds = max_rounds
        self.topology, self.algorithm = topology, algorithm
        self.population = resolve(num_nodes, topology)[0]
        arr = (C.c_uint64 * max(1, len(self.seeds)))(*self.seeds)
        h = C.c_void_p()
        self.faults, self.tracing = faults, trace
        f = None if faults is None else L.GpFaults(faults.node_fail, faults.msg_drop, faults.fail_round, 0)
        self.values = values
        t = None if trace is None else L.GpTraceCfg(trace.stride, trace.capacity)
        if values is not None:
            dp = C.POINTER(C.c_double)
            v = L.GpValues(values.x.ctypes.data_as(dp), None if values.w is None else values.w.ctypes.data_as(dp),
                           len(values.x), values.mean, 0)
            L.check(self._L.gp_ensemble_create_values(C.byref(cfg), C.byref(v), None if f is None else C.byref(f),
                                                      None if t is None else C.byref(t), arr, len(self.seeds),
                                                      C.byref(h)), self._L)
        elif trace is not None:
            L.check(self._L.gp_ensemble_create_traced(C.byref(cfg), None if f is None else C.byref(f), C.byref(t), arr,
                                                      len(self.seeds), C.byref(h)), self._L)
        elif faults is None:
            L.check(self._L.gp_ensemble_create(C.byref(cfg), arr, len(self.seeds), C.byref(h)), self._L)
        else:
            L.check(self._L.gp_ensemble_create_faults(C.byref(cfg), C.byref(f), arr, len(self.seeds), C.byref(h)),
                    self._L)
        self._h = h

    @classmethod
    def on_graph(cls, graph: Graph, algorithm: str, seeds, max_rounds: int, device: int = 0,
                 faults: "Faults | None" = None, trace: "Trace | None" = None, values: "Values | None" = None):
        """An ensemble on your own network (gp_ensemble_create_graph; SRS v1-G):
        every member runs on ``graph``, a :class:`Graph`, with P = T = ``graph.num_nodes``.  Faults,
        trace and values compose as in the constructor, and every method works on the result; its
        ``topology`` reads "graph"."""
        self = cls.__new__(cls)
        self._L = L.lib()
        self.seeds = [int(s) for s in seeds]
        cfg = L.GpConfig()
        cfg.num_nodes = graph.num_nodes
        cfg.topology = L.GP_GRAPH
        cfg.algorithm = parse_algorithm(algorithm)
        cfg.num_gpus = 1
        cfg.device = device
        cfg.max_rounds = max_rounds
        self.topology, self.algorithm, self.graph = "graph", algorithm, graph
        self.population = graph.num_nodes
        self.faults, self.tracing, self.values = faults, trace, values
        arr = (C.c_uint64 * max(1, len(self.seeds)))(*self.seeds)
        f = None if faults is None else L.GpFaults(faults.node_fail, faults.msg_drop, faults.fail_round, 0)
        t = None if trace is None else L.GpTraceCfg(trace.stride, trace.capacity)
        v = None
        if values is not None:
            dp = C.POINTER(C.c_double)
            v = L.GpValues(values.x.ctypes.data_as(dp), None if values.w is None else values.w.ctypes.data_as(dp),
                           len(values.x), values.mean, 0)
        h = C.c_void_p()
        L.check(self._L.gp_ensemble_create_graph(C.byref(cfg), C.byref(_gp_graph(graph)),
                                                 None if v is None else C.byref(v), None if f is None else C.byref(f),
                                                 None if t is None else C.byref(t), arr, len(self.seeds), C.byref(h)),
                self._L)
        self._h = h
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._L.gp_ensemble_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def __len__(self):
        return len(self.seeds)

    def step(self, nrounds: int) -> int:
        """Every unfinished member runs up to nrounds more rounds; returns how many still run."""
        return L.check(self._L.gp_ensemble_step(self._h, nrounds), self._L)

    def run(self):
        """Run every member to convergence (or max_rounds); returns the member records."""
        out = (L.GpMember * len(self.seeds))()
        L.check(self._L.gp_ensemble_run(self._h, out), self._L)
        return list(out)

    def members(self):
        """The member records (GpMember: seed, rounds, converged, seed_node, status), in seed order."""
        out = (L.GpMember * len(self.seeds))()
        L.check(self._L.gp_ensemble_members(self._h, out), self._L)
        return list(out)

    def state(self, member: int, first: int = 0, count: int | None = None):
        """Node state of one member, as :meth:`Simulation.state`."""
        count = self.population - first if count is None else count
        c = np.zeros(count, np.int32)
        s = np.zeros(count, np.float64)
        w = np.zeros(count, np.float64)
        f = np.zeros(count, np.uint8)
        L.check(self._L.gp_ensemble_read_state(self._h, member, first, count, c.ctypes.data, s.ctypes.data,
                                               w.ctypes.data, f.ctypes.data), self._L)
        return {"c": c, "s": s, "w": w, "flags": f}

    def fault_stats(self):
        """One GpFaultStats per member, in seed order: doomed (|D|), down (|D| once the member's
        rounds reached fail_round), threshold (T_f) and lost (messages nobody received).  A plain
        ensemble reports zeros and threshold = T."""
        out = (L.GpFaultStats * len(self.seeds))()
        L.check(self._L.gp_ensemble_fault_stats(self._h, out), self._L)
        return list(out)

    def trace_rows(self):
        """Rows each member has recorded so far, in seed order: min(capacity, rounds // stride)."""
        out = (C.c_int64 * len(self.seeds))()
        L.check(self._L.gp_ensemble_trace_rows(self._h, out), self._L)
        return list(out)

    def trace(self, member: int, first: int = 0, count: int | None = None):
        """The recorded rows [first, first + count) of one member (all from `first` on by default) as
        a numpy structured array with the fields round, reached, alerts, sent and err_max
        (gp_trace_row): row k is the member's state after (k + 1) * stride rounds."""
        if count is None:
            count = self.trace_rows()[member] - first
        out = np.zeros(max(0, count), TRACE_DTYPE)
        L.check(self._L.gp_ensemble_trace_read(self._h, member, first, count, out.ctypes.data), self._L)
        return out

    def summary(self, tol: float = 1e-10):
        """One :class:`GpSummary` per member, in seed order, from one launch (gp_ensemble_summary);
        each equals ``Simulation(..., seed).summary(tol)`` at the member's round."""
        out = (L.GpSummary * len(self.seeds))()
        L.check(self._L.gp_ensemble_summary(self._h, tol, out), self._L)
        return list(out)


def run(num_nodes: int, topology: str, algorithm: str, seed: int = 1, max_rounds: int = 0, device: int = 0):
    """`dotnet run num_nodes topology algorithm` as a function: returns the gp_result."""
    with Simulation(num_nodes, topology, algorithm, seed=seed, max_rounds=max_rounds, device=device) as sim:
        return sim.run()
