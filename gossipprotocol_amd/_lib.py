"""ctypes binding of libgossip_hip.so (C-ABI: include/gossip_hip.h).

The product path: there is no CPU fallback.  If the in-tree HIP library is
missing, loading raises -- build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libgossip_hip.so")
# The experiments build (-DGP_EXPERIMENTS: kernel variants and GP_* environment
# overrides) -- loaded only by the kernel-variant tests and tools/, never by default.
EXP_LIB_PATH = os.path.join(PKG_DIR, "libgossip_hip_exp.so")
# tools/ablate.py may point the experiments slot at an ablation build
EXP_LIB_PATH = os.environ.get("GOSSIP_HIP_LIB_EXPERIMENT", EXP_LIB_PATH)

GP_LINE, GP_FULL, GP_3D, GP_IMP3D = 0, 1, 2, 3
GP_GRAPH = 4  # a caller-supplied graph: gp_ensemble_create_graph only, and it has no string
GP_GOSSIP, GP_PUSHSUM = 0, 1
GP_STATUS_CONVERGED, GP_STATUS_MAX_ROUNDS, GP_STATUS_RUNNING = 0, 1, 2
GP_FLAG_KERNEL_TIMING = 1
GP_FLAG_VIRTUAL_RANKS = 2
GP_SCOPE_LOCAL, GP_SCOPE_GLOBAL = 0, 1
GP_STATE_DOWN = 0x10  # gp_ensemble_read_state flag bit 4 (failure ensembles)
ERRORS = {-1: "GP_EINVAL", -2: "GP_ENOMEM", -3: "GP_EHIP", -4: "GP_ENCCL", -5: "GP_ESTATE", -6: "GP_ENODEV"}


class GpConfig(C.Structure):
    _fields_ = [("num_nodes", C.c_int64), ("topology", C.c_int32), ("algorithm", C.c_int32),
                ("seed", C.c_uint64), ("num_gpus", C.c_int32), ("device", C.c_int32),
                ("max_rounds", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


class GpResult(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("converged", C.c_int64), ("population", C.c_int64),
                ("threshold", C.c_int64), ("elapsed_ms", C.c_double), ("node_updates_per_s", C.c_double),
                ("hbm_bytes_alg", C.c_double), ("status", C.c_int32), ("reserved", C.c_int32)]


class GpInfo(C.Structure):
    _fields_ = [("population", C.c_int64), ("threshold", C.c_int64), ("grid", C.c_int64),
                ("seed_node", C.c_int64), ("rounds", C.c_int64), ("alerts_total", C.c_int64),
                ("active", C.c_int64), ("topology", C.c_int32), ("algorithm", C.c_int32),
                ("device", C.c_int32), ("num_gpus", C.c_int32), ("slab_first", C.c_int64),
                ("slab_count", C.c_int64)]


class GpMember(C.Structure):
    """One ensemble member (gp_member)."""
    _fields_ = [("seed", C.c_uint64), ("rounds", C.c_int64), ("converged", C.c_int64),
                ("seed_node", C.c_int64), ("status", C.c_int32), ("reserved", C.c_int32)]


class GpFaults(C.Structure):
    """Failure model of an ensemble (gp_faults)."""
    _fields_ = [("node_fail", C.c_double), ("msg_drop", C.c_double), ("fail_round", C.c_int64),
                ("reserved", C.c_int64)]


class GpFaultStats(C.Structure):
    """Per-member failure statistics (gp_fault_stats)."""
    _fields_ = [("doomed", C.c_int64), ("down", C.c_int64), ("threshold", C.c_int64), ("lost", C.c_int64)]


class GpTraceRow(C.Structure):
    """One row of an ensemble member's trace (gp_trace_row)."""
    _fields_ = [("round", C.c_int64), ("reached", C.c_uint32), ("alerts", C.c_uint32), ("sent", C.c_uint64),
                ("err_max", C.c_double)]


class GpTraceCfg(C.Structure):
    """Trace parameters of an ensemble (gp_trace_cfg)."""
    _fields_ = [("stride", C.c_int64), ("capacity", C.c_int64), ("reserved", C.c_int64 * 2)]


class GpValues(C.Structure):
    """Values and weights every member of an ensemble starts from (gp_values)."""
    _fields_ = [("x", C.POINTER(C.c_double)), ("w", C.POINTER(C.c_double)), ("count", C.c_int64),
                ("mean", C.c_double), ("reserved", C.c_int64)]


class GpGraph(C.Structure):
    """A directed graph in CSR form (gp_graph)."""
    _fields_ = [("indptr", C.POINTER(C.c_int64)), ("indices", C.POINTER(C.c_uint32)), ("num_nodes", C.c_int64),
                ("num_edges", C.c_int64), ("reserved", C.c_int64)]


class GpSummary(C.Structure):
    """What a run computed, reduced on the device (gp_summary)."""
    _fields_ = [("first", C.c_int64), ("count", C.c_int64), ("population", C.c_int64), ("rounds", C.c_int64),
                ("algorithm", C.c_int32), ("reserved", C.c_int32), ("active", C.c_int64), ("converged", C.c_int64),
                ("c_hist", C.c_int64 * 12), ("c_max", C.c_int32), ("reserved2", C.c_int32),
                ("cnt_hist", C.c_int64 * 4), ("est_min", C.c_double), ("est_max", C.c_double),
                ("w_min", C.c_double), ("w_max", C.c_double), ("err_max", C.c_double),
                ("err_max_node", C.c_int64), ("within_tol", C.c_int64), ("tol", C.c_double),
                ("sum_s", C.c_double * 2), ("sum_w", C.c_double * 2), ("sum_sqerr", C.c_double * 2)]

    # derived from the double-double sums (push-sum; 0 / nan-free for gossip, whose sums are 0)
    @property
    def mass(self):
        """(sum of s, sum of w): what push-sum conserves."""
        return self.sum_s[0], self.sum_w[0]

    @property
    def mean_estimate(self):
        """sum of s over sum of w: the average the covered nodes hold between them."""
        return self.sum_s[0] / self.sum_w[0] if self.sum_w[0] else 0.0

    @property
    def rms_error(self):
        """Root mean square over the covered nodes of e = s / w - mu (mu: the handle's mean)."""
        return (self.sum_sqerr[0] / self.count) ** 0.5 if self.count else 0.0

    def merge(self, other):
        """This summary joined with the one of the adjacent, higher id range (gp_summary_merge)."""
        out = GpSummary()
        check(lib().gp_summary_merge(C.byref(self), C.byref(other), C.byref(out)))
        return out


# (name, restype, argtypes) for every symbol include/gossip_hip.h declares
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
SIGNATURES = [
    ("gp_version", _i32, []),
    ("gp_last_error", C.c_char_p, []),
    ("gp_parse_topology", _i32, [C.c_char_p]),
    ("gp_parse_algorithm", _i32, [C.c_char_p]),
    ("gp_resolve", _i32, [_i64, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("gp_create", _i32, [C.POINTER(GpConfig), C.POINTER(_vp)]),
    ("gp_get_unique_id", _i32, [C.c_char_p]),
    ("gp_rendezvous_id", _i32, [_i32, C.c_char_p, _i32, C.c_char_p]),
    ("gp_create_rank", _i32, [C.POINTER(GpConfig), _i32, _i32, C.c_char_p, C.POINTER(_vp)]),
    ("gp_run", _i32, [_vp, C.POINTER(GpResult)]),
    ("gp_step", _i64, [_vp, _i64, C.POINTER(_i64)]),
    ("gp_read_state", _i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("gp_neighbors", _i32, [_vp, _i64, C.POINTER(_i64), _i64]),
    ("gp_get_info", _i32, [_vp, C.POINTER(GpInfo)]),
    ("gp_sync", _i32, [_vp]),
    ("gp_kernel_stats", _i32, [_vp, C.POINTER(C.c_double), C.POINTER(_i64), C.c_char_p, _i32, _i32]),
    ("gp_alg_bytes_per_node", C.c_double, [_vp]),
    ("gp_destroy", None, [_vp]),
    ("gp_ensemble_max_nodes", _i64, [_i32, _i32]),
    ("gp_ensemble_create", _i32, [C.POINTER(GpConfig), C.POINTER(C.c_uint64), _i64, C.POINTER(_vp)]),
    ("gp_ensemble_step", _i64, [_vp, _i64]),
    ("gp_ensemble_run", _i32, [_vp, C.POINTER(GpMember)]),
    ("gp_ensemble_members", _i32, [_vp, C.POINTER(GpMember)]),
    ("gp_ensemble_read_state", _i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("gp_ensemble_destroy", None, [_vp]),
    ("gp_ensemble_faults_max_nodes", _i64, [_i32, _i32]),
    ("gp_ensemble_create_faults", _i32, [C.POINTER(GpConfig), C.POINTER(GpFaults), C.POINTER(C.c_uint64), _i64,
                                         C.POINTER(_vp)]),
    ("gp_ensemble_fault_stats", _i32, [_vp, C.POINTER(GpFaultStats)]),
    ("gp_ensemble_trace_max_nodes", _i64, [_i32, _i32, _i32]),
    ("gp_ensemble_create_traced", _i32, [C.POINTER(GpConfig), C.POINTER(GpFaults), C.POINTER(GpTraceCfg),
                                         C.POINTER(C.c_uint64), _i64, C.POINTER(_vp)]),
    ("gp_ensemble_trace_rows", _i32, [_vp, C.POINTER(_i64)]),
    ("gp_ensemble_trace_read", _i32, [_vp, _i64, _i64, _i64, _vp]),
    ("gp_summary_take", _i32, [_vp, C.c_double, _i32, C.POINTER(GpSummary)]),
    ("gp_summary_merge", _i32, [C.POINTER(GpSummary), C.POINTER(GpSummary), C.POINTER(GpSummary)]),
    ("gp_ensemble_summary", _i32, [_vp, C.c_double, C.POINTER(GpSummary)]),
    ("gp_set_values", _i32, [_vp, _i64, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("gp_set_mean", _i32, [_vp, C.c_double]),
    ("gp_ensemble_create_values", _i32, [C.POINTER(GpConfig), C.POINTER(GpValues), C.POINTER(GpFaults),
                                         C.POINTER(GpTraceCfg), C.POINTER(C.c_uint64), _i64, C.POINTER(_vp)]),
    ("gp_ensemble_graph_lds_bytes", _i64, [C.POINTER(GpGraph), _i32, _i32, _i32]),
    ("gp_ensemble_create_graph", _i32, [C.POINTER(GpConfig), C.POINTER(GpGraph), C.POINTER(GpValues), C.POINTER(GpFaults),
                                        C.POINTER(GpTraceCfg), C.POINTER(C.c_uint64), _i64, C.POINTER(_vp)]),
]

_libs = {}


class GossipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


def lib(experimental: bool = False):
    """Load the in-tree HIP library (raises if it has not been built).
    experimental=True loads the experiments build instead (tests / tools only)."""
    path = EXP_LIB_PATH if experimental else LIB_PATH
    L = _libs.get(path)
    if L is None:
        if not os.path.exists(path):
            raise ImportError(f"{path} not built: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(path)
        for name, res, args in SIGNATURES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _libs[path] = L
    return L


def check(rc, L=None):
    if rc < 0:
        raise GossipError(rc, (L or lib()).gp_last_error().decode(errors="replace"))
    return rc
