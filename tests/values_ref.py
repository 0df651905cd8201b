"""Pure-Python SRS v1-V: push-sum over caller-supplied values and weights.

TEST INFRASTRUCTURE: the admissibility rules and the simulator outside the library
(gp_values.hip, gp_ensemble_kernels.hpp); tests compare the GPU with them bit for bit, and
tools/aggregate.py --backend ref runs through them.  ValueSim is tests/faults_ref.py's FaultSim
(itself a mirror of oracle/srs_py.py's PySim) with the initial (s, w) replaced and nothing else:
stop rule, Philox streams, fold order and ratio test are inherited.  trace_rows() and
ref_summary() wrap tests/trace_ref.py and tests/summary_ref.py, which hard-code mu = (P - 1) / 2,
with the mean as an input.
"""
from __future__ import annotations

import math

import numpy as np

from tests import summary_ref, trace_ref
from tests.faults_ref import FaultSim

# the rule an entry breaks, as gp_values.hpp numbers them (lowest first); 0: admissible
OK, X_SIGN, W_SIGN, W_RANGE, X_TINY, RATIO = range(6)
W_MIN, W_MAX, X_MIN = 2.0 ** -32, 2.0 ** 32, 2.0 ** -64
RULE_WORDS = {X_SIGN: "value must be finite", W_SIGN: "weight must be finite", W_RANGE: "[2^-32, 2^32]",
              X_TINY: "2^-64", RATIO: "below the weight"}


def _plain(v):
    """Finite with the sign bit clear."""
    return math.isfinite(v) and math.copysign(1.0, v) > 0


def rule(x, w=1.0):
    """The first rule the entry (x, w) breaks."""
    if not _plain(x):
        return X_SIGN
    if not _plain(w):
        return W_SIGN
    if not (W_MIN <= w <= W_MAX):
        return W_RANGE
    if not (x == 0.0 or x >= X_MIN):
        return X_TINY
    if not (x * 2.0 ** -32 < w):  # (exact: x is 0 or a normal number >= 2^-64)
        return RATIO
    return OK


def first_offender(x, w=None):
    """(node id, rule) of the lowest inadmissible entry, or None."""
    for i, xv in enumerate(x):
        r = rule(float(xv), 1.0 if w is None else float(w[i]))
        if r:
            return i, r
    return None


def mean_ok(mu):
    return math.isfinite(mu) and 0.0 <= mu < 2.0 ** 32


def default_mean(x, w=None):
    """math.fsum(x) / math.fsum(w), or / P without weights: correctly rounded sums, one division."""
    return math.fsum(float(v) for v in x) / (math.fsum(float(v) for v in w) if w is not None else len(x))


class ValueSim(FaultSim):
    """FaultSim (no faults by default) started from s_i = x_i, w_i = w_i."""

    def __init__(self, num_nodes, topology, x, w=None, seed=1, mean=None, node_fail=0.0, msg_drop=0.0, fail_round=0,
                 max_rounds=400):
        super().__init__(num_nodes, topology, "push-sum", seed, node_fail, msg_drop, fail_round, max_rounds)
        if len(x) != self.P or (w is not None and len(w) != self.P):
            raise ValueError(f"{len(x)} values for a population of {self.P}")
        bad = first_offender(x, w)
        if bad:
            raise ValueError(f"node {bad[0]} breaks rule {bad[1]}")
        self.s = [float(v) for v in x]
        self.w = [1.0] * self.P if w is None else [float(v) for v in w]
        self.mean = default_mean(x, w) if mean is None else float(mean)
        if not mean_ok(self.mean):
            raise ValueError(self.mean)

    def state(self):
        return {"c": np.zeros(self.P, np.int32), "s": np.array(self.s, np.float64), "w": np.array(self.w, np.float64),
                "flags": np.array(self.flags(), np.uint8)}


def err_max_bits(s, w, mu):
    """tests/trace_ref.py's err_max_bits with mu given."""
    with np.errstate(all="ignore"):
        e = np.asarray(s, np.float64) / np.asarray(w, np.float64) - mu
    top = int((e.view(np.uint64) & trace_ref.ABS_MASK).max())
    return trace_ref.QNAN_BITS if top > trace_ref.INF_BITS else top


def trace_rows(sim, stride=1, capacity=0):
    """tests/trace_ref.py's trace() over a fresh ValueSim, run to its end, err_max against sim.mean:
    trace_ref's own loop (the one definition of a row), with the simulator it builds and its
    err_max_bits substituted for the call.  Returns (rows, rounds, alerts, stats)."""
    saved = trace_ref.FaultSim, trace_ref.err_max_bits
    trace_ref.FaultSim = lambda *a, **k: sim
    trace_ref.err_max_bits = lambda s, w, population: err_max_bits(s, w, sim.mean)
    try:
        return trace_ref.trace.__wrapped__(0, sim.topology, "push-sum", sim.seed, stride, capacity, sim.max_rounds,
                                           (0.0, 0.0, 0))
    finally:
        trace_ref.FaultSim, trace_ref.err_max_bits = saved


def ref_summary(state, first, P, rounds, seed_node, tol, mu):
    """tests/summary_ref.py's push-sum ref_summary with the fields measured against mu redone."""
    r = summary_ref.ref_summary(state, first, P, rounds, 1, seed_node, tol)
    s, w = np.asarray(state["s"], np.float64), np.asarray(state["w"], np.float64)
    with np.errstate(all="ignore"):
        e = s / w - mu
    ae = np.abs(e)
    r["err_max"] = float(ae.max())
    r["err_max_node"] = first + int(np.argmax(ae))
    r["within_tol"] = int((ae <= tol).sum())
    r["terms"]["sum_sqerr"] = e * e
    return r
