"""GPU: ensemble traces (gp_ensemble_create_traced, gp_ensemble_trace.hip; SRS v1-T, DESIGN.md
section 12) -- every field of every row a member records equals the reference's
(tests/trace_ref.py: the C oracle, or the pure-Python SRS v1-F simulator under a failure model,
stepped a round at a time), err_max by its bits; and tracing observes only: members, state (raw
bits of s and w), fault stats and summary equal those of the untraced ensemble of the same
arguments.

Shapes, from the existing ensemble tests: line / full n = 1, 2 (P = 2, 3), 31, 32 (P = 32, 33: the
bitmap word edge), 64 (one node past a wave); 3D / Imp3D n = 8, 27, 28; line push-sum n = 1100 (two
node slots per thread); the traced caps (eight slots per thread, strided gossip loops) for 24
rounds; one line push-sum member at n = 1000 run to convergence (about 13 000 rounds, across the
8192-round launch chunk).  Reference runs are capped at 400 rounds (300 at n = 1100).

err_max under loss: within 400 rounds no weight reaches 0 at these shapes (a weight halves at most
once a round, 2^-400 is a normal double), so those rows pin the rule with finite values only; one
more case, push-sum with every message dropped for 1100 rounds at P = 3, takes the seed node's
weight through the subnormals to 0 in round 1075 and its rows hold +inf and the canonical NaN.
"""
import numpy as np
import pytest

from gossipprotocol_amd import Ensemble, Faults, Trace, ensemble_max_nodes
from gossipprotocol_amd import _lib as L
from tests import trace_ref

pytestmark = pytest.mark.gpu

TOPOS = ("line", "full", "3D", "Imp3D")
ALGS = ("gossip", "push-sum")
PAIRS = [(t, a) for t in TOPOS for a in ALGS]
SEEDS = (1, 2, 2**63 + 3)  # (the high seed word reaches the Philox key)
# the five parameter sets of tests/test_gpu_ensemble_faults.py: (node_fail, msg_drop, fail_round)
PARAMS = [(0.25, 0.0, 0), (0.0, 0.25, 0), (0.2, 0.1, 5), (1.0, 0.0, 0), (0.0, 1.0, 0)]
GP_EINVAL, GP_ESTATE = -1, -5


def drive(ens, k):
    """run(), or step(k) until nobody runs."""
    if k is None:
        ens.run()
    else:
        while ens.step(k):
            pass


def observe(ens):
    """Everything but the trace that a caller can read from an ensemble."""
    recs = [(r.seed, r.rounds, r.converged, r.seed_node, r.status) for r in ens.members()]
    state = [tuple(ens.state(m)[k].tobytes() for k in ("c", "s", "w", "flags")) for m in range(len(ens))]
    stats = [(f.doomed, f.down, f.threshold, f.lost) for f in ens.fault_stats()]
    return recs, state, stats, [bytes(s) for s in ens.summary()]


def check(n, topo, alg, seeds, max_rounds, stride=1, capacity=0, faults=None, step=None, untraced=True):
    """One traced ensemble against the reference and against the untraced ensemble; returns the rows."""
    fa = None if faults is None else Faults(*faults)
    want = [trace_ref.trace(n, topo, alg, s, stride, capacity, max_rounds, faults) for s in seeds]
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=fa, trace=Trace(stride, capacity)) as ens:
        drive(ens, step)
        recs, nrows = ens.members(), ens.trace_rows()
        got = [ens.trace(m) for m in range(len(seeds))]
        seen = observe(ens)
    for m, seed in enumerate(seeds):
        rows, rounds, alerts, _ = want[m]
        what = f"{topo} {alg} n={n} seed={seed} stride={stride} capacity={capacity} faults={faults} step={step}"
        assert (recs[m].rounds, recs[m].converged) == (rounds, alerts), what
        assert nrows[m] == len(rows) == min(capacity or max_rounds // stride, rounds // stride), what
        trace_ref.assert_rows_equal(got[m], rows, what)
    if untraced:
        with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=fa) as plain:
            drive(plain, step)
            assert observe(plain) == seen, f"{topo} {alg} n={n}: the traced ensemble differs from the untraced one"
    return got, want


# ---------------------------------------------------------------- small shapes, every pair
def small_shapes():
    for topo, alg in PAIRS:
        for n in ([1, 2, 31, 32, 64] if topo in ("line", "full") else [8, 27, 28]):
            yield topo, alg, n


@pytest.mark.parametrize("topo,alg,n", list(small_shapes()))
def test_rows_equal_the_reference(topo, alg, n):
    got, _ = check(n, topo, alg, SEEDS, 400)
    assert all(len(g) >= 1 for g in got)


def test_two_node_slots_per_thread():
    got, _ = check(1100, "line", "push-sum", SEEDS, 300)
    assert all(len(g) == 300 for g in got)


# ---------------------------------------------------------------- stepping and launch boundaries
@pytest.mark.parametrize("topo,alg,n,faults", [("Imp3D", "push-sum", 27, None), ("line", "gossip", 31, None),
                                               ("full", "push-sum", 32, (0.2, 0.1, 5)),
                                               ("3D", "gossip", 28, (0.2, 0.1, 5))])
@pytest.mark.parametrize("stride", (1, 3))
def test_stepping_gives_the_same_rows(topo, alg, n, faults, stride):
    # the recount of `reached` at launch start, `sent` persisting in the member's record, the row clock
    for step in (1, 7, 64, None):
        check(n, topo, alg, SEEDS, 200, stride=stride, faults=faults, step=step, untraced=step is None)


def test_rows_across_the_launch_chunk():
    n, stride = 1000, 64
    got, want = check(n, "line", "push-sum", (1,), 200_000, stride=stride)
    rounds = want[0][1]
    assert rounds > 8192 and len(got[0]) == rounds // stride  # more than one launch of a run()
    assert got[0]["reached"][-1] == n + 1 and got[0]["err_max"][-1] < got[0]["err_max"][0]


# ---------------------------------------------------------------- stride and capacity edges
def test_capacity_stops_the_recording_not_the_run():
    n, topo, alg = 64, "line", "push-sum"
    full, want = check(n, topo, alg, SEEDS, 400, stride=7)
    cap = min(w[1] for w in want) // 7 - 2
    assert cap >= 2
    got, want = check(n, topo, alg, SEEDS, 400, stride=7, capacity=cap)
    for m in range(len(SEEDS)):
        assert len(got[m]) == cap < want[m][1] // 7
        assert got[m].tobytes() == full[m][:cap].tobytes()


def test_stride_beyond_the_run_records_nothing():
    with Ensemble(27, "Imp3D", "gossip", SEEDS, max_rounds=400, trace=Trace(stride=399)) as ens:
        recs = ens.run()
        assert all(r.rounds < 399 for r in recs)
        assert ens.trace_rows() == [0, 0, 0]
        assert len(ens.trace(1)) == 0
        lib, buf = L.lib(), (L.GpTraceRow * 1)()
        assert lib.gp_ensemble_trace_read(ens._h, 1, 0, 0, buf) == 0
        assert lib.gp_ensemble_trace_read(ens._h, 1, 0, 1, buf) == GP_EINVAL
        assert b"recorded" in lib.gp_last_error()


def test_read_past_the_recorded_rows_is_refused():
    lib = L.lib()
    with Ensemble(27, "3D", "push-sum", SEEDS, max_rounds=400, trace=Trace(stride=2)) as ens:
        ens.step(9)
        assert ens.trace_rows() == [4, 4, 4]
        buf = (L.GpTraceRow * 8)()
        assert lib.gp_ensemble_trace_read(ens._h, 0, 0, 4, buf) == 0
        assert [buf[k].round for k in range(4)] == [2, 4, 6, 8]
        assert lib.gp_ensemble_trace_read(ens._h, 2, 3, 1, buf) == 0 and buf[0].round == 8
        for member, first, count in ((0, 0, 5), (0, 4, 1), (0, 5, 0), (0, -1, 1), (0, 0, -1), (3, 0, 0), (-1, 0, 0)):
            assert lib.gp_ensemble_trace_read(ens._h, member, first, count, buf) == GP_EINVAL, (member, first, count)
        assert lib.gp_ensemble_trace_read(ens._h, 0, 4, 0, buf) == 0


def test_untraced_ensemble_has_no_trace():
    lib = L.lib()
    with Ensemble(27, "3D", "gossip", SEEDS, max_rounds=400, faults=Faults(0.1, 0.1, 2)) as ens:
        ens.run()
        out = (L.GpTraceRow * 1)()
        n = (L.C.c_int64 * 3)()
        assert lib.gp_ensemble_trace_rows(ens._h, n) == GP_ESTATE
        assert lib.gp_ensemble_trace_read(ens._h, 0, 0, 0, out) == GP_ESTATE
        with pytest.raises(L.GossipError):
            ens.trace_rows()


# ---------------------------------------------------------------- at the traced caps (eight node slots per thread)
@pytest.mark.parametrize("faults", (None, (0.0, 0.0, 0)))
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_rows_at_the_traced_cap(topo, alg, faults):
    # (with a failure model only the zero one: the pure-Python reference cannot hold full's lists at the cap)
    n = ensemble_max_nodes(topo, alg, faults=faults is not None, trace=True)
    want = trace_ref.trace(n, topo, alg, 1, 8, 0, 24, None)
    fa = None if faults is None else Faults(*faults)
    with Ensemble(n, topo, alg, [1], max_rounds=24, faults=fa, trace=Trace(stride=8)) as ens:
        ens.run()
        rec = ens.members()[0]
        assert (rec.rounds, rec.converged) == want[1:3]
        assert ens.trace_rows() == [3]
        trace_ref.assert_rows_equal(ens.trace(0), want[0], f"{topo} {alg} n={n}")
        seen = observe(ens)
    with Ensemble(n, topo, alg, [1], max_rounds=24, faults=fa) as plain:
        plain.run()
        assert observe(plain) == seen


# ---------------------------------------------------------------- failure model
def fault_shapes():
    for topo, alg in PAIRS:
        for n in ([32, 64] if topo in ("line", "full") else [27, 28]):
            yield topo, alg, n


@pytest.mark.parametrize("k", range(len(PARAMS)))
@pytest.mark.parametrize("topo,alg,n", list(fault_shapes()))
def test_rows_under_the_failure_model(topo, alg, n, k):
    nf, md, fr = PARAMS[k]
    got, want = check(n, topo, alg, SEEDS, 400, faults=PARAMS[k])
    # not vacuous: the case dooms a node / loses a message in at least one member
    if nf > 0:
        assert any(w[3][0] >= 1 for w in want), "no member has a doomed node"
    assert any(w[3][3] >= 1 for w in want), "no member loses a message"
    if alg == "push-sum":  # 400 rounds take no weight to 0 (module docstring): every err_max is finite
        assert all(np.isfinite(g["err_max"]).all() for g in got)
        if k == 4:  # only the seed node ever sends: into the void, every round
            for m, g in enumerate(got):
                assert (g["reached"] == 1).all() and list(g["sent"]) == list(range(1, 401))


def test_err_max_once_a_weight_is_zero():
    got, _ = check(2, "line", "push-sum", SEEDS, 1100, faults=(0.0, 1.0, 0))
    bits = np.concatenate([g["err_max"].view(np.uint64) for g in got])
    assert (bits == trace_ref.QNAN_BITS).any(), "no row holds the canonical NaN"
    assert ((bits <= trace_ref.INF_BITS) | (bits == trace_ref.QNAN_BITS)).all()
    for g in got:  # w = 2^-R is 0 from round 1075 on: 0 / 0, or s / 0 while s is still a subnormal
        b = g["err_max"].view(np.uint64)
        assert (b[:1074] < trace_ref.INF_BITS).all() and (b[1074:] >= trace_ref.INF_BITS).all()


# ---------------------------------------------------------------- many members, duplicate seeds
def test_600_members_with_duplicate_seeds():
    n, topo, alg, max_rounds = 27, "Imp3D", "push-sum", 200
    seeds = [1 + (m % 300) for m in range(600)]
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, faults=Faults(0.2, 0.1, 5), trace=Trace(2)) as ens:
        recs = ens.run()
        nrows = ens.trace_rows()
        rows = [ens.trace(m) for m in range(600)]
    for m in range(300):
        assert nrows[m] == nrows[m + 300] == recs[m].rounds // 2
        assert rows[m].tobytes() == rows[m + 300].tobytes(), m
    assert len({r.tobytes() for r in rows[:300]}) > 1, "the members should differ"
    for m in (0, 7, 299):
        want = trace_ref.trace(n, topo, alg, seeds[m], 2, 0, max_rounds, (0.2, 0.1, 5))
        trace_ref.assert_rows_equal(rows[m], want[0], f"member {m}")
