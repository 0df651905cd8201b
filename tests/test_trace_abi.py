"""CPU tests of the ensemble-trace boundary (gp_trace_row, gp_trace_cfg, gp_ensemble_trace_*,
include/gossip_hip.h): the row matches its C layout, the traced caps cover
the report's range, every argument check of gp_ensemble_create_traced answers before any HIP call
(so it works on a host without a GPU), and the reference of the rows (tests/trace_ref.py) is
consistent with itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gossipprotocol_amd import _lib as L
from tests import trace_ref
from tests.oracle_ctypes import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_ensemble_trace_max_nodes", "gp_ensemble_create_traced", "gp_ensemble_trace_rows",
         "gp_ensemble_trace_read")
PAIRS = [(t, a) for t in (L.GP_LINE, L.GP_FULL, L.GP_3D, L.GP_IMP3D) for a in (L.GP_GOSSIP, L.GP_PUSHSUM)]
GP_EINVAL = -1


def test_version_is_unchanged():
    assert L.lib().gp_version() == 10100


def test_library_exports_the_trace_symbols():
    raw = C.CDLL(L.LIB_PATH)
    bound = {n for n, _, _ in L.SIGNATURES}
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in bound, n


def test_row_layout_matches_c(tmp_path):
    src = tmp_path / "row.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gp_trace_row), offsetof(gp_trace_row, round),'
                   'offsetof(gp_trace_row, reached), offsetof(gp_trace_row, alerts), offsetof(gp_trace_row, sent),'
                   'offsetof(gp_trace_row, err_max));'
                   'printf("%zu %zu %zu %zu\\n", sizeof(gp_trace_cfg), offsetof(gp_trace_cfg, stride),'
                   'offsetof(gp_trace_cfg, capacity), offsetof(gp_trace_cfg, reserved));return 0;}\n')
    exe = tmp_path / "row"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got[:6] == [32, 0, 8, 12, 16, 24]
    R, T = L.GpTraceRow, L.GpTraceCfg
    assert got[:6] == [C.sizeof(R), R.round.offset, R.reached.offset, R.alerts.offset, R.sent.offset, R.err_max.offset]
    assert got[6:] == [C.sizeof(T), T.stride.offset, T.capacity.offset, T.reserved.offset] == [32, 0, 8, 16]
    # the numpy rows Ensemble.trace returns, and the reference's
    from gossipprotocol_amd.sim import TRACE_DTYPE
    for dt in (TRACE_DTYPE, trace_ref.ROW):
        assert dt.itemsize == 32
        assert [dt.fields[k][1] for k in ("round", "reached", "alerts", "sent", "err_max")] == [0, 8, 12, 16, 24]


@pytest.mark.parametrize("faults", (0, 1))
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_traced_cap_covers_the_report_range(topo, alg, faults):
    lib = L.lib()
    cap = lib.gp_ensemble_trace_max_nodes(topo, alg, faults)
    plain = lib.gp_ensemble_faults_max_nodes(topo, alg) if faults else lib.gp_ensemble_max_nodes(topo, alg)
    assert 1000 <= cap <= plain


def test_traced_cap_refuses_unknown_pair_and_python_reports_it():
    lib = L.lib()
    assert lib.gp_ensemble_trace_max_nodes(4, L.GP_GOSSIP, 0) == GP_EINVAL
    assert b"topology" in lib.gp_last_error()
    assert lib.gp_ensemble_trace_max_nodes(L.GP_LINE, 2, 1) == GP_EINVAL
    assert b"algorithm" in lib.gp_last_error()
    from gossipprotocol_amd import ensemble_max_nodes
    for f in (False, True):
        assert ensemble_max_nodes("full", "push-sum", faults=f, trace=True) == \
            lib.gp_ensemble_trace_max_nodes(L.GP_FULL, L.GP_PUSHSUM, int(f))


def _create(n=100, topo=L.GP_3D, alg=L.GP_PUSHSUM, nseeds=2, max_rounds=1000, trace=(1, 0, 0, 0), faults=None):
    cfg = L.GpConfig()
    cfg.num_nodes, cfg.topology, cfg.algorithm = n, topo, alg
    cfg.num_gpus, cfg.device, cfg.max_rounds, cfg.flags = 1, 0, max_rounds, 0
    arr = (C.c_uint64 * 2)(1, 2)  # (a refused call reads no seed)
    t = None if trace is None else L.GpTraceCfg(trace[0], trace[1], (C.c_int64 * 2)(trace[2], trace[3]))
    f = None if faults is None else L.GpFaults(*faults)
    h = C.c_void_p()
    rc = L.lib().gp_ensemble_create_traced(C.byref(cfg), None if f is None else C.byref(f),
                                           None if t is None else C.byref(t), arr, nseeds, C.byref(h))
    if rc == 0:  # (a GPU is present and the arguments were fine)
        L.lib().gp_ensemble_destroy(h)
    return rc, L.lib().gp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(trace=None), b"trace is null"),
    (dict(trace=(0, 0, 0, 0)), b"stride"),
    (dict(trace=(-4, 0, 0, 0)), b"stride"),
    (dict(trace=(1, -1, 0, 0)), b"capacity"),
    (dict(trace=(1, 0, 1, 0)), b"reserved"),
    (dict(trace=(1, 0, 0, 7)), b"reserved"),
    (dict(faults=(1.5, 0.0, 0, 0)), b"node_fail"),
    (dict(faults=(0.0, 0.0, 0, 3)), b"reserved"),
    (dict(max_rounds=0), b"max_rounds"),
    (dict(nseeds=0), b"nseeds"),
    (dict(topo=9), b"topology"),
])
def test_create_traced_refuses_bad_arguments(kw, word):
    rc, msg = _create(**kw)
    assert rc == GP_EINVAL, (kw, rc, msg)
    assert word in msg, msg


def test_create_traced_refuses_more_than_one_gib_of_rows():
    # 2^25 rows of 32 bytes are 1 GiB: 2 members x 2^24 rows fit, one row more per member does not
    rows = 1 << 24
    rc, msg = _create(max_rounds=1 << 40, trace=(1, rows + 1, 0, 0))
    assert rc == GP_EINVAL and b"1 GiB" in msg, (rc, msg)
    rc, msg = _create(max_rounds=1 << 40, trace=(1, rows, 0, 0))
    assert rc in (0, -2, -6), (rc, msg)  # past the argument checks (refused, if at all, for the missing GPU or memory)
    # capacity 0 is floor(max_rounds / stride) rows: the message names the smallest stride that fits
    M = 100 * rows + 5
    rc, msg = _create(max_rounds=M, trace=(1, 0, 0, 0))
    assert rc == GP_EINVAL and b"1 GiB" in msg, (rc, msg)
    stride = M // (rows + 1) + 1
    assert M // stride <= rows < M // (stride - 1)
    assert f"stride that records every row (capacity 0) is {stride}".encode() in msg, msg
    rc, msg = _create(max_rounds=M, trace=(stride - 1, 0, 0, 0))
    assert rc == GP_EINVAL and b"1 GiB" in msg, (rc, msg)


@pytest.mark.parametrize("faults", (None, (0.1, 0.1, 3, 0)))
@pytest.mark.parametrize("topo,alg", PAIRS)
def test_create_traced_refuses_one_node_past_the_traced_cap(topo, alg, faults):
    cap = L.lib().gp_ensemble_trace_max_nodes(topo, alg, int(faults is not None))
    rc, msg = _create(n=cap + 1, topo=topo, alg=alg, faults=faults)
    assert rc == GP_EINVAL and b"cap" in msg and b"trace layout" in msg, (rc, msg)
    rc, msg = _create(n=cap, topo=topo, alg=alg, faults=faults, trace=(64, 4, 0, 0))
    assert rc in (0, -6), (rc, msg)


def test_trace_calls_refuse_a_null_handle():
    lib = L.lib()
    out = (C.c_int64 * 1)()
    assert lib.gp_ensemble_trace_rows(None, out) == GP_EINVAL
    assert lib.gp_ensemble_trace_read(None, 0, 0, 0, None) == GP_EINVAL


@pytest.mark.parametrize("alg", ("gossip", "push-sum"))
@pytest.mark.parametrize("faults", (None, (0.2, 0.1, 5)))
def test_reference_rows_are_consistent(alg, faults):
    n, topo, seed = 27, "Imp3D", 2
    rows, rounds, alerts, stats = trace_ref.trace(n, topo, alg, seed, 1, 0, 400, faults)
    assert (stats is None) == (faults is None)
    assert len(rows) == rounds and list(rows["round"]) == list(range(1, rounds + 1))
    for k in ("reached", "alerts", "sent"):
        assert (np.diff(rows[k].astype(np.int64)) >= 0).all(), k
    assert rows["alerts"][-1] == alerts and rows["reached"][-1] <= 27
    assert rows["sent"][0] == 1  # round 1: the seed node alone draws a target
    if faults is None:
        o = Oracle(n, topo, alg, seed, max_rounds=400, threads=1)
        o.run(max_rounds=400)
        assert (rounds, alerts) == (o.rounds, o.alerts_total) and alerts == o.T
        assert rows["reached"][-1] == 27
        o.close()
    if alg == "gossip":
        assert not rows["err_max"].any()
    else:
        assert np.isfinite(rows["err_max"]).all() and rows["err_max"][0] == 13.0  # (the node 0 or 26 holds)
    # a strided, capped trace is the matching subset of the full one
    sub, r2, a2, _ = trace_ref.trace(n, topo, alg, seed, 3, 4, 400, faults)
    assert (r2, a2) == (rounds, alerts)
    assert sub.tobytes() == rows[2::3][:4].tobytes()


def test_reference_err_max_rule():
    b = trace_ref.err_max_bits
    assert b([1.0, 3.0], [1.0, 1.0], 3) == np.array([2.0]).view(np.uint64)[0]          # |3 - 1|
    assert b([0.0, 3.0], [1.0, 1.0], 3) == np.array([2.0]).view(np.uint64)[0]          # |0 - 1| < |3 - 1|
    assert b([-5.0, 1.0], [0.0, 1.0], 3) == trace_ref.INF_BITS                        # -inf: the sign is cleared
    assert b([0.0, 5.0], [0.0, 0.0], 3) == trace_ref.QNAN_BITS                        # 0 / 0 beats +inf
    assert b([1.0, -np.nan], [1.0, 1.0], 3) == trace_ref.QNAN_BITS                    # any NaN reads as the quiet one
