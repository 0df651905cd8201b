"""CPU tests of the failure-model boundary (gp_ensemble_create_faults and friends,
include/gossip_hip.h): the symbols exist, gp_faults and gp_fault_stats match their C
layout, the failure caps cover the report's range and never exceed the plain ones, and
every refusal answers before any HIP call (so it works on a host without a GPU)."""
import ctypes as C
import os
import subprocess

import pytest

from gossipprotocol_amd import Faults, ensemble_max_nodes
from gossipprotocol_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_ensemble_faults_max_nodes", "gp_ensemble_create_faults", "gp_ensemble_fault_stats")
TOPOS = {"line": L.GP_LINE, "full": L.GP_FULL, "3D": L.GP_3D, "Imp3D": L.GP_IMP3D}
ALGS = {"gossip": L.GP_GOSSIP, "push-sum": L.GP_PUSHSUM}
PAIRS = [(t, a) for t in TOPOS for a in ALGS]
GP_EINVAL, GP_ENODEV = -1, -6


def test_library_exports_the_symbols():
    raw = C.CDLL(L.LIB_PATH)
    bound = {n for n, _, _ in L.SIGNATURES}
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in bound, n
    assert L.lib().gp_version() == 10100  # the ABI grew, the version did not move


def test_struct_layouts_match_c(tmp_path):
    src = tmp_path / "faults.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(gp_faults), offsetof(gp_faults, node_fail),'
                   'offsetof(gp_faults, msg_drop), offsetof(gp_faults, fail_round), offsetof(gp_faults, reserved));'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(gp_fault_stats), offsetof(gp_fault_stats, doomed),'
                   'offsetof(gp_fault_stats, down), offsetof(gp_fault_stats, threshold), offsetof(gp_fault_stats, lost));'
                   'printf("%d\\n", (int)GP_STATE_DOWN);return 0;}\n')
    exe = tmp_path / "faults"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    F, S = L.GpFaults, L.GpFaultStats
    assert got == [C.sizeof(F), F.node_fail.offset, F.msg_drop.offset, F.fail_round.offset, F.reserved.offset,
                   C.sizeof(S), S.doomed.offset, S.down.offset, S.threshold.offset, S.lost.offset, L.GP_STATE_DOWN]
    assert C.sizeof(F) == 32 and C.sizeof(S) == 32 and L.GP_STATE_DOWN == 0x10


@pytest.mark.parametrize("topo,alg", PAIRS)
def test_failure_cap_covers_the_report_range(topo, alg):
    lib = L.lib()
    cap = lib.gp_ensemble_faults_max_nodes(TOPOS[topo], ALGS[alg])
    assert 1000 <= cap <= lib.gp_ensemble_max_nodes(TOPOS[topo], ALGS[alg])
    assert ensemble_max_nodes(topo, alg, faults=True) == cap
    assert ensemble_max_nodes(topo, alg) == lib.gp_ensemble_max_nodes(TOPOS[topo], ALGS[alg])


def test_bitmap_lowers_the_full_pushsum_cap():
    # 22 B per node become 22 1/8: the one pair whose plain cap the LDS bounds below a cube or 8192
    lib = L.lib()
    assert lib.gp_ensemble_faults_max_nodes(L.GP_FULL, L.GP_PUSHSUM) < lib.gp_ensemble_max_nodes(L.GP_FULL, L.GP_PUSHSUM)


def test_failure_cap_refuses_unknown_pair():
    lib = L.lib()
    assert lib.gp_ensemble_faults_max_nodes(4, L.GP_GOSSIP) == GP_EINVAL
    assert b"topology" in lib.gp_last_error()
    assert lib.gp_ensemble_faults_max_nodes(L.GP_LINE, 2) == GP_EINVAL
    assert b"algorithm" in lib.gp_last_error()


def _create(n=100, topo=L.GP_3D, alg=L.GP_PUSHSUM, seeds=(1, 2), nseeds=None, num_gpus=1, flags=0, max_rounds=1000,
            faults=(0.1, 0.1, 0, 0)):
    cfg = L.GpConfig()
    cfg.num_nodes, cfg.topology, cfg.algorithm = n, topo, alg
    cfg.num_gpus, cfg.device, cfg.max_rounds, cfg.flags = num_gpus, 0, max_rounds, flags
    arr = None if seeds is None else (C.c_uint64 * max(1, len(seeds)))(*seeds)
    f = None if faults is None else C.byref(L.GpFaults(*faults))
    h = C.c_void_p()
    n_arg = nseeds if nseeds is not None else (len(seeds) if seeds is not None else 2)
    rc = L.lib().gp_ensemble_create_faults(C.byref(cfg), f, arr, n_arg, C.byref(h))
    if rc == 0:  # (a GPU is present and the arguments were fine)
        L.lib().gp_ensemble_destroy(h)
    return rc, L.lib().gp_last_error()


@pytest.mark.parametrize("kw,word", [
    # the new refusals name their field
    (dict(faults=None), b"faults"),
    (dict(faults=(float("nan"), 0.0, 0, 0)), b"node_fail"),
    (dict(faults=(-0.01, 0.0, 0, 0)), b"node_fail"),
    (dict(faults=(1.01, 0.0, 0, 0)), b"node_fail"),
    (dict(faults=(0.0, float("nan"), 0, 0)), b"msg_drop"),
    (dict(faults=(0.0, -1.0, 0, 0)), b"msg_drop"),
    (dict(faults=(0.0, float("inf"), 0, 0)), b"msg_drop"),
    (dict(faults=(0.0, 0.0, -1, 0)), b"fail_round"),
    (dict(faults=(0.0, 0.0, 0, 1)), b"reserved"),
    # every check of gp_ensemble_create still applies
    (dict(nseeds=0), b"nseeds"),
    (dict(seeds=None), b"seeds"),
    (dict(num_gpus=2), b"one GPU"),
    (dict(flags=L.GP_FLAG_VIRTUAL_RANKS), b"one GPU"),
    (dict(max_rounds=0), b"max_rounds"),
    (dict(n=1, topo=L.GP_3D), b"population"),
    (dict(n=0), b"num_nodes"),
    (dict(topo=7), b"topology"),
    (dict(alg=5), b"algorithm"),
])
def test_create_refuses_bad_arguments(kw, word):
    rc, msg = _create(**kw)
    assert rc == GP_EINVAL, (kw, rc, msg)
    assert word in msg, msg


@pytest.mark.parametrize("faults", [(0.0, 0.0, 0, 0), (1.0, 1.0, 2**40, 0)])
def test_create_accepts_the_edges_of_the_ranges(faults):
    rc, msg = _create(faults=faults)
    assert rc in (0, GP_ENODEV), (rc, msg)  # refused, if at all, for the missing GPU


@pytest.mark.parametrize("topo,alg", PAIRS)
def test_create_refuses_one_node_past_the_failure_cap(topo, alg):
    cap = L.lib().gp_ensemble_faults_max_nodes(TOPOS[topo], ALGS[alg])
    rc, msg = _create(n=cap + 1, topo=TOPOS[topo], alg=ALGS[alg])
    assert rc == GP_EINVAL and b"cap" in msg, (rc, msg)
    rc, msg = _create(n=cap, topo=TOPOS[topo], alg=ALGS[alg])
    assert rc in (0, GP_ENODEV), (rc, msg)


def test_null_handle_arguments():
    lib = L.lib()
    assert lib.gp_ensemble_fault_stats(None, None) == GP_EINVAL


def test_faults_value():
    f = Faults()
    assert (f.node_fail, f.msg_drop, f.fail_round) == (0.0, 0.0, 0)
    f = Faults(0.1, msg_drop=0.2, fail_round=7)
    assert (f.node_fail, f.msg_drop, f.fail_round) == (0.1, 0.2, 7) and "0.2" in repr(f)
