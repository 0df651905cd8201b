"""CPU tests of the ensemble boundary (gp_ensemble_*, include/gossip_hip.h): the
symbols exist, gp_member matches its C layout, the population cap covers the
report's range, and every argument check answers before any HIP call (so it works
on a host without a GPU)."""
import ctypes as C
import os
import subprocess

import pytest

from gossipprotocol_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_ensemble_max_nodes", "gp_ensemble_create", "gp_ensemble_step", "gp_ensemble_run",
         "gp_ensemble_members", "gp_ensemble_read_state", "gp_ensemble_destroy")
PAIRS = [(t, a) for t in (L.GP_LINE, L.GP_FULL, L.GP_3D, L.GP_IMP3D) for a in (L.GP_GOSSIP, L.GP_PUSHSUM)]
GP_EINVAL = -1


def test_library_exports_the_ensemble_symbols():
    raw = C.CDLL(L.LIB_PATH)
    bound = {n for n, _, _ in L.SIGNATURES}
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in bound, n


def test_member_layout_matches_c(tmp_path):
    src = tmp_path / "member.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gp_member), offsetof(gp_member, seed),'
                   'offsetof(gp_member, rounds), offsetof(gp_member, converged), offsetof(gp_member, seed_node),'
                   'offsetof(gp_member, status), offsetof(gp_member, reserved));return 0;}\n')
    exe = tmp_path / "member"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    M = L.GpMember
    assert got == [C.sizeof(M), M.seed.offset, M.rounds.offset, M.converged.offset, M.seed_node.offset,
                   M.status.offset, M.reserved.offset]


@pytest.mark.parametrize("topo,alg", PAIRS)
def test_max_nodes_covers_the_report_range(topo, alg):
    assert L.lib().gp_ensemble_max_nodes(topo, alg) >= 1000


# num_nodes caps of the four layouts (plain, trace, failure, failure + trace), computed from the LDS
# layout of gp_ensemble.hpp on the CPU.  Only full push-sum is LDS-bound in every layout.
CAPS = {(L.GP_LINE, L.GP_GOSSIP): 8191, (L.GP_LINE, L.GP_PUSHSUM): 8191, (L.GP_FULL, L.GP_GOSSIP): 8191,
        (L.GP_3D, L.GP_GOSSIP): 8000, (L.GP_3D, L.GP_PUSHSUM): 8000, (L.GP_IMP3D, L.GP_GOSSIP): 8000,
        (L.GP_IMP3D, L.GP_PUSHSUM): 5832, (L.GP_FULL, L.GP_PUSHSUM): (6979, 6978, 6940, 6939)}


@pytest.mark.parametrize("topo,alg", PAIRS)
def test_the_caps_of_every_layout_are_what_they_were(topo, alg):
    lib = L.lib()
    want = CAPS[topo, alg]
    want = want if isinstance(want, tuple) else (want,) * 4
    got = (lib.gp_ensemble_max_nodes(topo, alg), lib.gp_ensemble_trace_max_nodes(topo, alg, 0),
           lib.gp_ensemble_faults_max_nodes(topo, alg), lib.gp_ensemble_trace_max_nodes(topo, alg, 1))
    assert got == want


def test_max_nodes_refuses_unknown_pair():
    lib = L.lib()
    assert lib.gp_ensemble_max_nodes(4, L.GP_GOSSIP) == GP_EINVAL
    assert b"topology" in lib.gp_last_error()
    assert lib.gp_ensemble_max_nodes(-1, L.GP_GOSSIP) == GP_EINVAL
    assert lib.gp_ensemble_max_nodes(L.GP_LINE, 2) == GP_EINVAL
    assert b"algorithm" in lib.gp_last_error()


def test_python_wrapper_reports_the_cap():
    from gossipprotocol_amd import ensemble_max_nodes
    assert ensemble_max_nodes("Imp3D", "push-sum") == L.lib().gp_ensemble_max_nodes(L.GP_IMP3D, L.GP_PUSHSUM)


def _create(n=100, topo=L.GP_3D, alg=L.GP_PUSHSUM, seeds=(1, 2), nseeds=None, num_gpus=1, flags=0, max_rounds=1000):
    cfg = L.GpConfig()
    cfg.num_nodes, cfg.topology, cfg.algorithm = n, topo, alg
    cfg.num_gpus, cfg.device, cfg.max_rounds, cfg.flags = num_gpus, 0, max_rounds, flags
    arr = None if seeds is None else (C.c_uint64 * max(1, len(seeds)))(*seeds)
    h = C.c_void_p()
    n_arg = nseeds if nseeds is not None else (len(seeds) if seeds is not None else 2)
    rc = L.lib().gp_ensemble_create(C.byref(cfg), arr, n_arg, C.byref(h))
    if rc == 0:  # (a GPU is present and the arguments were fine)
        L.lib().gp_ensemble_destroy(h)
    return rc, L.lib().gp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(nseeds=0), b"nseeds"),
    (dict(nseeds=-3), b"nseeds"),
    (dict(seeds=None), b"seeds"),
    (dict(num_gpus=2), b"one GPU"),
    (dict(num_gpus=0), b"one GPU"),
    (dict(flags=L.GP_FLAG_VIRTUAL_RANKS), b"one GPU"),
    (dict(max_rounds=0), b"max_rounds"),
    (dict(max_rounds=-1), b"max_rounds"),
    (dict(n=1, topo=L.GP_3D), b"population"),   # P = 1: the oracle's push-sum never converges there
    (dict(n=0), b"num_nodes"),
    (dict(topo=7), b"topology"),
    (dict(alg=5), b"algorithm"),
])
def test_create_refuses_bad_arguments(kw, word):
    rc, msg = _create(**kw)
    assert rc == GP_EINVAL, (kw, rc, msg)
    assert word in msg, msg


@pytest.mark.parametrize("topo,alg", PAIRS)
def test_create_refuses_one_node_past_the_cap(topo, alg):
    cap = L.lib().gp_ensemble_max_nodes(topo, alg)
    rc, msg = _create(n=cap + 1, topo=topo, alg=alg)
    assert rc == GP_EINVAL and b"cap" in msg, (rc, msg)
    # the cap itself passes the argument checks: it is refused, if at all, for the missing GPU
    rc, msg = _create(n=cap, topo=topo, alg=alg)
    assert rc in (0, -6), (rc, msg)
