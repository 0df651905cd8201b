"""GPU: summaries over the one-process-per-GPU RCCL path, as two rank processes on one MI355X
(started like tests/test_gpu_rccl_multiproc.py: a fresh child process per rank, RCCL's socket
transport, a NCCL_HOSTID per rank).  GP_SCOPE_GLOBAL is collective: every rank receives the same
bytes, equal to the reference over the oracle's whole state; GP_SCOPE_LOCAL is the rank's slab.
And the CLI's --summary line under --gpus 2."""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.summary_ref import assert_matches, ref_summary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "summary_worker.py")
EXE = os.path.join(ROOT, "gossipprotocol_amd", "gossip")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(world, n, topo, alg, seed, rounds, timeout=150):
    out = tempfile.mkdtemp(prefix="gp_summary_mp_")
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GP_BENCH_DEVICE="0",
                   NCCL_HOSTID=f"gp-rehearsal-{r}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-u", WORKER, out, str(n), topo, alg, str(seed), str(rounds)],
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      start_new_session=True))
    logs, codes = [], []
    try:
        for p in procs:  # each process has its own time limit
            o, _ = p.communicate(timeout=timeout)
            logs.append(o.decode(errors="replace")[-3000:])
            codes.append(p.returncode)
    finally:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, 9)
                p.wait()
    assert codes == [0] * world, "rank processes failed:\n" + "\n----\n".join(logs)
    return [dict(np.load(os.path.join(out, f"rank{r}.npz"))) for r in range(world)]


def as_summary(a):
    from gossipprotocol_amd import _lib as L
    return L.GpSummary.from_buffer_copy(a.tobytes())


@pytest.mark.parametrize("n,topo,alg", [(32768, "Imp3D", "push-sum"), (4099, "line", "gossip")])
def test_global_and_local_scope_over_two_ranks(n, topo, alg, oracle):
    rounds, seed = 40, 3
    recs = run_ranks(2, n, topo, alg, seed, rounds)
    orc = oracle(n, topo, alg, seed)
    want = orc.step(rounds)
    st, P, seed_node = orc.state(), orc.P, orc.seed_node
    want += orc.step(3)
    orc.close()
    aid = 1 if alg == "push-sum" else 0
    whole = ref_summary(st, 0, P, rounds, aid, seed_node, 1e-10)
    for r, rec in enumerate(recs):
        assert list(rec["alerts"]) == want, f"rank {r}: alerts differ from the oracle (summaries in between)"
        assert rec["g1"].tobytes() == recs[0]["g1"].tobytes(), "GLOBAL: every rank receives the same bytes"
        assert rec["g2"].tobytes() == rec["g1"].tobytes(), "two GLOBAL summaries of one state are identical"
        assert_matches(as_summary(rec["g1"]), whole, f"rank {r} GLOBAL")
        lo, cnt = int(rec["first"]), int(rec["count"])
        part = {k: v[lo:lo + cnt] for k, v in st.items()}
        assert_matches(as_summary(rec["loc"]), ref_summary(part, lo, P, rounds, aid, seed_node, 1e-10), f"rank {r} LOCAL")
    assert int(recs[0]["first"]) == 0 and int(recs[0]["count"]) == int(recs[1]["first"])
    assert int(recs[1]["first"]) + int(recs[1]["count"]) == P
    # the ranks' LOCAL summaries join to the GLOBAL one
    both = as_summary(recs[0]["loc"]).merge(as_summary(recs[1]["loc"]))
    assert_matches(both, whole, "LOCAL joined")


@pytest.mark.parametrize("n,topo,alg", [(27000, "Imp3D", "push-sum"), (27000, "Imp3D", "gossip")])
def test_cli_summary_line_under_gpus(n, topo, alg):
    """--gpus 2 --summary: the extra line appears exactly once, after the reference's lines; without
    the flag the output is the reference's contract alone."""
    base = [EXE, str(n), topo, alg, "--gpus", "2", "--device", "0"]
    start = "Gossip Starts" if alg == "gossip" else "Push Sum Starts"
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    lines = plain.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0] == start and lines[1].startswith("Convergence Time: "), plain.stdout
    assert lines[1].endswith(" ms") and "Summary" not in plain.stdout
    for flag in ("--summary", "--summary=1e-6"):
        r = subprocess.run(base + [flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 3 and lines[0] == start and lines[1].startswith("Convergence Time: "), r.stdout
        assert lines[2].startswith("Summary: rounds=") and r.stdout.count("Summary:") == 1
        kv = dict(f.split("=", 1) for f in lines[2].split()[1:])
        P = 27000 if topo == "Imp3D" else n + 1
        assert int(kv["nodes"]) == P  # the whole network, not rank 0's slab
        if alg == "push-sum":
            assert float(kv["tol"]) == (1e-10 if flag == "--summary" else 1e-6)
            assert float(kv["sum_w"]) > 0 and float(kv["est_min"]) <= float(kv["mean"]) <= float(kv["est_max"])
        else:
            assert sum(int(v) for v in kv["c_hist"].split(",")) == P
    if alg == "gossip":  # integers only: the one-GPU run prints the same line
        one = subprocess.run([EXE, str(n), topo, alg, "--summary"], capture_output=True, text=True, timeout=300)
        assert one.returncode == 0 and one.stdout.strip().splitlines()[2] == lines[2], one.stdout
