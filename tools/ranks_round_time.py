"""Wall time per round of a run over virtual ranks, for comparing two builds (experiment tool).

    python tools/ranks_round_time.py --root <checkout with built libraries> --tag NAME --case CASE

Loads gossipprotocol_amd from --root (this checkout, or another one built from another commit),
runs CASE on four in-process ranks of device 0 and prints one JSON line: ms per round over
--windows windows of --window rounds after --warmup rounds (host clock around step + sync; a
window the run converges in is dropped), the round kernel's ms per launch (kernel timing), the
device memory the handle took (hipMemGetInfo before and after create), and a digest of what was
computed (every round's alert count, the first 2 M and last 1 M nodes' state).  Run the two
builds alternately in one session and compare like windows; equal digests say they computed the
same.  profiles/xkind/timing.txt is a record.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--case", required=True, choices=["gossip_tile", "gossip_tile_big", "pushsum", "gossip_col", "full_gossip"])
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--window", type=int, default=100)
ap.add_argument("--windows", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
CASES = {  # nodes, topology, algorithm, virtual ranks, experiments build, env
    "gossip_tile": (199 ** 3, "Imp3D", "gossip", 4, False, {}),
    "gossip_tile_big": (400 ** 3, "Imp3D", "gossip", 4, True, {"GP_KERNEL": "tile"}),
    "gossip_col": (400 ** 3, "Imp3D", "gossip", 4, False, {}),
    "pushsum": (400 ** 3, "Imp3D", "push-sum", 4, False, {}),
    "full_gossip": (10 ** 8, "full", "gossip", 4, False, {}),
}
n, topo, alg, W, exp, env = CASES[a.case]
os.environ.update(env)
import gossipprotocol_amd as gp  # noqa: E402
from gossipprotocol_amd import _lib  # noqa: E402

assert os.path.abspath(_lib.PKG_DIR).startswith(os.path.abspath(a.root)), _lib.PKG_DIR
hip = C.CDLL("libamdhip64.so")


def free_bytes():
    f, t = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


assert hip.hipSetDevice(0) == 0
hip.hipFree(None)
f0 = free_bytes()
sim = gp.Simulation(n, topo, alg, seed=3, virtual_ranks=W, kernel_timing=True, experimental=exp)
sim.sync()
f1 = free_bytes()
h = hashlib.sha256()
alerts = sim.step(a.warmup)
h.update(repr(alerts).encode())
sim.sync()
sim.kernel_stats(reset=True)
ms = []
for _ in range(a.windows):
    t0 = time.perf_counter()
    got = sim.step(a.window)
    sim.sync()
    t1 = time.perf_counter()
    h.update(repr(got).encode())
    if len(got) < a.window:
        break
    ms.append((t1 - t0) * 1e3 / len(got))
kms, kn, kname = sim.kernel_stats()
st = sim.state(0, min(n, 2_000_000))
for k in ("c", "s", "w", "flags"):
    h.update(st[k].tobytes())
tail = sim.state(n - 1_000_000, 1_000_000)
for k in ("c", "s", "w", "flags"):
    h.update(tail[k].tobytes())
print(json.dumps({"tag": a.tag, "case": a.case, "nodes": n, "ranks": W, "rounds": sim.rounds,
                  "ms_per_round": [round(x, 4) for x in ms], "kernel": kname,
                  "kernel_ms_per_launch": round(kms / max(1, kn), 4), "handle_bytes": f0 - f1,
                  "digest": h.hexdigest()[:16]}), flush=True)
sim.close()
