"""Time of the on-device state summary.

    python tools/summary_time.py [--calls 11] [--skip-large] [--out DIR]

Three measurements, all in one process on one device:

  1. Summary time at the headline size (Imp3D push-sum, 10^9 nodes) and at the C3 size (Imp3D
     gossip, 10^8): the median of --calls summaries of one state, beside the round kernel's time
     in the same run (gp_kernel_stats) and as bytes per second on the summary's 17 B per push-sum
     node / 4 B per gossip node.
  2. Summary against readback at 10^8 push-sum nodes: Simulation.summary() against
     Simulation.state() plus the numpy reduction of the same quantities.
  3. Ensemble overhead: Ensemble.summary() at n = 1000 with 256 seeds against the ensemble's run
     wall time.

A summary is timed as its caller sees it: the wall time of the call on an idle handle (the call
synchronises the stream before and after its two launches, so this is the kernels' time plus one
launch and one 224-byte copy, tens of microseconds).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(f, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def numpy_summary(st, P, tol):
    """What a caller computed from a readback before summaries existed (push-sum)."""
    est = st["s"] / st["w"]
    e = est - (P - 1) / 2
    ae = np.abs(e)
    f = st["flags"]
    return (int((f & 1).sum()), int(((f >> 1) & 1).sum()), np.bincount((f >> 2) & 3, minlength=4), est.min(), est.max(),
            st["w"].min(), st["w"].max(), ae.max(), int(np.argmax(ae)), int((ae <= tol).sum()), st["s"].sum(),
            st["w"].sum(), (e * e).sum())


def size_row(n, topo, alg, rounds, calls):
    from gossipprotocol_amd import Simulation
    with Simulation(n, topo, alg, seed=1, kernel_timing=True) as sim:
        sim.step(rounds)
        sim.kernel_stats(reset=True)
        sim.step(20)
        ms, launches, name = sim.kernel_stats()
        sim.summary()  # first use: scratch allocation, code object load
        med, lo, hi = timed(sim.summary, calls)
        m = sim.summary()
        P = sim.population
        per_node = 17.0 if alg == "push-sum" else 4.0
        return {"algorithm": alg, "topology": topo, "population": P, "rounds": int(m.rounds),
                "summary_ms_median": med, "summary_ms_min": lo, "summary_ms_max": hi, "calls": calls,
                "summary_bytes_per_node": per_node, "summary_GBps": per_node * P / (med * 1e6),
                "round_kernel": name, "round_kernel_ms": ms / max(1, launches),
                "round_alg_bytes_per_node": sim.alg_bytes_per_node(),
                "summary_over_round": med / (ms / max(1, launches)),
                "err_max": m.err_max, "active": int(m.active), "converged": int(m.converged)}


def readback_row(n, calls):
    from gossipprotocol_amd import Simulation
    with Simulation(n, "Imp3D", "push-sum", seed=1) as sim:
        sim.step(60)
        P = sim.population
        sim.summary()
        s_med, _, _ = timed(sim.summary, calls)
        r_med, _, _ = timed(lambda: numpy_summary(sim.state(), P, 1e-10), 3)
        c_med, _, _ = timed(sim.state, 3)
        return {"population": P, "summary_ms": s_med, "state_plus_numpy_ms": r_med, "state_copy_ms": c_med,
                "ratio": r_med / s_med}


def ensemble_row(calls):
    from gossipprotocol_amd import Ensemble
    rows = []
    for topo, alg in (("Imp3D", "push-sum"), ("line", "push-sum"), ("Imp3D", "gossip")):
        with Ensemble(1000, topo, alg, list(range(1, 257)), max_rounds=10**6) as ens:
            t0 = time.perf_counter()
            ens.run()
            run_ms = (time.perf_counter() - t0) * 1e3
            ens.summary()
            med, _, _ = timed(ens.summary, calls)
            sums = ens.summary()
            rows.append({"algorithm": alg, "topology": topo, "n": 1000, "members": 256, "run_ms": run_ms,
                         "summary_ms": med, "summary_over_run": med / run_ms,
                         "err_max_median": statistics.median(m.err_max for m in sums),
                         "err_max_max": max(m.err_max for m in sums)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=11, help="summaries per median (>= 10)")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 10^9 push-sum row")
    ap.add_argument("--out", default=None, help="directory for summary_time.json")
    a = ap.parse_args()
    res = {"sizes": [], "readback": None, "ensembles": None}
    sizes = [(10**8, "Imp3D", "gossip", 60)]
    if not a.skip_large:
        sizes.append((10**9, "Imp3D", "push-sum", 120))
    for n, topo, alg, rounds in sizes:
        row = size_row(n, topo, alg, rounds, a.calls)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    res["readback"] = readback_row(10**8, a.calls)
    print(json.dumps(res["readback"]), flush=True)
    res["ensembles"] = ensemble_row(a.calls)
    for row in res["ensembles"]:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "summary_time.json"), "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
