"""Convergence statistics over many seeds with ensemble runs.

    python tools/ensemble_stats.py --nodes 100 200 ... 1000 --seeds 256 [--sequential] [--summary] [--out DIR]

For every topology x algorithm pair and node count one ensemble (gossipprotocol_amd.Ensemble:
one workgroup per seed, all seeds at once) is run to convergence; the tool prints the median
and the 5 % / 95 % quantiles of the members' convergence rounds (the synchronous equivalent of
the reference's `Convergence Time`, Program.fs:53-55, at the node counts of its Report.pdf)
and the wall time of the ensemble: create, run and destroy.  `round us` is the run's wall
time divided by the slowest member's rounds, i.e. what one round costs inside the kernel.

--sequential also runs the same members one by one through Simulation (create, run,
destroy per seed: what a seed cost before ensembles), checks that both paths report the
same rounds for every seed, and prints the ratio of members per second.

--summary adds, per (n, pair), the median and the maximum over the seeds of the members' err_max
(Ensemble.summary: the largest |s / w - (P - 1) / 2| of a member when it stopped; 0 for gossip).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOPOLOGIES = ("line", "full", "3D", "Imp3D")
ALGORITHMS = ("gossip", "push-sum")


def quantile(sorted_vals, q):
    """Nearest-rank quantile of an ascending list."""
    k = min(len(sorted_vals) - 1, max(0, int(round(q * (len(sorted_vals) - 1)))))
    return sorted_vals[k]


def run_ensemble(n, topo, alg, seeds, max_rounds, device, summary=False):
    from gossipprotocol_amd import Ensemble
    from gossipprotocol_amd import _lib as L
    t0 = time.perf_counter()
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, device=device) as ens:
        t1 = time.perf_counter()
        recs = ens.run()
        t2 = time.perf_counter()
        errs = [m.err_max for m in ens.summary()] if summary else None  # (outside the timed run)
    t3 = time.perf_counter()
    rounds = [int(r.rounds) for r in recs]
    conv = sum(r.status == L.GP_STATUS_CONVERGED for r in recs)
    if summary:
        return rounds, conv, (t3 - t0) * 1e3, (t2 - t1) * 1e3, errs
    return rounds, conv, (t3 - t0) * 1e3, (t2 - t1) * 1e3


def run_sequential(n, topo, alg, seeds, max_rounds, device):
    from gossipprotocol_amd import Simulation
    t0 = time.perf_counter()
    rounds = []
    for sd in seeds:
        with Simulation(n, topo, alg, seed=sd, max_rounds=max_rounds, device=device) as sim:
            rounds.append(int(sim.run().rounds))
    return rounds, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=list(range(100, 1001, 100)))
    ap.add_argument("--seeds", type=int, default=256, help="members per ensemble: seeds 1..S")
    ap.add_argument("--topologies", nargs="+", default=list(TOPOLOGIES), choices=TOPOLOGIES)
    ap.add_argument("--algorithms", nargs="+", default=list(ALGORITHMS), choices=ALGORITHMS)
    ap.add_argument("--max-rounds", type=int, default=10**6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sequential", action="store_true", help="also run every member alone through Simulation")
    ap.add_argument("--summary", action="store_true", help="add the median / max over seeds of the members' err_max")
    ap.add_argument("--out", default=None, help="directory for ensemble_stats.json")
    a = ap.parse_args()
    seeds = list(range(1, a.seeds + 1))

    # first use of the device (context, code object load) is not part of any row
    run_ensemble(8, "3D", "gossip", [1], 1000, a.device)
    if a.sequential:
        run_sequential(8, "3D", "gossip", [1], 1000, a.device)

    head = f"{'algorithm':9s} {'topology':8s} {'n':>6s} {'median':>8s} {'q05':>8s} {'q95':>8s} {'max':>8s} " \
           f"{'conv':>9s} {'wall ms':>9s} {'round us':>9s}"
    if a.summary:
        head += f" {'err med':>10s} {'err max':>10s}"
    if a.sequential:
        head += f" {'seq ms':>10s} {'speedup':>8s}"
    print(head, flush=True)
    rows = []
    for alg in a.algorithms:
        for topo in a.topologies:
            for n in a.nodes:
                rounds, conv, wall_ms, run_ms, *errs = run_ensemble(n, topo, alg, seeds, a.max_rounds, a.device,
                                                                    summary=a.summary)
                srt = sorted(rounds)
                row = {"algorithm": alg, "topology": topo, "n": n, "members": len(seeds), "rounds": rounds,
                       "median_rounds": quantile(srt, 0.5), "q05_rounds": quantile(srt, 0.05),
                       "q95_rounds": quantile(srt, 0.95), "max_rounds": srt[-1], "converged": conv,
                       "ensemble_wall_ms": wall_ms, "ensemble_run_ms": run_ms,
                       "round_us": run_ms * 1e3 / max(1, srt[-1]),
                       "ensemble_members_per_s": len(seeds) / (wall_ms * 1e-3)}
                line = f"{alg:9s} {topo:8s} {n:6d} {row['median_rounds']:8d} {row['q05_rounds']:8d} " \
                       f"{row['q95_rounds']:8d} {srt[-1]:8d} {conv:5d}/{len(seeds):<3d} {wall_ms:9.2f} " \
                       f"{row['round_us']:9.3f}"
                if a.summary:
                    es = sorted(errs[0])
                    row["err_max_median"], row["err_max_max"] = quantile(es, 0.5), es[-1]
                    line += f" {row['err_max_median']:10.3e} {es[-1]:10.3e}"
                if a.sequential:
                    seq_rounds, seq_ms = run_sequential(n, topo, alg, seeds, a.max_rounds, a.device)
                    if seq_rounds != rounds:
                        raise SystemExit(f"{alg} {topo} n={n}: ensemble and Simulation disagree on the rounds")
                    row["sequential_wall_ms"] = seq_ms
                    row["sequential_members_per_s"] = len(seeds) / (seq_ms * 1e-3)
                    row["speedup"] = seq_ms / wall_ms
                    line += f" {seq_ms:10.1f} {row['speedup']:8.1f}"
                print(line, flush=True)
                rows.append(row)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "ensemble_stats.json"), "w") as fh:
            json.dump({"seeds": a.seeds, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
