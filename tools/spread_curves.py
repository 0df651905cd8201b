"""Spread curves: how gossip and push-sum get to their end, round by round, from the traces the
ensemble kernels record (SRS v1-T).

    python tools/spread_curves.py --nodes 1000 --seeds 256 [--stride S]
        [--node-fail p --msg-drop q --fail-round r] [--csv PATH]

For each of the eight algorithm x topology pairs one traced ensemble
(gossipprotocol_amd.Ensemble(..., trace=Trace(stride)): one workgroup per seed, a 32-byte row per
`stride` rounds) is run to its end and one line is printed, every cell the median over the seeds
with the 5-95 % range in brackets ('-': no member got there):

  r50 r90 r99 r100   rounds until 50 / 90 / 99 / 100 % of the P nodes are reached (gossip: know the
                     rumour; push-sum: are active), i.e. the round of the first recorded row that
                     shows it -- exact at stride 1, late by less than a stride otherwise
  msg/node           node-to-node messages sent per node up to that r100 row
  e-3 e-6 e-9        push-sum: rounds until the worst estimate error err_max is <= 1e-3 / 1e-6 / 1e-9
                     (a NaN or inf err_max, a weight lost to 0 under message loss, is above all)

--csv writes the per-round median curve of every pair: for row k the median over the members of
reached, alerts, sent and err_max; a member that has ended keeps its last row (its state no longer
changes), one without rows yet is left out.
"""
import argparse
import csv
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOPOLOGIES = ("line", "full", "3D", "Imp3D")
ALGORITHMS = ("gossip", "push-sum")
FRACTIONS = (0.5, 0.9, 0.99, 1.0)
TOLERANCES = (1e-3, 1e-6, 1e-9)


# ---------------------------------------------------------------- rows -> numbers (pure; tests/test_spread_curves.py)
def quantile(sorted_vals, q):
    """Nearest-rank quantile of an ascending list."""
    k = min(len(sorted_vals) - 1, max(0, int(round(q * (len(sorted_vals) - 1)))))
    return sorted_vals[k]


def first_row(hit):
    """Index of the first true entry of a boolean array over the rows, or None."""
    k = int(np.argmax(hit)) if len(hit) else 0
    return k if len(hit) and hit[k] else None


def rounds_to_reach(rows, population, fractions=FRACTIONS):
    """Per fraction: the round of the first row with reached >= ceil(fraction * population), or None."""
    out = []
    for f in fractions:
        need = min(population, max(1, math.ceil(f * population - 1e-9)))
        k = first_row(rows["reached"] >= need)
        out.append(None if k is None else int(rows[k]["round"]))
    return out


def messages_to_full_reach(rows, population):
    """sent / population at the first row that shows every node reached, or None."""
    k = first_row(rows["reached"] >= population)
    return None if k is None else int(rows[k]["sent"]) / population


def rounds_to_error(rows, tolerances=TOLERANCES):
    """Per tolerance: the round of the first row with err_max <= tol (never true of a NaN), or None."""
    out = []
    for tol in tolerances:
        k = first_row(rows["err_max"] <= tol)
        out.append(None if k is None else int(rows[k]["round"]))
    return out


def spread(values):
    """(median, 5 %, 95 %, members) over the values that are not None; all None if there is none."""
    v = sorted(x for x in values if x is not None)
    if not v:
        return None, None, None, 0
    return quantile(v, 0.5), quantile(v, 0.05), quantile(v, 0.95), len(v)


def median_curve(traces, stride):
    """Per row index k the tuple (round, reached, alerts, sent, err_max): round = (k + 1) * stride, the
    rest medians over the members; a member with fewer than k + 1 rows keeps its last one, a member
    without rows is left out.  err_max: the median of the values that are not NaN (nan if all are)."""
    have = [t for t in traces if len(t)]
    K = max((len(t) for t in have), default=0)
    if not K:
        return []
    # members x K, each member's last row carried forward; sorted down the members (NaN sorts last)
    at = np.stack([t[np.minimum(np.arange(K), len(t) - 1)] for t in have])
    mid = int(round(0.5 * (len(have) - 1)))  # quantile()'s nearest rank
    cols = [np.sort(at[f], axis=0)[mid] for f in ("reached", "alerts", "sent")]
    err = np.sort(at["err_max"], axis=0)
    valid = (~np.isnan(err)).sum(axis=0)
    emid = np.rint(0.5 * (np.maximum(valid, 1) - 1)).astype(np.int64)
    emed = np.where(valid > 0, err[emid, np.arange(K)], np.nan)
    return [((k + 1) * stride, int(cols[0][k]), int(cols[1][k]), int(cols[2][k]), float(emed[k])) for k in range(K)]


def pair_numbers(traces, population, push_sum):
    """The printed cells of one pair from its members' rows: a dict of spread() tuples."""
    reach = [rounds_to_reach(t, population) for t in traces]
    out = {f"r{int(f * 100)}": spread(r[i] for r in reach) for i, f in enumerate(FRACTIONS)}
    out["msg_per_node"] = spread(messages_to_full_reach(t, population) for t in traces)
    if push_sum:
        errs = [rounds_to_error(t) for t in traces]
        for i, tol in enumerate(TOLERANCES):
            out[f"e{int(round(-math.log10(tol)))}"] = spread(e[i] for e in errs)
    return out


def cell(sp, spec="d"):
    med, lo, hi, _ = sp
    return "-" if med is None else f"{med:{spec}} [{lo:{spec}}-{hi:{spec}}]"


def write_csv(path, curves):
    """curves: {(algorithm, topology): median_curve(...)}."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["algorithm", "topology", "round", "reached", "alerts", "sent", "err_max"])
        for (alg, topo), curve in curves.items():
            for row in curve:
                w.writerow([alg, topo] + [repr(x) if isinstance(x, float) else x for x in row])


# ---------------------------------------------------------------- the runs
def traces_gpu(n, topo, alg, seeds, stride, faults, max_rounds, device):
    from gossipprotocol_amd import Ensemble, Faults, Trace
    fa = Faults(*faults) if faults else None
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, device=device, faults=fa, trace=Trace(stride)) as ens:
        ens.run()
        return ens.population, [ens.trace(m) for m in range(len(seeds))]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--seeds", type=int, default=256, help="members per ensemble: seeds 1..K")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--topologies", nargs="+", default=list(TOPOLOGIES), choices=TOPOLOGIES)
    ap.add_argument("--algorithms", nargs="+", default=list(ALGORITHMS), choices=ALGORITHMS)
    ap.add_argument("--node-fail", type=float, default=0.0)
    ap.add_argument("--msg-drop", type=float, default=0.0)
    ap.add_argument("--fail-round", type=int, default=0)
    ap.add_argument("--max-rounds", type=int, default=50_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--csv", default=None, help="file for the per-round median curves")
    a = ap.parse_args(argv)
    seeds = list(range(1, a.seeds + 1))
    faults = (a.node_fail, a.msg_drop, a.fail_round) if (a.node_fail or a.msg_drop) else None

    print(f"n={a.nodes} seeds={a.seeds} stride={a.stride} faults={faults}: median [5%-95%] over the seeds", flush=True)
    print(f"{'algorithm':9s} {'topology':8s} {'r50':>20s} {'r90':>20s} {'r99':>20s} {'r100':>20s} {'msg/node':>22s} "
          f"{'e-3':>20s} {'e-6':>20s} {'e-9':>20s}", flush=True)
    curves, table = {}, []
    for alg in a.algorithms:
        for topo in a.topologies:
            population, traces = traces_gpu(a.nodes, topo, alg, seeds, a.stride, faults, a.max_rounds, a.device)
            nums = pair_numbers(traces, population, alg == "push-sum")
            cells = [cell(nums[k]) for k in ("r50", "r90", "r99", "r100")] + [cell(nums["msg_per_node"], ".1f")]
            cells += [cell(nums[k]) if k in nums else "" for k in ("e3", "e6", "e9")]
            print(f"{alg:9s} {topo:8s} " + " ".join(f"{c:>{22 if i == 4 else 20}s}" for i, c in enumerate(cells)), flush=True)
            curves[(alg, topo)] = median_curve(traces, a.stride)
            table.append((alg, topo, nums))
    if a.csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.csv)), exist_ok=True)
        write_csv(a.csv, curves)
    return table


if __name__ == "__main__":
    main()
