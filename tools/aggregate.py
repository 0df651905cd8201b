"""Aggregate your own data with push-sum: how many rounds it takes on a topology, and how wrong the
estimate is at that point, over many seeds and optionally under failures (SRS v1-V).

    python tools/aggregate.py --values FILE.npy [--weights FILE.npy] --topology Imp3D --seeds 256
        [--node-fail p --msg-drop q --fail-round r] [--stride k] [--max-rounds R] [--backend gpu|ref]

FILE.npy holds the P values (P = n + 1 for line / full, a cube for 3D / Imp3D; negative data has to
be shifted first, see include/gossip_hip.h for what is admissible).  One ensemble
(gossipprotocol_amd.Ensemble(..., values=Values(x, w))) runs every seed to its end, within the
ensemble's population cap.  Printed: the mean (math.fsum(x) / math.fsum(w): correctly rounded sums,
one division), the distribution over the seeds of the rounds run and of the final err_max (the
worst |s / w - mean| over the nodes), each as median [5 %-95 %], and with --stride k the median
error-decay curve, one line per k rounds.  --backend ref runs the same through the pure-Python
reference (tests/values_ref.py): small inputs only, no GPU needed.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.spread_curves import cell, median_curve, spread  # noqa: E402


def nodes_for(count, topology):
    """num_nodes whose population is `count`, or None."""
    if topology in ("line", "full"):
        return count - 1 if count >= 2 else None
    g = round(count ** (1.0 / 3.0))
    return count if g ** 3 == count else None


def run_gpu(n, topology, x, w, mean, seeds, max_rounds, faults, stride):
    """Per seed (rounds, final err_max, trace rows or None) from one ensemble."""
    from gossipprotocol_amd import Ensemble, Faults, Trace, Values
    f = Faults(*faults) if faults else None
    with Ensemble(n, topology, "push-sum", seeds, max_rounds, faults=f, trace=Trace(stride) if stride else None,
                  values=Values(x, w, mean=mean)) as e:
        recs = e.run()
        sums = e.summary()
        return [(r.rounds, sums[m].err_max, e.trace(m) if stride else None) for m, r in enumerate(recs)]


def run_ref(n, topology, x, w, mean, seeds, max_rounds, faults, stride):
    """The same from tests/values_ref.py's ValueSim."""
    from tests import values_ref as V
    out = []
    for seed in seeds:
        mk = lambda: V.ValueSim(n, topology, x, w, seed, mean, *(faults or (0.0, 0.0, 0)), max_rounds=max_rounds)  # noqa: E731
        rows = V.trace_rows(mk(), stride)[0] if stride else None
        sim = mk().run()
        err = V.ref_summary(sim.state(), 0, sim.P, sim.round, sim.seed_node, 0.0, mean)["err_max"]
        out.append((sim.round, err, rows))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--values", required=True)
    ap.add_argument("--weights")
    ap.add_argument("--topology", required=True, choices=("line", "full", "3D", "Imp3D"))
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--node-fail", type=float, default=0.0)
    ap.add_argument("--msg-drop", type=float, default=0.0)
    ap.add_argument("--fail-round", type=int, default=0)
    ap.add_argument("--stride", type=int, default=0)
    ap.add_argument("--max-rounds", type=int, default=20000)
    ap.add_argument("--backend", choices=("gpu", "ref"), default="gpu")
    a = ap.parse_args(argv)
    x = np.load(a.values).astype(np.float64).ravel()
    w = np.load(a.weights).astype(np.float64).ravel() if a.weights else None
    if w is not None and len(w) != len(x):
        ap.error(f"{len(x)} values but {len(w)} weights")
    n = nodes_for(len(x), a.topology)
    if n is None:
        ap.error(f"{len(x)} values are no population of the {a.topology} topology (line / full: n + 1; 3D / Imp3D: a cube)")
    mean = math.fsum(x.tolist()) / (math.fsum(w.tolist()) if w is not None else len(x))
    faults = (a.node_fail, a.msg_drop, a.fail_round) if (a.node_fail or a.msg_drop) else None
    seeds = list(range(1, a.seeds + 1))
    res = (run_gpu if a.backend == "gpu" else run_ref)(n, a.topology, x, w, mean, seeds, a.max_rounds, faults, a.stride)
    print(f"push-sum over {len(x)} values on {a.topology}, {len(seeds)} seeds"
          + (f", node_fail {a.node_fail} msg_drop {a.msg_drop} from round {a.fail_round}" if faults else ""))
    print(f"mean {mean!r}")
    print("rounds " + cell(spread(r for r, _, _ in res)) + "  per seed: " + " ".join(str(r) for r, _, _ in res[:16])
          + (" ..." if len(res) > 16 else ""))
    errs = [e for _, e, _ in res if not math.isnan(e)]
    print("err_max " + cell(spread(errs), ".3e") + (f"  ({len(res) - len(errs)} members ended with a NaN estimate)" if len(errs) < len(res) else ""))
    if a.stride:
        print("round  median err_max  median reached")
        for rnd, reached, _, _, err in median_curve([t for _, _, t in res], a.stride):
            print(f"{rnd:5d}  {err:.6e}  {reached}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
