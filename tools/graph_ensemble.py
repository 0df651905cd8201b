"""Gossip or push-sum on your own network: how many rounds it takes, over many seeds, and for
push-sum how wrong the estimate is at that point (SRS v1-G).

    python tools/graph_ensemble.py (--edges FILE.npy [--nodes N] [--directed] | --ring N K | --torus W H |
        --star N | --watts-strogatz N K P [--graph-seed S] | --lattice3d G | --imp3d G SEED)
        --algorithm gossip|push-sum [--seeds 256] [--node-fail p --msg-drop q --fail-round r]
        [--stride k] [--max-rounds R] [--backend gpu|ref]

FILE.npy holds an (m, 2) integer array of edges (u, v); undirected unless --directed, N = the
largest id + 1 unless --nodes is given.  One ensemble (gossipprotocol_amd.Ensemble.on_graph) runs
every seed to its end.  Printed: the graph's size and the LDS image a member takes, the
distribution over the seeds of the rounds run as median [5 %-95 %], how many members converged (a
graph that is not strongly connected ends push-sum at --max-rounds), for push-sum the final err_max
(the worst |s / w - (P - 1) / 2| over the nodes), and with --stride k the median spread curve, one
line per k rounds.  --backend ref runs the same through the pure-Python reference
(tests/graph_ref.py): small graphs only, no GPU needed.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gossipprotocol_amd.graph import Graph  # noqa: E402
from tools.spread_curves import cell, median_curve, spread  # noqa: E402


def build_graph(a):
    if a.edges:
        e = np.load(a.edges).astype(np.int64).reshape(-1, 2)
        return Graph.from_edges(a.nodes or int(e.max()) + 1, e, directed=a.directed), f"{a.edges}"
    if a.ring:
        return Graph.ring(*a.ring), f"ring({a.ring[0]}, {a.ring[1]})"
    if a.torus:
        return Graph.torus(*a.torus), f"torus({a.torus[0]}, {a.torus[1]})"
    if a.star:
        return Graph.star(a.star), f"star({a.star})"
    if a.watts_strogatz:
        n, k, p = int(a.watts_strogatz[0]), int(a.watts_strogatz[1]), float(a.watts_strogatz[2])
        return Graph.watts_strogatz(n, k, p, a.graph_seed), f"watts_strogatz({n}, {k}, {p}, seed {a.graph_seed})"
    if a.lattice3d:
        return Graph.lattice3d(a.lattice3d), f"lattice3d({a.lattice3d})"
    return Graph.imp3d(*a.imp3d), f"imp3d({a.imp3d[0]}, seed {a.imp3d[1]})"


def run_gpu(graph, alg, seeds, max_rounds, faults, stride):
    """Per seed (rounds, status, final err_max, trace rows or None) from one ensemble."""
    from gossipprotocol_amd import Ensemble, Faults, Trace
    f = Faults(*faults) if faults else None
    with Ensemble.on_graph(graph, alg, seeds, max_rounds, faults=f, trace=Trace(stride) if stride else None) as e:
        recs = e.run()
        sums = e.summary()
        return [(r.rounds, r.status, sums[m].err_max, e.trace(m) if stride else None) for m, r in enumerate(recs)]


def run_ref(graph, alg, seeds, max_rounds, faults, stride):
    """The same from tests/graph_ref.py's GraphSim."""
    from tests import graph_ref as R
    from tests import values_ref as V
    out = []
    for seed in seeds:
        mk = lambda: R.GraphSim(graph, alg, seed, *(faults or (0.0, 0.0, 0)), max_rounds=max_rounds)  # noqa: E731
        rows = R.trace_rows(mk(), stride)[0] if stride else None
        sim = mk().run()
        err = 0.0
        if alg == "push-sum":
            err = V.ref_summary(sim.state(), 0, sim.P, sim.round, sim.seed_node, 0.0, sim.mean)["err_max"]
        out.append((sim.round, sim.status, err, rows))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--edges")
    src.add_argument("--ring", type=int, nargs=2, metavar=("N", "K"))
    src.add_argument("--torus", type=int, nargs=2, metavar=("W", "H"))
    src.add_argument("--star", type=int, metavar="N")
    src.add_argument("--watts-strogatz", nargs=3, metavar=("N", "K", "P"))
    src.add_argument("--lattice3d", type=int, metavar="G")
    src.add_argument("--imp3d", type=int, nargs=2, metavar=("G", "SEED"))
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--directed", action="store_true")
    ap.add_argument("--graph-seed", type=int, default=1)
    ap.add_argument("--algorithm", required=True, choices=("gossip", "push-sum"))
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--node-fail", type=float, default=0.0)
    ap.add_argument("--msg-drop", type=float, default=0.0)
    ap.add_argument("--fail-round", type=int, default=0)
    ap.add_argument("--stride", type=int, default=0)
    ap.add_argument("--max-rounds", type=int, default=20000)
    ap.add_argument("--backend", choices=("gpu", "ref"), default="gpu")
    a = ap.parse_args(argv)
    graph, name = build_graph(a)
    faults = (a.node_fail, a.msg_drop, a.fail_round) if (a.node_fail or a.msg_drop) else None
    seeds = list(range(1, a.seeds + 1))
    print(f"{a.algorithm} on {name}: {graph.num_nodes} nodes, {graph.num_edges} entries, {len(seeds)} seeds"
          + (f", node_fail {a.node_fail} msg_drop {a.msg_drop} from round {a.fail_round}" if faults else ""))
    if a.backend == "gpu":
        from gossipprotocol_amd import ensemble_graph_lds_bytes
        print(f"LDS image {ensemble_graph_lds_bytes(graph, a.algorithm, bool(faults), bool(a.stride))} bytes a member")
    res = (run_gpu if a.backend == "gpu" else run_ref)(graph, a.algorithm, seeds, a.max_rounds, faults, a.stride)
    print("rounds " + cell(spread(r[0] for r in res)) + "  per seed: " + " ".join(str(r[0]) for r in res[:16])
          + (" ..." if len(res) > 16 else ""))
    print(f"converged {sum(r[1] == 0 for r in res)} of {len(res)} (the rest ended at max_rounds {a.max_rounds})")
    if a.algorithm == "push-sum":
        errs = [r[2] for r in res if not math.isnan(r[2])]
        print("err_max " + cell(spread(errs), ".3e")
              + (f"  ({len(res) - len(errs)} members ended with a NaN estimate)" if len(errs) < len(res) else ""))
    if a.stride:
        print("round  reached  alerts  sent" + ("  median err_max" if a.algorithm == "push-sum" else ""))
        for rnd, reached, alerts, sent, err in median_curve([r[3] for r in res], a.stride):
            print(f"{rnd:5d}  {reached}  {alerts}  {sent}" + (f"  {err:.6e}" if a.algorithm == "push-sum" else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
