"""Failure curves: how gossip and push-sum behave when nodes crash and messages are lost
(SRS v1-F).

    python tools/failure_curves.py --nodes 1000 --seeds 256 --node-fail 0 0.01 0.05 0.1 0.2 \\
        --msg-drop 0 0.01 0.05 0.1 0.2 [--fail-round R] [--backend gpu|ref] [--out DIR]

For every algorithm x topology x node count x node_fail x msg_drop one ensemble with a failure
model (gossipprotocol_amd.Ensemble(..., faults=Faults(...)): one workgroup per seed) is run to
its end and one row is printed:

  conv       the fraction of members that converged (reached T_f counted alerts by --max-rounds)
  med / p90  median and 90th-percentile rounds of the members that converged ('-' if none)
  est err    push-sum: median over the members of |mean survivor estimate - mu| / mu, mu = (P-1)/2.
             The mean is taken of s / w over the survivors -- the nodes that are not down (state()
             flag bit 4 clear) -- that still hold an estimate, i.e. have w > 0: a node that sent into
             the void for a thousand rounds has halved its weight down to 0 and s / w is 0 / 0.
             A member in which no survivor holds an estimate (thousands of rounds under loss end
             like that, converged or not) has no estimate either: it is left out of the median and counted
             in the next column; '-' if no member holds one.
  no est     push-sum: the members left out of est err for that reason
  mass       push-sum: median over all members of sum(w) / P, the sum over all survivors (w = 0
             included): what the lost messages left of the network's weight

--backend ref runs the same sweep through the pure-Python reference (tests/faults_ref.py) on
the CPU -- slow, for small sweeps and for testing the table code without a GPU.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOPOLOGIES = ("line", "full", "3D", "Imp3D")
ALGORITHMS = ("gossip", "push-sum")
CONVERGED, DOWN = 0, 0x10


def quantile(sorted_vals, q):
    """Nearest-rank quantile of an ascending list."""
    k = min(len(sorted_vals) - 1, max(0, int(round(q * (len(sorted_vals) - 1)))))
    return sorted_vals[k]


def survivors(s, w, flags):
    """(mean of s / w over the nodes without the down bit that have w > 0, or None if there is no
    such node; sum of w over all nodes without the down bit)."""
    est = [si / wi for si, wi, f in zip(s, w, flags) if not f & DOWN and wi > 0.0]
    return (sum(est) / len(est) if est else None), sum(wi for wi, f in zip(w, flags) if not f & DOWN)


def members_gpu(n, topo, alg, seeds, faults, max_rounds, device):
    """Per member (rounds, status, survivor mean estimate, survivor weight).  Gossip: both None;
    push-sum: the estimate is None for a member without one (see survivors)."""
    from gossipprotocol_amd import Ensemble, Faults
    out = []
    with Ensemble(n, topo, alg, seeds, max_rounds=max_rounds, device=device, faults=Faults(*faults)) as ens:
        recs = ens.run()
        for m, r in enumerate(recs):
            est = mass = None
            if alg == "push-sum":
                st = ens.state(m)
                est, mass = survivors(st["s"].tolist(), st["w"].tolist(), st["flags"].tolist())
            out.append((int(r.rounds), int(r.status), est, mass))
        population = ens.population
    return population, out


def members_ref(n, topo, alg, seeds, faults, max_rounds, device):
    from tests.faults_ref import FaultSim
    out, population = [], 0
    for seed in seeds:
        sim = FaultSim(n, topo, alg, seed, *faults, max_rounds=max_rounds).run()
        est = mass = None
        if alg == "push-sum":
            est, mass = survivors(sim.s, sim.w, sim.flags())
        out.append((sim.round, sim.status, est, mass))
        population = sim.P
    return population, out


def point(population, members):
    """One row of the table from the members of one ensemble.  Push-sum members have a weight
    (members[m][3] is not None); those without an estimate are left out of est_err and counted."""
    rounds = sorted(r for r, status, _, _ in members if status == CONVERGED)
    row = {"members": len(members), "converged": len(rounds), "conv_fraction": len(rounds) / len(members),
           "median_rounds": quantile(rounds, 0.5) if rounds else None,
           "p90_rounds": quantile(rounds, 0.9) if rounds else None, "est_err": None, "no_estimate": None,
           "mass": None}
    if members[0][3] is not None:
        mu = (population - 1) / 2
        errs = sorted(abs(est - mu) / mu for _, _, est, _ in members if est is not None and est == est)
        row["est_err"] = quantile(errs, 0.5) if errs else None
        row["no_estimate"] = len(members) - len(errs)
        row["mass"] = quantile(sorted(mass / population for _, _, _, mass in members), 0.5)
    return row


def fmt(v, spec):
    """format(v, spec), or a right-aligned '-' of the same width for a missing value."""
    width = int(spec.split(".")[0].rstrip("de"))
    return format("-", f">{width}s") if v is None else format(v, spec)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1000])
    ap.add_argument("--seeds", type=int, default=256, help="members per ensemble: seeds 1..S")
    ap.add_argument("--topologies", nargs="+", default=list(TOPOLOGIES), choices=TOPOLOGIES)
    ap.add_argument("--algorithms", nargs="+", default=list(ALGORITHMS), choices=ALGORITHMS)
    ap.add_argument("--node-fail", type=float, nargs="+", default=[0.0, 0.01, 0.05, 0.1, 0.2])
    ap.add_argument("--msg-drop", type=float, nargs="+", default=[0.0, 0.01, 0.05, 0.1, 0.2])
    ap.add_argument("--fail-round", type=int, default=0, help="first round in which the doomed nodes are down")
    ap.add_argument("--max-rounds", type=int, default=100_000)
    ap.add_argument("--backend", choices=("gpu", "ref"), default="gpu")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="directory for failure_curves.json")
    a = ap.parse_args(argv)
    seeds = list(range(1, a.seeds + 1))
    members_of = members_gpu if a.backend == "gpu" else members_ref

    print(f"{'algorithm':9s} {'topology':8s} {'n':>6s} {'node_fail':>9s} {'msg_drop':>9s} {'conv':>6s} {'med':>8s} "
          f"{'p90':>8s} {'est err':>10s} {'no est':>6s} {'mass':>10s}", flush=True)
    rows = []
    for alg in a.algorithms:
        for topo in a.topologies:
            for n in a.nodes:
                for nf in a.node_fail:
                    for md in a.msg_drop:
                        population, members = members_of(n, topo, alg, seeds, (nf, md, a.fail_round), a.max_rounds,
                                                         a.device)
                        row = point(population, members)
                        row.update(algorithm=alg, topology=topo, n=n, node_fail=nf, msg_drop=md,
                                   fail_round=a.fail_round, max_rounds=a.max_rounds)
                        print(f"{alg:9s} {topo:8s} {n:6d} {nf:9.4g} {md:9.4g} {row['conv_fraction']:6.3f} "
                              f"{fmt(row['median_rounds'], '8d')} {fmt(row['p90_rounds'], '8d')} "
                              f"{fmt(row['est_err'], '10.3e')} {fmt(row['no_estimate'], '6d')} {fmt(row['mass'], '10.3e')}", flush=True)
                        rows.append(row)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "failure_curves.json"), "w") as fh:
            json.dump({"seeds": a.seeds, "backend": a.backend, "rows": rows}, fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
