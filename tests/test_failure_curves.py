"""CPU: tools/failure_curves.py on a tiny sweep through the pure-Python reference
(--backend ref): the table's columns are what their definitions say."""
import importlib.util
import json
import os

from tests.faults_ref import DOWN, FaultSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("failure_curves", os.path.join(ROOT, "tools", "failure_curves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_quantile_and_point():
    fc = load_tool()
    assert fc.quantile([1, 2, 3, 4, 5], 0.5) == 3 and fc.quantile([1, 2, 3, 4, 5], 0.9) == 5
    # four members of a P = 5 network (mu = 2): three converged; estimates off by 0, 10 %, 10 %, 50 %
    row = fc.point(5, [(10, 0, 2.0, 5.0), (30, 0, 2.2, 4.0), (20, 0, 1.8, 4.5), (99, 1, 3.0, 1.0)])
    assert (row["members"], row["converged"], row["conv_fraction"]) == (4, 3, 0.75)
    assert (row["median_rounds"], row["p90_rounds"]) == (20, 30)
    assert abs(row["est_err"] - 0.1) < 1e-12 and row["mass"] == 0.9 and row["no_estimate"] == 0
    row = fc.point(5, [(99, 1, None, None)])  # gossip, nobody converged
    assert row["conv_fraction"] == 0 and row["median_rounds"] is None and row["est_err"] is None
    assert row["no_estimate"] is None and row["mass"] is None


def test_members_without_an_estimate_leave_the_median():
    fc = load_tool()
    # a survivor with w = 0 holds no estimate and leaves the mean; its weight still counts (as 0)
    assert fc.survivors([4.0, 0.0, 9.0], [2.0, 0.0, 1.0], [0, 0, fc.DOWN]) == (2.0, 2.0)
    assert fc.survivors([0.0, 9.0], [0.0, 1.0], [0, fc.DOWN]) == (None, 0.0)
    # P = 5, mu = 2: errors 0.1, 0.2, 0.4 and two members without an estimate (None, and a NaN for
    # good measure), placed where a sort that met them would go wrong
    members = [(50, 1, None, 0.0), (10, 0, 2.8, 5.0), (50, 1, float("nan"), 0.0), (12, 0, 2.2, 4.0), (11, 0, 1.6, 3.0)]
    for order in (members, members[::-1], members[2:] + members[:2]):
        row = fc.point(5, order)
        assert abs(row["est_err"] - 0.2) < 1e-12, row
        assert row["no_estimate"] == 2 and row["mass"] == 0.6 and row["converged"] == 3
    # nobody holds an estimate: the cell is missing, not NaN
    row = fc.point(5, [(50, 1, None, 0.0), (50, 1, None, 0.0)])
    assert row["est_err"] is None and row["no_estimate"] == 2 and row["mass"] == 0.0
    assert fc.fmt(None, "8d") == "       -" and fc.fmt(None, "10.3e") == " " * 9 + "-" and fc.fmt(7, "8d") == "       7"


def test_ref_backend_table(tmp_path, capsys):
    fc = load_tool()
    rows = fc.main(["--backend", "ref", "--nodes", "8", "--seeds", "3", "--topologies", "3D", "full",
                    "--node-fail", "0", "0.25", "--msg-drop", "0", "1", "--max-rounds", "150", "--out", str(tmp_path)])
    text = capsys.readouterr().out.splitlines()
    assert len(rows) == 2 * 2 * 2 * 2 and len(text) == 1 + len(rows)
    assert text[0].split() == ["algorithm", "topology", "n", "node_fail", "msg_drop", "conv", "med", "p90", "est",
                               "err", "no", "est", "mass"]
    assert json.load(open(tmp_path / "failure_curves.json"))["rows"] == rows
    by = {(r["algorithm"], r["topology"], r["node_fail"], r["msg_drop"]): r for r in rows}
    # no faults: everybody converges, push-sum finds the mean and keeps its mass
    r = by[("push-sum", "3D", 0.0, 0.0)]
    assert r["conv_fraction"] == 1.0 and r["est_err"] < 1e-6 and abs(r["mass"] - 1.0) < 1e-12
    # every message dropped: gossip lives on the injector (3D), full gossip and push-sum never converge
    assert by[("gossip", "3D", 0.0, 1.0)]["conv_fraction"] == 1.0
    assert by[("gossip", "full", 0.0, 1.0)]["conv_fraction"] == 0.0
    r = by[("push-sum", "full", 0.0, 1.0)]
    assert (r["conv_fraction"], r["median_rounds"], r["p90_rounds"]) == (0.0, None, None) and r["mass"] < 1.0
    # one point recomputed from the reference by hand
    r = by[("push-sum", "3D", 0.25, 0.0)]
    sims = [FaultSim(8, "3D", "push-sum", s, 0.25, 0.0, 0, max_rounds=150).run() for s in (1, 2, 3)]
    conv = sorted(s.round for s in sims if s.status == 0)
    assert r["converged"] == len(conv) and r["median_rounds"] == (fc.quantile(conv, 0.5) if conv else None)
    errs, masses = [], []
    for s in sims:
        alive = [i for i, f in enumerate(s.flags()) if not f & DOWN]
        est = sum(s.s[i] / s.w[i] for i in alive) / len(alive)
        errs.append(abs(est - 3.5) / 3.5)
        masses.append(sum(s.w[i] for i in alive) / 8)
    assert r["est_err"] == sorted(errs)[1] and r["mass"] == sorted(masses)[1] and r["no_estimate"] == 0
