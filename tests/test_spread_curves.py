"""CPU: the pure functions of tools/spread_curves.py on synthetic rows -- the numbers of the table
are what their definitions say."""
import csv
import importlib.util
import math
import os

import numpy as np

from tests import trace_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("spread_curves", os.path.join(ROOT, "tools", "spread_curves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rows(*r):
    return np.array(list(r), trace_ref.ROW)


# P = 10, stride 2: reached 1, 5, 9, 10, 10
A = rows((2, 1, 0, 1, 4.5), (4, 5, 0, 9, 2.0), (6, 9, 1, 30, 1e-4), (8, 10, 4, 61, 1e-7), (10, 10, 10, 93, 1e-7))


def test_rounds_to_reach():
    sc = load_tool()
    assert sc.rounds_to_reach(A, 10) == [4, 6, 8, 8]            # 50 % = 5, 90 % = 9, 99 % -> 10, 100 % = 10
    assert sc.rounds_to_reach(A[:3], 10) == [4, 6, None, None]  # never got to everybody
    assert sc.rounds_to_reach(A[:0], 10) == [None] * 4
    assert sc.rounds_to_reach(A, 1000, (0.001, 0.0101)) == [2, None]  # 1 node; ceil(10.1) = 11 nodes
    assert sc.rounds_to_reach(rows((1, 3, 0, 1, 0.0)), 3, (0.5,)) == [1]  # ceil(1.5) = 2 <= 3


def test_messages_and_error():
    sc = load_tool()
    assert sc.messages_to_full_reach(A, 10) == 6.1 and sc.messages_to_full_reach(A[:3], 10) is None
    assert sc.rounds_to_error(A) == [6, 8, None]
    nan, inf = float("nan"), float("inf")
    B = rows((1, 1, 0, 1, inf), (2, 1, 0, 2, nan), (3, 1, 0, 3, 5e-10), (4, 1, 0, 4, nan))
    assert sc.rounds_to_error(B) == [3, 3, 3]                   # a NaN or inf is above every tolerance
    assert sc.rounds_to_error(B[:2]) == [None, None, None]
    assert sc.rounds_to_error(rows((7, 1, 0, 1, 0.0))) == [7, 7, 7]  # gossip rows would read so: not printed


def test_spread_and_cells():
    sc = load_tool()
    assert sc.spread([None, None]) == (None, None, None, 0)
    assert sc.spread([5]) == (5, 5, 5, 1)
    vals = list(range(1, 102))                                  # 1..101: nearest ranks 51, 6, 96
    assert sc.spread(vals[::-1] + [None]) == (51, 6, 96, 101)
    assert sc.cell((51, 6, 96, 101)) == "51 [6-96]" and sc.cell((None, None, None, 0)) == "-"
    assert sc.cell((6.125, 6.0, 7.5, 3), ".1f") == "6.1 [6.0-7.5]"


def test_median_curve_and_csv(tmp_path):
    sc = load_tool()
    nan = float("nan")
    t1 = rows((2, 1, 0, 1, 4.0), (4, 3, 0, 5, 2.0), (6, 4, 4, 9, 1.0))
    t2 = rows((2, 2, 0, 2, 3.0), (4, 4, 4, 6, nan))             # ended after round 4: keeps its last row
    t3 = rows((2, 3, 1, 3, nan))
    t4 = rows()                                                 # ended before its first row: left out
    curve = sc.median_curve([t1, t2, t3, t4], 2)
    assert [c[0] for c in curve] == [2, 4, 6]
    assert curve[0] == (2, 2, 0, 2, 3.0)                        # err: nearest-rank median of [3, 4]: rank round(0.5) = 0
    assert curve[1][:4] == (4, 3, 1, 5) and curve[1][4] == 2.0  # rows (4,3,0,5) (4,4,4,6) (2,3,1,3); the NaNs leave err
    assert curve[2][:4] == (6, 4, 4, 6) and curve[2][4] == 1.0
    assert sc.median_curve([t4], 2) == [] and sc.median_curve([], 1) == []
    only_nan = sc.median_curve([t3], 2)
    assert len(only_nan) == 1 and math.isnan(only_nan[0][4])
    path = tmp_path / "curves.csv"
    sc.write_csv(path, {("push-sum", "3D"): curve, ("gossip", "line"): curve[:1]})
    got = list(csv.reader(open(path)))
    assert got[0] == ["algorithm", "topology", "round", "reached", "alerts", "sent", "err_max"]
    assert got[1] == ["push-sum", "3D", "2", "2", "0", "2", "3.0"] and got[4] == ["gossip", "line", "2", "2", "0", "2", "3.0"]
    assert len(got) == 5


def test_pair_numbers():
    sc = load_tool()
    short = A[:3]
    ps = sc.pair_numbers([A, A, short], 10, push_sum=True)
    assert set(ps) == {"r50", "r90", "r99", "r100", "msg_per_node", "e3", "e6", "e9"}
    assert ps["r50"] == (4, 4, 4, 3) and ps["r100"] == (8, 8, 8, 2) and ps["msg_per_node"] == (6.1, 6.1, 6.1, 2)
    assert ps["e3"] == (6, 6, 6, 3) and ps["e6"] == (8, 8, 8, 2) and ps["e9"] == (None, None, None, 0)
    go = sc.pair_numbers([A], 10, push_sum=False)
    assert set(go) == {"r50", "r90", "r99", "r100", "msg_per_node"}


def test_on_reference_rows():
    """The tool's numbers on a real (reference) trace: every node is reached by the end, and the
    messages per node up to there are the row's."""
    sc = load_tool()
    r, rounds, _, _ = trace_ref.trace(27, "Imp3D", "gossip", 1, 1, 0, 400, None)
    reach = sc.rounds_to_reach(r, 27)
    assert reach == sorted(reach) and reach[3] <= rounds
    assert r["reached"][reach[3] - 1] == 27 and r["reached"][reach[3] - 2] < 27
    assert sc.messages_to_full_reach(r, 27) == r["sent"][reach[3] - 1] / 27
