"""CPU: tools/aggregate.py through --backend ref on 60 values and three seeds: the printed mean and
rounds are ValueSim's (tests/values_ref.py)."""
import math
import os
import subprocess
import sys

import numpy as np

from tests import values_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tool_prints_the_reference_mean_and_rounds(tmp_path):
    x = 0.1 * (np.arange(60) + 1.0)
    w = 1.0 + 0.5 * (np.arange(60) % 3)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "w.npy", w)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate.py"), "--values", str(tmp_path / "x.npy"),
                          "--weights", str(tmp_path / "w.npy"), "--topology", "full", "--seeds", "3", "--stride", "10",
                          "--max-rounds", "300", "--backend", "ref"], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    mean = math.fsum(x.tolist()) / math.fsum(w.tolist())
    assert f"mean {mean!r}" in lines
    sims = [V.ValueSim(59, "full", x, w, seed, max_rounds=300).run() for seed in (1, 2, 3)]
    assert all(s.mean == mean for s in sims)
    rounds = [s.round for s in sims]
    line = [l for l in lines if l.startswith("rounds ")][0]
    assert line.endswith("per seed: " + " ".join(map(str, rounds))), line
    assert line.split()[1] == str(sorted(rounds)[1])  # the median
    errs = sorted(V.ref_summary(s.state(), 0, s.P, s.round, s.seed_node, 0.0, mean)["err_max"] for s in sims)
    assert [l for l in lines if l.startswith("err_max ")][0].split()[1] == f"{errs[1]:.3e}"
    curve = lines[lines.index("round  median err_max  median reached") + 1:]
    assert len(curve) == max(rounds) // 10 and curve[0].split()[0] == "10"


def test_tool_refuses_a_count_that_is_no_population(tmp_path):
    np.save(tmp_path / "x.npy", np.ones(60))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate.py"), "--values", str(tmp_path / "x.npy"),
                        "--topology", "3D", "--backend", "ref"], capture_output=True, text=True)
    assert r.returncode != 0 and "cube" in r.stderr
