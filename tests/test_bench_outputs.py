"""bench.py --dump-outputs and the plain / --full split.

The window sampling is checked on the host against a stand-in for Simulation; the
GPU case runs a small bench.py and compares what it dumped with the oracle."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ("alerts", "state_index", "state_c", "state_s", "state_w", "state_flags")


class FakeSim:
    """info() / state() of a slab whose node i holds c = i mod 1000, s = i, w = i / 2, flags = i mod 4."""

    def __init__(self, first, count):
        self.first, self.count, self.reads = first, count, []

    def info(self):
        return SimpleNamespace(slab_first=self.first, slab_count=self.count)

    def state(self, first, count):
        assert self.first <= first and first + count <= self.first + self.count
        self.reads.append((first, count))
        i = np.arange(first, first + count, dtype=np.int64)
        return {"c": (i % 1000).astype(np.int32), "s": i.astype(np.float64), "w": i / 2.0,
                "flags": (i % 4).astype(np.uint8)}


def load(d, suffix=""):
    return {k: np.load(os.path.join(d, k + suffix + ".npy")) for k in NAMES}


def test_dump_small_slab_is_whole(tmp_path):
    sim = FakeSim(0, 27000)
    bench.dump_outputs(sim, [0, 3, 5], str(tmp_path), 0, 1)
    got = load(tmp_path)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["alerts"].tolist() == [0.0, 3.0, 5.0]
    assert np.array_equal(got["state_index"], np.arange(27000.0))
    assert np.array_equal(got["state_s"], got["state_index"]) and np.array_equal(got["state_w"], got["state_index"] / 2)
    assert np.array_equal(got["state_c"], got["state_index"] % 1000)
    assert np.array_equal(got["state_flags"], got["state_index"] % 4)


def test_dump_large_slab_is_a_fixed_sample(tmp_path):
    """10^9 nodes: 64 disjoint windows inside the slab, first and last node included, the same
    windows on every call, under 64 MB in all; rank 1's files carry its suffix."""
    P, half = 10**9, 5 * 10**8
    for d in ("a", "b"):
        bench.dump_outputs(FakeSim(0, P), [1], str(tmp_path / d), 0, 1)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    idx = a["state_index"]
    assert idx.size == bench.DUMP_WINDOWS * bench.DUMP_WINDOW_NODES
    assert idx[0] == 0 and idx[-1] == P - 1 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["state_s"], idx) and np.array_equal(a["state_flags"], idx % 4)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10**6
    sim = FakeSim(half, half)
    bench.dump_outputs(sim, [1], str(tmp_path / "r"), 1, 2)
    r = load(tmp_path / "r", "_rank1")
    assert r["state_index"][0] == half and r["state_index"][-1] == P - 1 and len(sim.reads) == bench.DUMP_WINDOWS
    # a slab one window past the threshold still fits 62 distinct middle windows
    edge = (bench.DUMP_WINDOWS + 1) * bench.DUMP_WINDOW_NODES
    bench.dump_outputs(FakeSim(0, edge), [1], str(tmp_path / "e"), 0, 1)
    e = load(tmp_path / "e")["state_index"]
    assert e[0] == 0 and e[-1] == edge - 1 and np.all(np.diff(e) > 0)


@pytest.mark.gpu
def test_plain_bench_dumps_the_oracles_state(tmp_path, oracle):
    """A plain run measures nothing beyond its rounds, runs exactly --steps timed rounds, and what
    it dumps is the oracle's alerts and state after the same number of rounds."""
    n, steps, warmup = 27000, 6, 3
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--nodes", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0
    assert abs(out["value"] - out["config"]["population"] * 1e3 / out["ms_per_step"]) <= 1e-9 * out["value"]
    assert out["cpu_baseline"] is None and out["akka_baseline"] is None and out["roofline"]["traffic"] is None
    got = load(tmp_path)
    orc = oracle(n, "Imp3D", "push-sum", 1)
    orc.step(out["config"]["activation_preroll_rounds"] + warmup)
    assert got["alerts"].tolist() == [float(a) for a in orc.step(steps)]
    want, P = orc.state(), orc.P
    orc.close()
    assert np.array_equal(got["state_index"], np.arange(float(P)))
    for k in ("c", "s", "w", "flags"):
        assert np.array_equal(got["state_" + k], want[k].astype(np.float64)), k
