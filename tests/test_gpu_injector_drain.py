"""GPU: the gossip injector's two-chunk list through its whole drain, against the oracle's recorded
runs (tests/golden/runs_injector.json; tests/injector_record.py says what a record holds and
tests/golden/make_golden_injector.py makes it).  The oracle is not run here.

The injector (Program.fs:141-163) keeps its list as a bitmap in chunks of 65536 ids with a live
count per chunk; once per round one workgroup rank-selects a pick in it (inj_find, gp_kernels.hip)
and removes a converged pick (inj_remove).  The three recorded runs are the smallest with two
chunks -- line n = 65537 (chunk 1 holds one id) and the lattice g = 41 (T = 68921, chunk 1 holds
3385) as 3D and Imp3D; seeds in injector_record.CASES -- run to convergence, about 10^5 rounds
each: thousands of removals from chunk 1, words and then the whole chunk becoming empty while the run goes on (line: chunk 1
is empty for nearly half the run while chunk 0 holds tens of thousands), chunk_live reaching 0 and
|L| falling from T to a handful.  A wrong pick delivers a rumour to the wrong node or removes the
wrong id and shifts every later pick, so per-round alerts and `c` pin the list completely.

Every case steps its handle 2048 rounds at a time and compares, per segment, the digest of the
per-round alerts, the cumulative alerts and the digests of `c` and `flags` of all nodes, and at the
end rounds and alerts_total.  A mismatch reports the first differing segment, the fields that
differ and the list's recorded shape around it, with the segment's alerts re-hashed in 256-round
pieces for comparison with an oracle run.

Handles: the product library on one rank (all three topologies run k_gossip_tile at this size,
asserted), the column march forced on 3D (GP_KERNEL=col, experiments build) -- both round kernels
read inj_target -- and virtual ranks, where the list is replicated: k_finalize_pre picks, the owner
says whether the pick has converged, k_finalize_post removes it on every rank.  Id 65536 lies in
plane 38 of 41, inside the last slab of both the two- and the three-way split (planes 20..40 and
27..40), so the ownership test of k_finalize_pre sees picks of both chunks on the last rank and
picks of chunk 0 on every rank.

Wall times on an MI355X: profiles/injector_drain/pytest_gpu.txt (1.3 to 1.6 s on one rank with the
product kernel, 3.5 to 11.8 s otherwise).  A case that takes more than 20 s there runs with
GP_BASELINE_FULL=1 only (FULL_ONLY; none does); the three single-rank product cases and the line
on two virtual ranks always run.
"""
import hashlib
import os

import numpy as np
import pytest

from tests import injector_record as rec
from tests.test_gpu_parity import Sim

pytestmark = pytest.mark.gpu

TILE, COL = "k_gossip_tile", "k_gossip_col"
PRODUCT_KERNEL = TILE   # plan_variant (gp_kernel_plan.hpp): the column march from g = 200 on
PIECE = 256

# (record, virtual ranks, forced kernel or None)
RUNS = [("line", 1, None), ("line", 2, None),
        ("3D", 1, None), ("3D", 1, "col"), ("3D", 2, None),
        ("Imp3D", 1, None), ("Imp3D", 2, None), ("Imp3D", 3, None)]
FULL_ONLY = set()   # members of RUNS measured above 20 s (module docstring)


def run_id(r):
    return f"{r[0]}-ranks{r[1]}-{r[2] or 'product'}"


def describe(case, i, fields, alerts):
    """The report of the first differing segment i."""
    lo, hi = i * rec.SEG, min((i + 1) * rec.SEG, case["rounds"])
    before = (case["listed"][i - 1], case["live"][i - 1]) if i else ([min(rec.INJ_CHUNK, case["threshold"]),
                                                                     case["threshold"] - rec.INJ_CHUNK], case["threshold"])
    pieces = [(lo + k, sum(alerts[k:k + PIECE]), hashlib.sha256(np.asarray(alerts[k:k + PIECE], "<i8").tobytes()).hexdigest()[:16])
              for k in range(0, len(alerts), PIECE)]
    return (f"segment {i} (rounds {lo}..{hi}) is the first to differ from the record in: {', '.join(fields)}\n"
            f"  recorded list before the segment: per chunk {before[0]}, |L| = {before[1]}\n"
            f"  recorded list after the segment:  per chunk {case['listed'][i]}, |L| = {case['live'][i]}\n"
            f"  this run's alerts in {PIECE}-round pieces (first round, sum, sha256[:16] of int64 LE):\n    " +
            "\n    ".join(f"{a}: {s} {h}" for a, s, h in pieces))


def drain(name, ranks, kernel, monkeypatch):
    case = rec.load()[name]
    n, topo, seed = rec.CASES[name]
    if kernel:
        monkeypatch.setenv("GP_KERNEL", kernel)
    sim = Sim(n, topo, "gossip", seed=seed, virtual_ranks=ranks, experimental=bool(kernel))
    try:
        info = sim.info()
        assert (info.population, info.threshold, info.num_gpus) == (case["population"], case["threshold"], ranks)
        nseg = len(case["live"])
        for i in range(nseg):
            a = sim.step(rec.SEG)
            c, f = rec.state_digests(sim.state())
            got = {"alerts_sha256": rec.alerts_digest(a), "alerts_cum": sim.alerts_total, "c_sha256": c, "flags_sha256": f}
            bad = [k for k, v in got.items() if v != case[k][i]]
            if len(a) != min(rec.SEG, case["rounds"] - i * rec.SEG):
                bad.insert(0, f"rounds run ({len(a)})")
            assert not bad, describe(case, i, bad, a)
            if i == 0:
                want = COL if kernel == "col" else PRODUCT_KERNEL
                assert want in sim.kernel_stats()[2], sim.kernel_stats()[2]
        assert sim.step(rec.SEG) == [], "the run went on past the recorded convergence round"
        assert (sim.rounds, sim.alerts_total) == (case["rounds"], case["alerts_total"])
    finally:
        sim.close()


@pytest.mark.parametrize("name,ranks,kernel", RUNS, ids=[run_id(r) for r in RUNS])
def test_injector_drain_matches_oracle_record(name, ranks, kernel, monkeypatch):
    if (name, ranks, kernel) in FULL_ONLY and os.environ.get("GP_BASELINE_FULL") != "1":
        pytest.skip("more than 20 s on an MI355X: GP_BASELINE_FULL=1")
    drain(name, ranks, kernel, monkeypatch)
