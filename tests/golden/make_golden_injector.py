"""Generate tests/golden/runs_injector.json: gossip runs to convergence whose injector list has two
chunks of 65536 ids and drains to a handful, from the C oracle (oracle/srs_oracle.c).

    python tests/golden/make_golden_injector.py [case ...]     # cases: line 3D Imp3D (default: all)

The cases, the segmentation and the fields are those of tests/injector_record.py; about a minute
of oracle time per case.  No per-round arrays: every segment of 2048 rounds is stored as digests
(tests/test_gpu_injector_drain.py compares the product with them without running the oracle).
The coverage conditions (injector_record.check_coverage) are asserted from the oracle's own
counts before anything is written.  Fixtures of the build's own oracle: parity with the reference
stays "parity unpinned" (SURVEY.md §8c).

`oracle_seconds` is the one field that is not a function of the run: a case whose other fields
come out as recorded keeps the recorded figure, so the script reproduces the file byte for byte.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import injector_record as rec  # noqa: E402
from tests.oracle_ctypes import Oracle  # noqa: E402


def record(name, n, topo, seed, log=None):
    t0 = time.time()
    orc = Oracle(n, topo, "gossip", seed)
    out = {"num_nodes": n, "topology": topo, "algorithm": "gossip", "seed": seed, "population": orc.P,
           "threshold": orc.T, "segment": rec.SEG}
    out.update({k: [] for k in rec.FIELDS})
    assert orc.injector_live == orc.T and rec.nchunks(orc.T) == 2
    while orc.alerts_total < orc.T:
        a = orc.step(rec.SEG)
        assert a, f"{name}: the oracle stopped short of convergence"
        c, f = rec.state_digests(orc.state())
        out["alerts_cum"].append(orc.alerts_total)
        out["alerts_sha256"].append(rec.alerts_digest(a))
        out["c_sha256"].append(c)
        out["flags_sha256"].append(f)
        out["listed"].append([orc.injector_listed(k * rec.INJ_CHUNK, rec.INJ_CHUNK) for k in range(2)])
        out["live"].append(orc.injector_live)
        if log:
            log(f"[{name}] round {orc.rounds}: alerts {orc.alerts_total} of {orc.T}, listed {out['listed'][-1]} "
                f"({time.time() - t0:.0f} s)")
    out["rounds"], out["alerts_total"] = orc.rounds, orc.alerts_total
    orc.close()
    rec.check_coverage(name, out)
    out["oracle_seconds"] = round(time.time() - t0, 1)
    return out


def main(names):
    out = rec.load() if os.path.exists(rec.PATH) else {}
    for name in names:
        new = record(name, *rec.CASES[name], log=lambda m: print(m, file=sys.stderr, flush=True))
        old = out.get(name)
        if old and {**old, "oracle_seconds": 0} == {**new, "oracle_seconds": 0}:
            new["oracle_seconds"] = old["oracle_seconds"]
        out[name] = new
        with open(rec.PATH, "w") as f:
            json.dump({k: out[k] for k in rec.CASES if k in out}, f, separators=(",", ":"))
            f.write("\n")
        print(f"[{name}] converged in {new['rounds']} rounds", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(rec.CASES))
