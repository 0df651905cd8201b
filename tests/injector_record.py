"""The recorded gossip runs that drain the injector's two-chunk list (tests/golden/runs_injector.json):
what the generator (tests/golden/make_golden_injector.py), the CPU test of the record
(tests/test_injector_record.py) and the GPU cases (tests/test_gpu_injector_drain.py) share.

A run is cut into segments of SEG rounds (the last one shorter).  Per segment the record holds, as
one list per field with one entry per segment:
  alerts_cum     cumulative alerts at the segment's end
  alerts_sha256  sha256 of the segment's per-round alert counts as little-endian int64
  c_sha256       sha256 of c of all P nodes (little-endian int32) after the segment
  flags_sha256   sha256 of flags of all P nodes (uint8) after the segment
  listed         the oracle's count of listed ids per chunk of INJ_CHUNK ids after the segment
  live           |L| after the segment
hashlib only: the GPU machine needs nothing beyond the standard library and numpy.
"""
import hashlib
import json
import os

import numpy as np

SEG = 2048
INJ_CHUNK = 65536   # ids per chunk of the product's list (gp_internal.hpp)
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runs_injector.json")
FIELDS = ("alerts_cum", "alerts_sha256", "c_sha256", "flags_sha256", "listed", "live")

# name -> (num_nodes, topology, seed); all gossip.  65537 is the smallest line and 41^3 = 68921 the
# smallest lattice whose list has two chunks (40^3 = 64000).  Seed 3 where it meets check_coverage.
# Imp3D does not with seeds 3..11: those runs end 1300 to 2000 rounds after a segment end, at
# which chunk 1 still lists 38 to 53 ids (seed 3: 38 at round 96 256 of 97 560); seed 12 is the
# first that does (98 394 rounds, 3 ids at round 98 304).
CASES = {"line": (65537, "line", 3), "3D": (68921, "3D", 3), "Imp3D": (68921, "Imp3D", 12)}


def alerts_digest(alerts):
    return hashlib.sha256(np.asarray(alerts, "<i8").tobytes()).hexdigest()


def state_digests(st):
    """(c_sha256, flags_sha256) of a state() dictionary."""
    return (hashlib.sha256(np.ascontiguousarray(st["c"], "<i4").tobytes()).hexdigest(),
            hashlib.sha256(np.ascontiguousarray(st["flags"], "u1").tobytes()).hexdigest())


def nchunks(T):
    return (T + INJ_CHUNK - 1) // INJ_CHUNK


def load():
    with open(PATH) as f:
        return json.load(f)


def check_coverage(name, case):
    """The conditions a recorded run must meet to be worth comparing: asserted by the generator
    before it writes and by the CPU test of the committed file.  Never relaxed: a run that misses
    one is recorded with another seed."""
    T, rounds, listed, live = case["threshold"], case["rounds"], case["listed"], case["live"]
    nseg = len(live)
    assert nseg == -(-rounds // SEG) and all(len(case[k]) == nseg for k in FIELDS)
    assert nchunks(T) == 2 and all(len(row) == 2 and sum(row) == lv for row, lv in zip(listed, live))
    assert case["alerts_total"] == case["alerts_cum"][-1] == T, f"{name}: the run did not converge"
    ends = [min((i + 1) * SEG, rounds) for i in range(nseg)]
    if case["topology"] == "line":
        assert T - INJ_CHUNK == 1
        assert any(row[1] == 0 and rounds - end >= 20000 for row, end in zip(listed, ends)), \
            f"{name}: chunk 1 is not empty with 20 000 rounds still to run"
        return
    first = T - INJ_CHUNK   # ids of chunk 1 at the start
    assert first == 3385
    assert first - listed[-2][1] >= 3000, f"{name}: chunk 1 lost fewer than 3000 ids before the last segment"
    assert any(row[1] < 32 for row in listed[:-1]), f"{name}: chunk 1 never below 32 ids at a segment end before the last"
    assert live[-1] < 64, f"{name}: |L| = {live[-1]} at the end"
