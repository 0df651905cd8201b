"""GPU: the LDS-resident 3D push-sum kernel (k_ps_block, gp_block.hip) at its box-shape and
replay edges, bit-exact against the CPU oracle.

Box shapes (test_box_shapes): the product build picks the kernel for every lattice side that has a
plan (gp_block_plan.hpp); the sides below stand for the shape classes of the plans on 256 CUs --
one box, slabs one and two nodes thick (both z neighbours of a node come from halos), faces
exactly as large as the workgroup, boxes of two and five node slots, LDS next to its limit, the
last planned side and the first side without a plan.  tests/test_block_plan.py pins that table to
the code on the CPU.

Steering (test_converging_launch): the launch in which the run converges.  gp_step(k) with
k <= 1024 is one cooperative launch of k rounds starting at the rounds done so far, and the oracle
gives the converging round Rc in advance, so stepping to Rc - d and then asking for m rounds puts
Rc at a chosen place of a chosen epoch: the checkpoint replay with one round and with many, from
the launch's input and from a checkpoint the kernel wrote; no replay when Rc ends an epoch;
partial epochs; the counter sets' rotation; both parities of the executed count; either side of
the host's 1024-round batch cut.
"""
import functools

import pytest

from tests.oracle_ctypes import Oracle
from tests.test_block_plan import PLANS_256
from tests.test_gpu_parity import Sim, assert_same_state

pytestmark = pytest.mark.gpu

BLOCK = "k_ps_block<GRID3D>"
EPOCH, BATCH = 64, 1024  # gp_internal.hpp BLOCK_EPOCH, gp_host.hpp BATCH


def frozen(st):
    for v in st.values():
        v.setflags(write=False)
    return st


# ---------------------------------------------------------------- box shapes
CHUNKS = (37, 64, 65, 1, 63)  # cut the 64-round epochs at odd places
SEED = 2


def rounds_after_full(g):
    # two epochs and a partial one with traffic on every face; from g = 104 one epoch, so that no
    # case needs more than about ten seconds of oracle time (1.1e6 nodes, full activation takes
    # ~350 rounds there)
    return 64 if g >= 104 else 130


@pytest.mark.parametrize("g", sorted(PLANS_256))
def test_box_shapes(g):
    """Per-round alerts and the full state after every chunk, from the seed's first message until
    every node has been active for rounds_after_full(g) rounds (g = 2: its 8 nodes converge
    before that; the comparison then runs through convergence)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sim, orc = Sim(g ** 3, "3D", "push-sum", seed=SEED), Oracle(g ** 3, "3D", "push-sum", SEED)
    assert sim.population == orc.P == g ** 3 and sim.info().grid == g
    name = sim.kernel_stats()[2]
    if cus == 256:  # the plan is the table's (tests/test_block_plan.py): g = 106 has none
        assert (name == BLOCK) == (PLANS_256[g] is not None), name
    assert name == BLOCK or "tile" in name, name
    print(f"g={g}: {name} on {cus} CUs, plan {PLANS_256[g]} "
          + ("(256 CUs: the table's plan)" if cus == 256 else "-- shape class unconfirmed on this CU count"))
    full_at, i = None, 0
    while full_at is None or orc.rounds < full_at + rounds_after_full(g):
        assert orc.rounds < 1000, "activation did not complete"
        k = CHUNKS[i % len(CHUNKS)]
        i += 1
        ga, oa = sim.step(k), orc.step(k)
        assert ga == oa, f"alerts differ in rounds {orc.rounds - len(oa)}..{orc.rounds}"
        assert_same_state("push-sum", sim.state(), orc.state())
        if full_at is None and orc.active_count() == orc.P:
            full_at = orc.rounds
        if len(oa) < k:  # converged
            break
    assert full_at is not None
    assert sim.rounds == orc.rounds and sim.alerts_total == orc.alerts_total
    assert sim.info().active == sim.population
    sim.close()
    orc.close()


# ---------------------------------------------------------------- steering the converging launch
# (d, m): step to r0 = Rc - d, then one step(m).  What the launch that converges then does, as
# (launch of the step call, its epoch, last, n, rounds it executes): `last` is the converging
# round's place in the epoch (1-based), n the epoch's length; last < n replays `last` rounds from
# the epoch's checkpoint, last == n does not.
STEER = [
    (0, 64, (0, 0, 1, 64, 1)),          # epoch 0, replay of one round from the input checkpoint
    (63, 64, (0, 0, 64, 64, 64)),       # last = n = 64: no replay, the launch ends on the epoch
    (63, 200, (0, 0, 64, 64, 64)),      # the same with further epochs requested
    (64, 128, (0, 1, 1, 64, 65)),       # epoch 1, replay of one round from a checkpoint the kernel wrote
    (94, 1024, (0, 1, 31, 64, 95)),     # mid epoch 1, odd executed count
    (95, 1024, (0, 1, 32, 64, 96)),     # mid epoch 1, even executed count
    (202, 300, (0, 3, 11, 64, 203)),    # epoch 3: counter set 0 again, after being cleared
    (20, 40, (0, 0, 21, 40, 21)),       # partial epoch
    (39, 40, (0, 0, 40, 40, 40)),       # partial epoch, last = n: no replay
    (20, 21, (0, 0, 21, 21, 21)),       # the launch ends exactly on the converging round
    (1029, 2000, (1, 0, 6, 64, 6)),     # the host cuts at 1024: the second launch converges in its epoch 0
    (1023, 2000, (0, 15, 64, 64, 1024)),  # the last round of the first launch's 16th epoch
]
ONE_BOX = [  # one box: epochs of one round, nothing to replay
    (0, 64, (0, 0, 1, 1, 1)),
    (7, 64, (0, 7, 1, 1, 8)),
]
STEER_CASES = [(g, seed, boxes, d, m, hit) for g, seed, boxes in ((17, 1, 6), (20, 7, 8)) for d, m, hit in STEER] \
    + [(10, 3, 1, d, m, hit) for d, m, hit in ONE_BOX]


def converging_launch(d, m, boxes):
    """gp_step's batches and the kernel's epoch loop, restated: where round r0 + d falls."""
    E = EPOCH if boxes > 1 else 1
    launch = d // BATCH
    dl, ml = d - launch * BATCH, min(BATCH, m - launch * BATCH)
    epoch = dl // E
    return launch, epoch, dl % E + 1, min(E, ml - E * epoch), dl + 1


@functools.lru_cache(maxsize=None)
def oracle_run(g, seed):
    """One oracle run to convergence, a round at a time: (R, every round's alerts, {r0: the state
    at the start of round r0} for the r0 = R - 1 - d of this lattice's cases, the final state, the
    alert total)."""
    offsets = sorted({c[3] for c in STEER_CASES if c[:2] == (g, seed)})
    orc = Oracle(g ** 3, "3D", "push-sum", seed)
    keep = max(offsets) + 1  # (R is not known before the end: the last `keep` round starts are held)
    ring, alerts = {}, []
    while orc.alerts_total < orc.T:
        assert orc.rounds < 100000
        r = orc.rounds
        st = orc.state()
        ring[r] = (st["s"], st["w"], st["flags"])
        ring.pop(r - keep, None)
        a = orc.step(1)
        assert len(a) == 1
        alerts += a
    R, total = orc.rounds, orc.alerts_total
    final = frozen(orc.state())
    orc.close()
    snaps = {}
    for d in offsets:
        s, w, f = ring[R - 1 - d]
        snaps[R - 1 - d] = frozen({"s": s, "w": w, "flags": f})
    return R, tuple(alerts), snaps, final, total


@pytest.mark.parametrize("g,seed,boxes,d,m,hit", STEER_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_converging_launch(g, seed, boxes, d, m, hit, monkeypatch):
    """GP_CHECK_CLOSE recounts the alerted nodes from the state after every launch and fails the
    step if the kernel's bookkeeping disagrees."""
    monkeypatch.setenv("GP_KERNEL", "block")
    monkeypatch.setenv("GP_CHECK_CLOSE", "1")
    R, alerts, snaps, final, total = oracle_run(g, seed)
    assert R > 2200 and len(alerts) == R  # every offset of the tables is a valid round
    Rc = R - 1
    r0 = Rc - d
    # what the case claims to hit, from d and m alone
    launch, epoch, last, n, executed = converging_launch(d, m, boxes)
    assert (launch, epoch, last, n, executed) == hit
    if boxes > 1 and launch == 0:
        assert (epoch, last, n) == (d // 64, d % 64 + 1, min(64, m - 64 * (d // 64)))
    assert 1 <= last <= n and d < m

    sim = Sim(g ** 3, "3D", "push-sum", seed=seed, experimental=True)
    assert sim.kernel_stats()[2] == BLOCK
    got = []
    while sim.rounds < r0:
        got += sim.step(min(997, r0 - sim.rounds))
    assert sim.rounds == r0 and tuple(got) == alerts[:r0]
    assert_same_state("push-sum", sim.state(), snaps[r0])

    assert tuple(sim.step(m)) == alerts[r0:]
    assert sim.rounds == R
    assert sim.alerts_total == total >= sim.threshold
    st = sim.state()
    assert_same_state("push-sum", st, final)
    assert sim.step(10) == [] and sim.rounds == R and sim.alerts_total == total
    assert_same_state("push-sum", sim.state(), st)
    sim.close()
