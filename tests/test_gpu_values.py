"""GPU: Simulation over caller-supplied values and weights (gp_set_values / gp_set_mean, SRS v1-V),
bit-exact on the raw bits of s and w, the flags and the per-round alerts.

The C oracle cannot be given values, but its or_pushsum_receivers performs one push-sum round for
chosen receivers from an arbitrary round-start state.  So every check stands on its own: read the
GPU state, step one round, read again, and require that the oracle maps the first state to the
second -- for all ids, or on the 106^3 lattice for a fixed sample that holds every tile edge --
and that its count of converging receivers is the round's alert count over those ids.  Between
checked steps the GPU runs unchecked batches, so that later phases are reached.  With non-dyadic
values (0.1 (i + 1)) every addition rounds, so the canonical fold order shows from the first
delivery on.

Shapes: the smallest at which each round kernel can still go wrong -- line at the tile edge,
3D as one box / one-node-thick slabs / uneven cuts / the first side on the tile kernel, Imp3D,
full at two bin sizes, and virtual ranks (each id routed to its slab's array, round 0's halo and
list exchange repeated after the values were set).
"""
import ctypes as C
import math

import numpy as np
import pytest

from gossipprotocol_amd import _lib as L
from gossipprotocol_amd import default_mean
from tests import summary_ref
from tests import values_ref as V
from tests.oracle_ctypes import pushsum_receivers
from tests.test_gpu_parity import Sim

pytestmark = pytest.mark.gpu

TILE = 1024
SEED = 3


def values_a(P):
    """Non-dyadic, no weights."""
    return 0.1 * (np.arange(P, dtype=np.float64) + 1.0), None


def values_b(P):
    """Zeros and 2^-64 among non-dyadic values; weights from 2^-32 to 2^32, and entries whose
    x * 2^-32 lies one ulp below the weight."""
    i = np.arange(P, dtype=np.int64)
    x = 0.1 * (i + 1.0)
    w = 1.0 + 0.25 * (i % 5)
    k = i % 8
    x[k == 1] = 0.0
    x[k == 2] = 2.0 ** -64
    w[k == 3] = 2.0 ** 32
    w[k == 4] = 2.0 ** -32
    x[k == 4] = 0.1 * ((i[k == 4] % 9) + 1.0)
    x[k == 5] = 12345.678 * (i[k == 5] + 1.0)
    w[k == 5] = np.nextafter(x[k == 5] * 2.0 ** -32, np.inf)
    w[k == 6] = 2.0 ** -32
    x[k == 6] = 0.0
    assert V.first_offender(x[:4096], w[:4096]) is None
    return x, w


SETS = {"a": values_a, "b": values_b}

# (topology, num_nodes, virtual ranks)
SHAPES = [("line", 1023, 1), ("line", 1024, 1), ("line", 1025, 1),
          ("3D", 16 ** 3, 1), ("3D", 21 ** 3, 1), ("3D", 29 ** 3, 1), ("3D", 106 ** 3, 1),
          ("Imp3D", 11 ** 3, 1), ("Imp3D", 17 ** 3, 1),
          ("full", 4096, 1), ("full", 20480, 1),
          ("Imp3D", 12 ** 3, 2), ("Imp3D", 12 ** 3, 3), ("full", 8192, 2), ("full", 8192, 3)]


def raw(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def receivers(P):
    if P <= 30000:
        return np.arange(P, dtype=np.int64)
    edges = np.arange(TILE, P, TILE, dtype=np.int64)
    rnd = np.random.default_rng(11).integers(0, P, 2000)
    return np.unique(np.concatenate([[0, P - 1], edges - 1, edges, rnd])).astype(np.int64)


def checked_step(sim, topo, n, ids, what, seed=SEED):
    """One round, checked against the oracle's receivers.  False: the run had converged."""
    a = sim.state()
    r = sim.rounds
    alerts = sim.step(1)
    if not alerts:
        return False
    b = sim.state()
    so, wo, fo, conv = pushsum_receivers(topo, n, seed, r, a["s"], a["w"], a["flags"], ids)
    bad = np.nonzero((raw(so) != raw(b["s"][ids])) | (raw(wo) != raw(b["w"][ids])) | (fo != b["flags"][ids]))[0]
    assert not len(bad), (f"{what}: round {r}: node {ids[bad[0]]} of {len(bad)} differs: s {b['s'][ids[bad[0]]]!r} / "
                          f"{so[bad[0]]!r}, w {b['w'][ids[bad[0]]]!r} / {wo[bad[0]]!r}, flags {b['flags'][ids[bad[0]]]} / {fo[bad[0]]}")
    newly = int((((b["flags"][ids] >> 1) & 1) & ~((a["flags"][ids] >> 1) & 1)).sum())
    assert conv == newly, f"{what}: round {r}: {conv} converging receivers, {newly} in the state"
    if len(ids) == len(a["s"]):
        assert alerts == [conv], f"{what}: round {r}: alerts {alerts}, oracle {conv}"
    return True


@pytest.mark.parametrize("vset", sorted(SETS))
@pytest.mark.parametrize("topo,n,ranks", SHAPES, ids=lambda v: str(v))
def test_rounds_from_values(topo, n, ranks, vset):
    sim = Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks)
    P = sim.population
    x, w = SETS[vset](P)
    before = sim.state()
    sim.set_values(x, w)
    st = sim.state()  # round 0: exactly what was set, everything else as it was
    assert np.array_equal(raw(st["s"]), raw(x)) and np.array_equal(raw(st["w"]), raw(np.ones(P) if w is None else w))
    assert np.array_equal(st["flags"], before["flags"]) and sim.rounds == 0
    ids = receivers(P)
    what = f"{topo} n={n} W={ranks} set {vset} ({sim.kernel_stats()[2]})"
    block = "block" in sim.kernel_stats()[2]
    target = P if block else (P + 9) // 10  # block kernel: until every face has carried traffic
    batch, extra, checked = 7, 0, 0
    while True:
        assert sim.rounds < 3000, f"{what}: {sim.info().active} of {P} active after {sim.rounds} rounds"
        if not checked_step(sim, topo, n, ids, what):
            break
        checked += 1
        if sim.info().active >= target:
            extra += 1
            if extra > 2:
                break
        sim.step(batch)
        batch = 7 if batch == 12 else 12  # (both parities of the round count get checked)
    assert sim.info().active >= target or sim.alerts_total >= sim.threshold, what
    print(f"{what}: {checked} checked rounds of {sim.rounds}, {sim.info().active} of {P} active, {len(ids)} receivers")
    sim.close()


@pytest.mark.parametrize("topo,n,ranks", [("Imp3D", 12 ** 3, 2), ("Imp3D", 12 ** 3, 3), ("3D", 12 ** 3, 3)], ids=str)
def test_round_zero_across_ranks(topo, n, ranks):
    """Round 0's halo planes and random-edge lists were packed at create, from s = id: after
    gp_set_values they travel again.  24 seeds put the seed node on slab edges and its first
    message on lattice and random edges that cross them; the first three rounds are checked."""
    crossed = 0
    for seed in range(1, 25):
        sim = Sim(n, topo, "push-sum", seed=seed, virtual_ranks=ranks)
        P = sim.population
        x, w = values_b(P)
        sim.set_values(x[:P // 2], w[:P // 2])
        sim.set_values(x[P // 2:], w[P // 2:], first=P // 2)
        ids = np.arange(P, dtype=np.int64)
        for _ in range(3):
            assert checked_step(sim, topo, n, ids, f"{topo} W={ranks} seed {seed}", seed)
        act = np.nonzero(sim.state()["flags"] & 1)[0]
        cut = [P * k // ranks for k in range(1, ranks)]  # (about where the slabs meet)
        crossed += any(act.min() < c <= act.max() for c in cut)
        sim.close()
    assert crossed >= 3, crossed


@pytest.mark.parametrize("g", [16, 21, 29])
def test_block_kernel_batches_equal_single_rounds(g):
    """The checked pairs above are one-round launches of k_ps_block; its multi-round launches --
    faces exchanged inside the launch through the sign-tagged words, 64-round epochs, checkpoints
    -- run there only as unchecked batches.  Here N = 150 rounds (two epochs and a partial one)
    as one step(N) give the state of N checked single rounds, twice in a row."""
    n, N = g ** 3, 150
    one, many = Sim(n, "3D", "push-sum", seed=SEED), Sim(n, "3D", "push-sum", seed=SEED)
    assert "block" in one.kernel_stats()[2]
    x, w = values_b(n)
    one.set_values(x, w)
    many.set_values(x, w)
    ids = np.arange(n, dtype=np.int64)
    for leg in range(2):
        before = many.alerts_total
        for k in range(N):
            if k % 10 == 0:  # (every tenth single round against the oracle as well)
                assert checked_step(many, "3D", n, ids, f"3D g={g} single rounds")
            else:
                assert len(many.step(1)) == 1
        got = one.step(N)
        assert len(got) == N and sum(got) == many.alerts_total - before == one.alerts_total - before
        a, b = one.state(), many.state()
        for f in ("s", "w", "flags"):
            assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), f"g={g} leg {leg}: {f} differs after {one.rounds} rounds"
    assert one.rounds == many.rounds == 2 * N
    one.close()
    many.close()


@pytest.mark.parametrize("topo,n,ranks", [("3D", 21 ** 3, 1), ("Imp3D", 12 ** 3, 3), ("full", 4096, 1)], ids=str)
def test_chunks_equal_one_call(topo, n, ranks):
    one, many = Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks), Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks)
    P = one.population
    x, w = values_b(P)
    one.set_values(x, w)
    cuts = [0, 1, 1000, 1001, P // 2 + 3, P]
    for a, b in reversed(list(zip(cuts, cuts[1:]))):  # (any order)
        many.set_values(x[a:b], w[a:b], first=a)
    many.set_mean(default_mean(x.tolist(), w.tolist()))
    for k in (0, 25):
        assert one.step(k) == many.step(k)
        s1, s2 = one.state(), many.state()
        assert all(np.array_equal(s1[f].view(np.uint8), s2[f].view(np.uint8)) for f in ("s", "w", "flags"))
    assert summary_ref.raw(one.summary()) == summary_ref.raw(many.summary())
    one.close()
    many.close()


@pytest.mark.parametrize("ranks", [1, 2])
def test_refused_chunk_leaves_the_state(ranks):
    sim = Sim(12 ** 3, "Imp3D", "push-sum", seed=SEED, virtual_ranks=ranks)
    P = sim.population
    x, w = values_b(P)
    sim.set_values(x, w, mean=5.0)
    before = sim.state()
    for bad_id, (bx, bw), word in ((700, (-0.0, None), "finite"), (1500, (1.0, 2.0 ** -33), "2^-32, 2^32"),
                                   (P - 1, (2.0 ** -70, None), "2^-64"), (0, (2.0 ** 32, 1.0), "below the weight"),
                                   (900, (math.nan, None), "finite")):
        x2, w2 = x.copy(), w.copy()
        x2[::8] *= 0.5  # (admissible, and different from what the state holds)
        x2[min(P - 1, bad_id + 5)] = math.inf  # a later offender: the lowest id is the one named
        x2[bad_id] = bx
        if bw is not None:
            w2[bad_id] = bw
        with pytest.raises(L.GossipError) as ei:
            sim.set_values(x2[bad_id // 2:], w2[bad_id // 2:], first=bad_id // 2)
        assert ei.value.code == -1 and f"node {bad_id} " in str(ei.value) and word in str(ei.value), str(ei.value)
        st = sim.state()
        assert all(np.array_equal(st[f].view(np.uint8), before[f].view(np.uint8)) for f in ("s", "w", "flags"))
    lib, h = sim._L, sim._h
    dp = C.POINTER(C.c_double)
    assert lib.gp_set_values(h, P - 1, 2, x.ctypes.data_as(dp), None) == -1 and b"owns" in lib.gp_last_error()
    assert lib.gp_set_values(h, -1, 1, x.ctypes.data_as(dp), None) == -1
    assert lib.gp_set_values(h, 0, 1, None, None) == -1
    assert lib.gp_set_values(h, 5, 0, None, None) == 0
    for mu in (math.nan, -1.0, 2.0 ** 32):
        assert lib.gp_set_mean(h, mu) == -1 and b"mean" in lib.gp_last_error()
    sim.close()


def test_state_errors():
    sim = Sim(1000, "3D", "push-sum", seed=SEED)
    x, _ = values_a(sim.population)
    sim.set_values(x)
    sim.step(1)
    with pytest.raises(L.GossipError) as ei:
        sim.set_values(x)
    assert ei.value.code == -5  # GP_ESTATE
    sim.set_mean(3.0)  # (any round)
    sim.close()
    g = Sim(1000, "3D", "gossip", seed=SEED)
    for call in (lambda: g.set_values(x), lambda: g.set_mean(1.0)):
        with pytest.raises(L.GossipError) as ei:
            call()
        assert ei.value.code == -1 and "gossip" in str(ei.value)
    g.close()


@pytest.mark.parametrize("topo,n,ranks,vset", [("3D", 21 ** 3, 1, "b"), ("Imp3D", 12 ** 3, 3, "a"), ("full", 4096, 1, "b"),
                                               ("line", 1025, 1, "a")], ids=str)
def test_summary_against_the_set_mean(topo, n, ranks, vset):
    sim = Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks)
    P = sim.population
    x, w = SETS[vset](P)
    sim.set_values(x, w)  # the default mean
    mu = V.default_mean(x.tolist(), None if w is None else w.tolist())
    tol = 0.25
    for k, mean in ((0, None), (40, None), (35, 17.25)):
        sim.step(k)
        if mean is not None:
            sim.set_mean(mean)
            mu = mean
        ref = V.ref_summary(sim.state(), 0, P, sim.rounds, sim.seed_node, tol, mu)
        summary_ref.assert_exact(sim.summary(tol), ref, f"{topo} W={ranks} round {sim.rounds}")
    plain = Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks)  # never set: mu = (P - 1) / 2
    plain.step(20)
    ref = summary_ref.ref_summary(plain.state(), 0, P, plain.rounds, 1, plain.seed_node, tol)
    summary_ref.assert_exact(plain.summary(tol), ref, "plain")
    sim.close()
    plain.close()
