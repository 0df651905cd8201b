"""GPU: what the tiled round kernels carry from one tile to the next, on grids small enough that a
block runs several tiles of a small slab; against the CPU oracle, bit-exact (per-round alerts, and
s / w / flags -- gossip: c / flags -- of every node at every checkpoint).

k_ps_tile, wide::k_ps_tile and k_gossip_tile are persistent: a block walks several tiles per launch
(TileWalk, gp_tile.hpp) and ps_tiles (gp_ps_tile.hip) carries state across them -- the next tile's
in-edge range (pf_tile / pf_lo / pf_hi), its senders copied by LDS-DMA during this tile's node phase
(snd / snd_tile / snd_off, consumed only when snd_tile == ti and skipped when the next tile is over
the staging cap), walk 3's claim published through L.qn by iteration parity, the `continue` on empty
items, the steal loop over the other XCDs' queues, and the LDS buffers the next tile restages
without a barrier while this tile's byte output drains.  choose_kernel (gp_setup.hip) sizes the
grid as min(roundup8(tiles + 1), 64 CUs) -- walk 3: the resident blocks -- so below ~1.7e7 nodes no
block ever gets a second tile and none of that runs.  GP_GRID (experiments build) lowers the grid;
gp_kernel_stats then reports the kernel as name@grid, which every case asserts.

Every case first proves on the CPU that it reaches its edge: the blocks' tile sequences from the
walk model (tests/tile_walk_ref.py, checked by tests/test_tile_walk_ref.py) and the tiles' in-edge
counts and largest node in-degrees recounted from Oracle.neighbors.  These conditions are asserted,
never skipped.

Seed 2 throughout.  Imp3D n = 8000 (g = 20): 8 tiles, the last of 832 nodes; in-edges per tile 987,
1011, 1022, 1066, 1032, 1030, 1039, 813; largest node in-degree 7; every node active from round 32;
converged in round 428.  A tile is `staged` when its in-edges fit min(slots, GP_STAGE_CAP) (1152
slots on one rank, 1216 across ranks; gossip 1536), `wide` when it holds a node of in-degree >=
GP_IND4_WIDE (15 in the product), `partial` at a slab's ends; only a whole, staged, not-wide tile
runs the FULL body.

Where the walk is not forced the product's choice applies: walk 0 (g / ranks < 64), x-window 8.

A slab's first tile is item 0 of block 0 (queue 0) in every walk, so a partial first tile can be
followed by another tile in its block but never preceded by one; a partial last tile is preceded
and, in the walk-3 queues of g = 33, also followed.
"""
import functools
from collections import Counter, namedtuple

import numpy as np
import pytest

from tests import multirank_emu as emu
from tests import tile_walk_ref as tw
from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim

pytestmark = pytest.mark.gpu

SEED = 2
SLOTS, SLOTS_REMOTE, SRC_CAP = 1152, 1216, 1536  # PsSlots<false>, PsSlots<true> (gp_ps_tile.hip); gp_gossip_tile.hip
NO_CAP = 0xFFFFFFFF
Ref = namedtuple("Ref", "chunks rounds alerts_total T")


# ---------------------------------------------------------------- the oracle's runs, once per case
@functools.lru_cache(maxsize=None)
def reference(n, topo, alg, limit, late=64):
    """chunks = [(rounds asked, alerts of the chunk, state after it)]: a checkpoint every 8 rounds up
    to round 64, then every `late`; limit = None: through convergence."""
    orc = Oracle(n, topo, alg, SEED)
    keys = ("c", "flags") if alg == "gossip" else ("s", "w", "flags")
    chunks = []
    while orc.alerts_total < orc.T and (limit is None or orc.rounds < limit):
        assert orc.rounds < 25000, "the oracle did not converge"
        k = 8 if orc.rounds < 64 else late
        if limit is not None:
            k = min(k, limit - orc.rounds)
        a = orc.step(k)
        st = {key: v for key, v in orc.state().items() if key in keys}
        for v in st.values():
            v.setflags(write=False)
        chunks.append((k, a, st))
        if len(a) < k:
            break
    ref = Ref(chunks, orc.rounds, orc.alerts_total, orc.T)
    orc.close()
    return ref


def check(sim, ref):
    done = 0
    for k, oa, ost in ref.chunks:
        ga = sim.step(k)
        assert ga == oa, f"alerts differ in rounds {done}..{done + k}"
        gs = sim.state()
        for key, v in ost.items():
            np.testing.assert_array_equal(gs[key], v, err_msg=f"'{key}' after round {done + len(oa)}")
        done += len(oa)
    assert sim.rounds == ref.rounds and sim.alerts_total == ref.alerts_total


KERNEL = {("push-sum", "Imp3D"): "k_ps_tile<IMP3D>", ("push-sum", "3D"): "k_ps_tile<GRID3D>",
          ("push-sum", "line"): "k_ps_tile<LINE>", ("gossip", "Imp3D"): "k_gossip_tile<IMP3D>",
          ("gossip", "3D"): "k_gossip_tile<GRID3D>", ("gossip", "line"): "k_gossip_tile<LINE>"}


def run(monkeypatch, n, topo, alg, ref, grid, ranks=1, wide="0", **extra):
    monkeypatch.setenv("GP_KERNEL", "tile")
    monkeypatch.setenv("GP_WIDE", wide)
    monkeypatch.setenv("GP_GRID", str(grid))
    for k, v in extra.items():
        monkeypatch.setenv(k, str(v))
    sim = Sim(n, topo, alg, seed=SEED, virtual_ranks=ranks, experimental=True)
    assert sim.info().num_gpus == ranks
    name = sim.kernel_stats()[2]
    assert name == ("wide::" if wide == "1" else "") + KERNEL[alg, topo] + f"@{grid}", name  # the override took effect
    check(sim, ref)
    sim.close()


# ---------------------------------------------------------------- the CPU side of every case
@functools.lru_cache(maxsize=None)
def in_degrees(g):
    """Random-edge in-degree of every node of the g^3 Imp3D network of SEED, from the oracle's
    neighbour lists: a node's random edge is the neighbour that is not one of its lattice ones, or the
    one listed twice."""
    n = g ** 3
    orc = Oracle(n, "Imp3D", "push-sum", SEED)
    assert orc.P == n
    deg = np.zeros(n, np.int64)
    for i in range(n):
        x, y, z = i // (g * g), i // g % g, i % g
        lat = {j for j, ok in ((i - g * g, x > 0), (i + g * g, x < g - 1), (i - g, y > 0), (i + g, y < g - 1),
                               (i - 1, z > 0), (i + 1, z < g - 1)) if ok}
        nb = orc.neighbors(i)
        assert len(nb) == len(lat) + 1 and lat <= set(nb)
        rnd = [t for t in nb if t not in lat] or [t for t, k in Counter(nb).items() if k > 1]
        assert len(rnd) == 1
        deg[rnd[0]] += 1
    orc.close()
    deg.setflags(write=False)
    return deg


Slab = namedtuple("Slab", "lo nloc nt edges maxdeg partial")


@functools.lru_cache(maxsize=None)
def slabs(topo, n, ranks=1):
    """Every rank's slab: its tiles' in-edge counts, largest node in-degrees (Imp3D) and which are partial."""
    P, _, g = emu.resolve(n, topo)
    bounds = emu.slab_bounds(P, g, topo, ranks)[0]
    out = []
    for r in range(ranks):
        lo, nloc = bounds[r], bounds[r + 1] - bounds[r]
        nt = tw.tiles_for(lo, nloc)
        rng = [tw.tile_range(lo, nloc, t) for t in range(nt)]
        deg = in_degrees(g) if topo == "Imp3D" else np.zeros(P, np.int64)
        out.append(Slab(lo, nloc, nt, tuple(int(deg[a:b].sum()) for a, b in rng), tuple(int(deg[a:b].max()) for a, b in rng),
                        tuple(b - a < tw.TILE for a, b in rng)))
    return out


def walks(topo, n, grid, ranks=1, walk=0, wx=8):
    """[(slab, mode, seq)] per rank (tile_walk_ref.tile_walk)."""
    g = emu.resolve(n, topo)[2]
    return [(s,) + tw.tile_walk(s.lo, s.nloc, g * g, grid, walk, wx) for s in slabs(topo, n, ranks)]


def pairs(seq):
    """Consecutive tiles of one block (empty items dropped)."""
    t = tw.tiles_of(seq)
    return list(zip(t, t[1:]))


def assert_multi_tile(topo, n, grid, ranks=1, walk=0, wx=8):
    """Static walks: some block of every slab runs two tiles, and every tile of the slab runs once."""
    for s, mode, seq in walks(topo, n, grid, ranks, walk, wx):
        assert mode != 3 and sorted(t for q in seq for t in tw.tiles_of(q)) == list(range(s.nt))
        assert max(len(tw.tiles_of(q)) for q in seq) >= 2, (topo, n, grid)


def median_cap(topo, n, ranks=1):
    return int(np.median([e for s in slabs(topo, n, ranks) for e in s.edges]))


N20, N9, N16, N32, N33, N40 = 8000, 729, 4096, 32 ** 3, 33 ** 3, 64000
IMP = (N20, "Imp3D", "push-sum")


# ================================================================ A. Imp3D push-sum, one rank
def a_seq(grid=1, cap=NO_CAP, wide_at=15):
    """g = 20 on `grid` blocks (walk 1 below 8 blocks): per block its tiles as (tile, staged, wide, partial)."""
    (s, mode, seq), = walks("Imp3D", N20, grid)
    assert mode == 1 and s.edges == (987, 1011, 1022, 1066, 1032, 1030, 1039, 813) and max(s.maxdeg) == 7
    assert s.partial == (False,) * 7 + (True,) and s.lo + s.nloc - 7 * 1024 == 832
    kind = [(t, s.edges[t] <= min(SLOTS, cap), s.maxdeg[t] >= wide_at, s.partial[t]) for t in range(s.nt)]
    return [[kind[t] for t in q] for q in seq]


def test_a1_one_block_runs_every_tile_in_order(monkeypatch):
    """GP_GRID=1, through convergence: tiles 0..7 in order on one block, every range and sender prefetch
    consumed, the partial tile last; activation (bitmap), every node active (redraw), alerts and the
    converged tail."""
    (seq,) = a_seq(1)
    assert [k[0] for k in seq] == list(range(8)) and all(k[1] and not k[2] for k in seq) and seq[-1][3]
    ref = reference(*IMP, None)
    assert ref.rounds == 428 and ref.alerts_total >= ref.T
    at32 = [st for k, a, st in ref.chunks][3]["flags"]
    assert np.all(at32 & 1)  # all active from round 32: both in-edge passes run for many rounds
    run(monkeypatch, *IMP, ref, 1)


@pytest.mark.parametrize("cap,pattern,limit", [(1025, "SSSUUUUS", 96), (1031, "SSSUUSUS", None)])
def test_a2_staged_and_unstaged_tiles_alternate(cap, pattern, limit, monkeypatch):
    """GP_STAGE_CAP between the tiles' in-edge counts.  Whether the senders are copied ahead depends on the
    NEXT tile alone: staged -> staged and unstaged -> staged consume a copy made during a FULL / a general
    node phase; staged -> unstaged and unstaged -> unstaged skip it and invalidate snd_tile, and the
    unstaged tile reads its in-edges one by one from the prefetched range."""
    (seq,) = a_seq(1, cap=cap)
    got = "".join("S" if k[1] else "U" for k in seq)
    assert got == pattern and {a + b for a, b in zip(got, got[1:])} == {"SS", "SU", "UU", "US"}
    run(monkeypatch, *IMP, reference(*IMP, limit), 1, GP_STAGE_CAP=cap)


def test_a3_wide_and_full_tiles_alternate(monkeypatch):
    """GP_IND4_WIDE=7: only the tiles holding a node of in-degree 7 read in_off per node."""
    (seq,) = a_seq(1, wide_at=7)
    got = "".join("W" if k[2] else "F" for k in seq)
    assert {"WF", "FW"} <= {a + b for a, b in zip(got, got[1:])}, got
    run(monkeypatch, *IMP, reference(*IMP, None), 1, GP_IND4_WIDE=7)


def test_a4_unpacked_senders(monkeypatch):
    """GP_NO_PACK=1: the prefetched senders are plain in_src words (degree recomputed per edge)."""
    a_seq(1)
    run(monkeypatch, *IMP, reference(*IMP, None), 1, GP_NO_PACK=1)


@pytest.mark.parametrize("grid,fuse", [(3, None), (5, None), (3, 0), (3, 1)])
def test_a5_strided_sequences_and_small_grid_round_close(grid, fuse, monkeypatch):
    """3 and 5 blocks: strided sequences of 3 3 2 and 2 2 2 1 1 tiles, and the round close on a grid
    below 8 (block_done_close_sharded with G < 8; GP_FUSE=1 the single counter, 0 k_finalize).
    GP_CHECK_CLOSE recounts the alerted nodes from the state after every step."""
    seq = a_seq(grid)
    assert [[k[0] for k in q] for q in seq] == [list(range(b, 8, grid)) for b in range(grid)]
    assert len({len(q) for q in seq}) == 2 and min(len(q) for q in seq) >= 1
    extra = {} if fuse is None else {"GP_FUSE": fuse}
    run(monkeypatch, *IMP, reference(*IMP, None), grid, GP_CHECK_CLOSE=1, **extra)


@pytest.mark.parametrize("n,walk,cap", [(n, w, False) for n in (N32, N33) for w in (0, 1, 2)] + [(N33, 2, True)])
def test_a6_static_walks(n, walk, cap, monkeypatch):
    """GP_WALK 0 / 1 / 2 on 8 blocks, x-windows of 3 planes.  g = 32: a plane is exactly one tile, 32
    tiles; g = 33: planes straddle tiles, the last tile is partial.  Every block runs >= 3 tiles; walk 2
    meets an empty item between two tiles of a block (the `continue`, with the prefetch of the tile
    before it still pending)."""
    (s, mode, seq), = walks("Imp3D", n, 8, walk=walk, wx=3)
    assert mode == walk and sorted(t for q in seq for t in tw.tiles_of(q)) == list(range(s.nt))
    assert min(len(tw.tiles_of(q)) for q in seq) >= 3
    assert s.partial[-1] == (n == N33) and s.nt == (32 if n == N32 else 36)
    if walk == 2:
        def gap(q):  # an empty item with a tile before and after it
            idx = [i for i, t in enumerate(q) if t is not tw.EMPTY]
            return any(b - a > 1 for a, b in zip(idx, idx[1:]))
        assert any(gap(q) for q in seq)
    extra = {}
    if cap:
        extra["GP_STAGE_CAP"] = median_cap("Imp3D", n)
        kinds = {(s.edges[a] <= extra["GP_STAGE_CAP"], s.edges[b] <= extra["GP_STAGE_CAP"]) for q in seq for a, b in pairs(q)}
        assert len(kinds) == 4  # S->S, S->U, U->U, U->S
    run(monkeypatch, n, "Imp3D", "push-sum", reference(n, "Imp3D", "push-sum", 96), 8, GP_WALK=walk, GP_WX=3, **extra)


def walk3_queues(n, grid, wx, ranks=1):
    out = []
    for s, mode, q in walks("Imp3D", n, grid, ranks, walk=3, wx=wx):
        assert mode == 3 and sorted(t for c in q for t in c) == list(range(s.nt))
        out.append((s, q))
    return out


A7 = [(n, grid, wx, 96, False) for n in (N32, N33, N40) for grid in (8, 16) for wx in (3, 16)] + \
     [(N33, 8, 3, None, False), (N40, 16, 3, 96, True)]


@pytest.mark.parametrize("n,grid,wx,limit,cap", A7)
def test_a7_walk3_queues_and_stealing(n, grid, wx, limit, cap, monkeypatch):
    """GP_WALK=3 forced: every XCD queue holds >= 2 tiles, so a block claims a second item while it runs
    its first (L.qn by parity), runs its own queue in order (8 blocks: alone) and then steals."""
    (s, q), = walk3_queues(n, grid, wx)
    assert min(len(c) for c in q) >= 2
    extra = {}
    if cap:
        extra["GP_STAGE_CAP"] = median_cap("Imp3D", n)
        assert 0 < sum(e <= extra["GP_STAGE_CAP"] for e in s.edges) < s.nt
    run(monkeypatch, n, "Imp3D", "push-sum", reference(n, "Imp3D", "push-sum", limit), grid, GP_WALK=3, GP_WX=wx, **extra)


@pytest.mark.parametrize("n,sizes", [(N20, [1] * 8), (N16, [1, 0] * 4), (N9, [1] + [0] * 7)])
def test_a8_walk3_short_and_empty_queues(n, sizes, monkeypatch):
    """Queues of one tile and of none.  g = 20: eight tiles, one per queue -- every block's second claim
    is past the end, and it then tries the seven other queues in vain.  g = 16: four tiles in the even
    queues -- the odd blocks' first claim is already past the end and they steal at once.  g = 9: seven
    empty queues, and the one tile is partial."""
    (s, q), = walk3_queues(n, 8, 16)
    assert [len(c) for c in q] == sizes
    assert s.partial[-1] == (n != N16) and s.nt == sum(sizes)
    ref = reference(n, "Imp3D", "push-sum", None)
    assert ref.alerts_total >= ref.T
    run(monkeypatch, n, "Imp3D", "push-sum", ref, 8, GP_WALK=3, GP_WX=16)


# ================================================================ B. Imp3D push-sum across virtual ranks
B = [(n, ranks, grid, walk, False) for n, ranks in ((N32, 2), (N33, 2), (N33, 3)) for grid in (1, 8) for walk in (None, 3)] + \
    [(N33, 2, 8, 3, True)]


@pytest.mark.parametrize("n,ranks,grid,walk,cap", B)
def test_b_remote_kernel_sequences(n, ranks, grid, walk, cap, monkeypatch):
    """k_ps_tile<IMP3D, true>: no sender prefetch, the range prefetch only.  g = 32 on two ranks: slabs of
    16 whole tiles; g = 33: slab 1 (and the middle slab of three) begins below its first tile's end and
    slabs end inside a tile, so partial tiles run with a tile after them (first) or before and, in the
    walk-3 queues, after them (last)."""
    model = walks("Imp3D", n, grid, ranks, walk=0 if walk is None else 3, wx=8)
    for s, mode, seq in model:
        assert sorted(t for q in seq for t in q) == list(range(s.nt))  # (walks 0, 1, 3: no empty items)
        assert mode == (1 if grid == 1 else 0 if walk is None else 3) and max(s.edges) <= SLOTS_REMOTE
        assert max(len(q) for q in seq) >= 2
    if n == N32:
        assert [(s.nt, any(s.partial)) for s, _, _ in model] == [(16, False)] * 2
    else:
        first = [s for s, _, _ in model if s.partial[0]]
        last = [(s, seq) for s, _, seq in model if s.partial[-1]]
        assert len(first) == ranks - 1 and len(last) >= ranks - 1
        for s, mode, seq in model:  # the partial first tile is followed by another tile of its block, but
            if s.partial[0]:        # for walk 0 on 8 blocks of a 13-tile slab, whose block 0 runs one tile
                assert any(a == 0 for q in seq for a, b in zip(q, q[1:])) == ((ranks, grid, walk) != (3, 8, None))
        for s, seq in last:         # the partial last tile is preceded by one
            assert any(b == s.nt - 1 for q in seq for a, b in zip(q, q[1:]))
        if walk == 3 and grid == 8:  # ... and, in some queue, followed by one: mid-sequence
            assert any(a == s.nt - 1 for s, seq in last for q in seq for a, b in zip(q, q[1:]))
    extra = {} if walk is None else {"GP_WALK": 3, "GP_WX": 8}
    if cap:
        extra["GP_STAGE_CAP"] = median_cap("Imp3D", n, ranks)
        assert all(0 < sum(e <= extra["GP_STAGE_CAP"] for e in s.edges) < s.nt for s, _, _ in model)
    run(monkeypatch, n, "Imp3D", "push-sum", reference(n, "Imp3D", "push-sum", 96), grid, ranks=ranks, **extra)


# ================================================================ C. 3D and line push-sum, both size classes
@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("grid", [1, 3, 8])
@pytest.mark.parametrize("n", [N20, N33])
def test_c_3d_both_size_classes(n, grid, wide, monkeypatch):
    """200 rounds (every node active, the first alerts).  8 blocks on the 8 tiles of g = 20 is the control:
    one tile per block, as on the product's grid."""
    if (n, grid) != (N20, 8):
        assert_multi_tile("3D", n, grid)
    run(monkeypatch, n, "3D", "push-sum", reference(n, "3D", "push-sum", 200), grid, wide=wide)


@functools.lru_cache(maxsize=None)
def line_all_active_round(n):
    orc = Oracle(n, "line", "push-sum", SEED)
    while orc.active_count() < orc.P:
        assert orc.rounds < 20000
        orc.step(1)
    r = orc.rounds
    orc.close()
    return r


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("grid", [1, 2])
def test_c_line_both_size_classes(grid, wide, monkeypatch):
    """P = 3001: 3 tiles, the last of 953 nodes; through activation (the oracle's first round with every
    node active, asserted <= 20000) and 64 rounds on."""
    (s,) = slabs("line", 3000)
    assert s.nt == 3 and s.lo + s.nloc - 2048 == 953
    assert_multi_tile("line", 3000, grid)
    r = line_all_active_round(3000)
    assert 64 < r <= 20000
    run(monkeypatch, 3000, "line", "push-sum", reference(3000, "line", "push-sum", r + 64, 256), grid, wide=wide)


# ================================================================ D. gossip tile kernel
def gossip_ref(n, topo):
    """Line: through convergence.  Lattices: 96 (3D) / 64 (Imp3D) rounds, by when -- asserted from the
    oracle's last compared state -- every node has been reached and at least half have converged."""
    if topo == "line":
        ref = reference(n, topo, "gossip", None, 256)
        assert ref.alerts_total >= ref.T
        return ref
    ref = reference(n, topo, "gossip", 96 if topo == "3D" else 64)
    c = ref.chunks[-1][2]["c"]
    assert ref.alerts_total >= ref.T or (c.min() >= 1 and 2 * np.count_nonzero(c > 10) >= c.size)
    return ref


@pytest.mark.parametrize("grid", [1, 3, 8])
@pytest.mark.parametrize("n,topo", [(N20, "Imp3D"), (N20, "3D"), (N33, "3D"), (3000, "line")])
def test_d_gossip_sequences(n, topo, grid, monkeypatch):
    """k_gossip_tile restages its LDS buffers tile after tile (no prefetch).  8 blocks on 8 (g = 20) or 3
    (line) tiles are the controls."""
    if grid < slabs(topo, n)[0].nt:
        assert_multi_tile(topo, n, grid)
    run(monkeypatch, n, topo, "gossip", gossip_ref(n, topo), grid)


@pytest.mark.parametrize("cap,pattern", [(1025, "SSSUUUUS"), (1031, "SSSUUSUS")])
def test_d_gossip_staged_and_unstaged_alternate(cap, pattern, monkeypatch):
    (seq,) = a_seq(1, cap=cap)
    assert "".join("S" if k[1] else "U" for k in seq) == pattern and max(slabs("Imp3D", N20)[0].edges) <= SRC_CAP
    run(monkeypatch, N20, "Imp3D", "gossip", gossip_ref(N20, "Imp3D"), 1, GP_STAGE_CAP=cap)


@pytest.mark.parametrize("grid", [1, 8])
def test_d_gossip_two_virtual_ranks(grid, monkeypatch):
    """k_gossip_tile<IMP3D, true> at g = 33: slab 1 begins inside a tile, both end inside one."""
    model = walks("Imp3D", N33, grid, 2)
    assert model[1][0].partial[0] and all(s.partial[-1] for s, _, _ in model)
    assert_multi_tile("Imp3D", N33, grid, 2)
    run(monkeypatch, N33, "Imp3D", "gossip", gossip_ref(N33, "Imp3D"), grid, ranks=2)
