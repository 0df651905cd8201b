"""GPU: the Imp3D push-sum list exchange (gp_xchg.hip: k_list_count, k_list_key, k_list_pack; the tables
list_tables / list_hw / exchange_layout of gp_plan.hpp; the REMOTE read side of k_ps_tile) and the
compacted halo planes of lattice push-sum (k_halo<PACK> / <!PACK>, halo_chunk_cap, setup_halo) at their
structural edges: in-process virtual ranks against the single-rank C oracle, s, w, flags and per-round
alerts bit for bit at every checkpoint (every 15 rounds), rounds and alerts_total at the end.  No
tolerances.

Every case runs from round 0 until the oracle shows every node active and 20 rounds beyond (during
activation the header bit of a list entry decides on the read side, afterwards the sender's draw), and
every case first shows on the CPU -- before its simulation is created -- that it is where it claims to
be: from the plan restatements of tests/multirank_emu.py (slab_bounds, tiles_for, region_tiles, xregion,
ListPlan, halo_chunk_cap; tests/test_plan.py compares them with gp_plan.hpp at these shapes) and from the
oracle's own state (the senders of round r are the nodes whose active flag the oracle shows at its
start; a sender's direction is its Philox draw, Geometry.draw_dir).  Nothing of the demonstration reads
the library under test.  The oracle is stepped once per (g, topology) and shared by the cases.

A  tile alignment and k_list_pack's blocks (LP_TILES = 8 tiles, one per wave; ntl = tiles of the last
   block), product build: a plane that is one tile (g = 32) or four (g = 64), regions of 4, 8, 9, 13/14,
   16 and 32 tiles, slabs that begin and end inside a tile (g = 33), one plane per rank with the whole
   slab inside one tile and regions without a tile (g = 5, 3, 2), and a rank that receives no list
   entry at all (xnv = 1: the read side clamps every index to slot 0).
B  segment word counts: (tile, destination) segments of 63, 64 and 65 entries with bit 63 of the first
   word and the one bit of the second word used in an executed round (g = 64, W = 16), and empty
   segments in the leading, a middle and the trailing position of a tile's words (g = 19, W = 16).
C  eight exchange regions at two ranks (GP_XREGIONS=8, experiments build), with one round launch and
   with eight region launches per round (GP_RREGIONS=1, GP_WALK=3: receive buffer by round parity), and
   at g = 6, where most of the eight regions hold no plane.
D  the capacity comparisons, experiments build: GP_XCAP / GP_HALO_CAP at M, the most entries any one
   buffer / halo chunk holds in any round of the run (bit-exact: the last slot is used), and at M - 1
   (the step fails with GP_ESTATE "overflow", the simulation closes, a fresh default one is bit-exact).
E  the halo compaction switch, product build: g = 31 (full planes travel), 32 (one full chunk), 33 (a
   second chunk of 65 nodes), 3D and Imp3D, W = 2 and 3.

The stores and loads the M - 1 cases reach were read before those cases were first run; each is bounded
by the capacity the run was given.  k_list_pack: a message goes to ovals[d] + idx only if idx <
ocap[d], idx counted from the chunk's first slot (the block's reservation off[d] + the tile's run +
wb + the bits below), and ocap[d] is the overridden capacity exchange_layout sized the chunk with; the
header words go to gw + (l - lw), which no capacity enters.  A header's base may point past its chunk
after an overflow; the read side takes min(base + popcount, xnv - 1), and xnv is the sum of the
overridden capacities (at least 1), the size of the vals region the receive buffer was allocated with.
k_halo: both template sides form the slot address blockIdx.x * cap + rank but touch it only if rank <
cap (PACK: else the overflow flag; !PACK: else the halo node keeps its old value, silently -- the
packing rank has raised the flag for the same direction bytes); halo_buf_slots sizes hsend / hrecv and
the transfer from the overridden cap.  Nothing was found unbounded.  The point of D is the designed
error path, not a fault.
"""
import functools

import numpy as np
import pytest

from tests.multirank_emu import (DIR_RANDOM, HALO_CHUNK, S_PUSHSUM, S_TOPO, XTILE, Geometry, ListPlan, halo_chunk_cap,
                                 region_tiles, slab_bounds, tiles_for, uniform, xregion)
from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim, assert_same_state

pytestmark = pytest.mark.gpu

SEED = 1
CHK = 15       # rounds per checkpoint
BEYOND = 20    # rounds past the first one every node is active in
LP_TILES = 8   # gp_xchg.hip


# ---------------------------------------------------------------- the oracle's run, once per (g, topology, seed)
class Trace:
    """R rounds of the oracle, stepped one at a time: active[r] the senders of round r (0..R: the lists
    of round R are packed behind round R - 1), alerts per round, the state after every CHK rounds and
    after R."""


@functools.lru_cache(maxsize=None)
def trace(g, topo, seed=SEED):
    t = Trace()
    t.P = g ** 3
    orc = Oracle(t.P, topo, "push-sum", seed)
    assert orc.P == orc.T == t.P
    t.active, t.alerts, t.states, t.full = [], [], {}, None
    while True:
        st = orc.state()
        r = len(t.alerts)
        t.active.append((st["flags"] & 1) != 0)
        if t.full is None and t.active[-1].all():
            t.full = r
        last = t.full is not None and r >= t.full + BEYOND
        if r and (r % CHK == 0 or last):
            for v in st.values():
                v.setflags(write=False)
            t.states[r] = st
        if last:
            break
        assert r < 1000, "activation did not complete"
        assert orc.alerts_total < orc.T, "converged before every node was active for 20 rounds"
        t.alerts += orc.step(1)
        assert len(t.alerts) == r + 1
    t.R = len(t.alerts)
    t.alerts_total = orc.alerts_total
    assert t.alerts_total < orc.T  # still running: the library executes all R rounds as well
    orc.close()
    return t


@functools.lru_cache(maxsize=None)
def directions(g, topo, seed=SEED):
    """dirs[r][i]: the direction node i sends in during round r (0..R), -1 if it is not active."""
    t, geo = trace(g, topo, seed), Geometry(g ** 3, g, topo, seed)
    out = []
    for r in range(t.R + 1):
        d = np.full(t.P, -1, dtype=np.int8)
        ids = np.nonzero(t.active[r])[0]
        d[ids] = geo.draw_dir(ids, S_PUSHSUM, r)
        out.append(d)
    return out


class World:
    """Slabs, tiles, regions and (Imp3D) the list plan of g^3 nodes on W ranks with NH regions."""

    def __init__(self, g, W, topo, seed, NH):
        self.g, self.W, self.P, self.NH = g, W, g ** 3, NH
        self.bounds, self.halo = slab_bounds(self.P, g, topo, W)
        assert self.halo == g * g and self.bounds[0] == 0 and self.bounds[-1] == self.P
        self.lo = self.bounds[:-1]
        self.n = [self.bounds[w + 1] - self.bounds[w] for w in range(W)]
        self.nt = [tiles_for(lo, n) for lo, n in zip(self.lo, self.n)]
        self.tb = [region_tiles(lo, n, g * g, NH, nt) for lo, n, nt in zip(self.lo, self.n, self.nt)]
        for w in range(W):  # the regions' senders are consecutive and cover the slab
            reg = [xregion(self.lo[w], self.n[w], self.tb[w], NH, h) for h in range(NH)]
            assert reg[0][0] == 0 and reg[-1][1] == self.n[w] and all(p[1] == q[0] for p, q in zip(reg, reg[1:]))
        if topo == "Imp3D":
            geo = Geometry(self.P, g, topo, seed)
            self.rnd = uniform(seed, S_TOPO, np.arange(self.P), 0, self.P - 1)
            self.plan = ListPlan(self.P, g, W, self.bounds, self.rnd, geo, NH=NH)
            pl = self.plan
            self.remote = pl.owner != pl.slab  # the list entries
            # every entry's (slab, tile, destination) segment, its size and the entry's rank in it
            tile = np.arange(self.P) // XTILE - np.array(self.lo)[pl.slab] // XTILE
            self.seg = (pl.slab * (max(self.nt) + 1) + tile) * W + pl.owner
            ids = np.nonzero(self.remote)[0]
            _, first, inv, cnt = np.unique(self.seg[ids], return_index=True, return_inverse=True, return_counts=True)
            self.seg_n = np.zeros(self.P, dtype=np.int64)
            self.rho = np.full(self.P, -1, dtype=np.int64)
            self.seg_n[ids] = cnt[inv]
            self.rho[ids] = pl.key_local[ids] - pl.key_local[ids[first]][inv]
            assert np.all((self.rho[ids] >= 0) & (self.rho[ids] < self.seg_n[ids]))

    def region_tile_counts(self, w):
        return np.diff(self.tb[w]).tolist()

    def pack_blocks(self, w):
        """ntl of every k_list_pack block of rank w, region by region."""
        return [[min(LP_TILES, n - k) for k in range(0, n, LP_TILES)] for n in self.region_tile_counts(w)]


@functools.lru_cache(maxsize=None)
def world(g, W, topo="Imp3D", seed=SEED, NH=4):
    return World(g, W, topo, seed, NH)


def used_entries(g, W, seed=SEED, NH=4):
    """Per round 0..R: the ids of the list entries in use (active senders whose draw is the random edge
    and whose random edge leaves their slab)."""
    wd = world(g, W, "Imp3D", seed, NH)
    return [np.nonzero((d == DIR_RANDOM) & wd.remote)[0] for d in directions(g, "Imp3D", seed)]


def run_exact(g, W, topo, monkeypatch=None, env=None, seed=SEED, regions=None):
    """The library on W virtual ranks against the oracle's trace, checkpoint by checkpoint."""
    t = trace(g, topo, seed)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    sim = Sim(t.P, topo, "push-sum", seed=seed, virtual_ranks=W, experimental=bool(env))
    try:
        assert sim.info().num_gpus == W and sim.population == t.P
        if regions is not None:
            assert sim._L.gp_debug_round_regions(sim._h) == regions
        done = 0
        while done < t.R:
            k = min(CHK, t.R - done)
            assert sim.step(k) == t.alerts[done:done + k], f"alerts differ in rounds {done}..{done + k}"
            done += k
            try:
                assert_same_state("push-sum", sim.state(), t.states[done])
            except AssertionError as e:
                raise AssertionError(f"state differs after round {done}: {e}") from None
        assert sim.rounds == t.R and sim.alerts_total == t.alerts_total
    finally:
        sim.close()
        for k in env or {}:
            monkeypatch.delenv(k)


def run_overflow(g, W, topo, monkeypatch, env, seed=SEED):
    """One slot short: the step fails with GP_ESTATE "overflow", the simulation closes, and a fresh
    default one is bit-exact (nothing was written past a buffer)."""
    from gossipprotocol_amd._lib import GossipError
    t = trace(g, topo, seed)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    sim = Sim(t.P, topo, "push-sum", seed=seed, virtual_ranks=W, experimental=True)
    try:
        with pytest.raises(GossipError) as e:
            sim.step(t.R)
        assert e.value.code == -5 and "overflow" in str(e.value)
    finally:
        sim.close()
        for k in env:
            monkeypatch.delenv(k)
    run_exact(g, W, topo, seed=seed)


def both_phases(g, W, seed=SEED, NH=4):
    """List entries are in use while some node is still inactive (the header bit decides) and in the
    rounds after (the draw decides) -- for every ordered pair of ranks that has entries at all."""
    t, wd, used = trace(g, "Imp3D", seed), world(g, W, "Imp3D", seed, NH), used_entries(g, W, seed, NH)
    assert t.R == t.full + BEYOND
    pl = wd.plan
    pair = lambda ids: set((pl.slab[ids] * W + pl.owner[ids]).tolist())
    have = pair(np.nonzero(wd.remote)[0])
    early = set().union(*[pair(u) for u in used[:t.full]])
    late = set().union(*[pair(u) for u in used[t.full:t.R]])
    assert early and late == have
    return early, late


# ---------------------------------------------------------------- A: tile alignment and pack blocks
def test_plane_is_one_tile():
    """g = 32, W = 2: a plane is exactly one tile, a slab 16 tiles, regions of 4 tiles -- every
    k_list_pack block has ntl = 4, waves 4-7 idle."""
    wd = world(32, 2)
    assert wd.g ** 2 == XTILE and wd.nt == [16, 16] and all(lo % XTILE == 0 for lo in wd.lo)
    for w in range(2):
        assert wd.region_tile_counts(w) == [4] * 4 and wd.pack_blocks(w) == [[4]] * 4
    both_phases(32, 2)
    run_exact(32, 2, "Imp3D")


@pytest.mark.parametrize("W,tiles,blocks", [(4, 16, [8, 8]), (2, 32, [8, 8, 8, 8]), (8, 8, [8])], ids=["W4", "W2", "W8"])
def test_plane_is_four_tiles(W, tiles, blocks):
    """g = 64: a plane is four tiles; W = 4: regions of 16 tiles, two full blocks; W = 2: 32 tiles, four
    full blocks; W = 8: 8 tiles, exactly one block."""
    wd = world(64, W)
    assert wd.g ** 2 == 4 * XTILE and all(lo % XTILE == 0 for lo in wd.lo)
    for w in range(W):
        assert wd.region_tile_counts(w) == [tiles] * 4 and wd.pack_blocks(w) == [blocks] * 4
    both_phases(64, W)
    run_exact(64, W, "Imp3D")


@pytest.mark.parametrize("W,sizes,blocks", [(2, {13, 14}, {(8, 5), (8, 6)}), (3, {9}, {(8, 1)})], ids=["W2", "W3"])
def test_second_block_partial(W, sizes, blocks):
    """g = 48 (g^2 = 2304, no plane on a tile boundary).  W = 2: regions of 13 or 14 tiles, one full
    block and one of 5 or 6; W = 3: every region 9 tiles, a second block with ntl = 1."""
    wd = world(48, W)
    assert wd.g ** 2 % XTILE != 0
    got_sizes, got_blocks = set(), set()
    for w in range(W):
        got_sizes |= set(wd.region_tile_counts(w))
        got_blocks |= set(tuple(b) for b in wd.pack_blocks(w))
    assert got_sizes == sizes and got_blocks == blocks
    both_phases(48, W)
    run_exact(48, W, "Imp3D")


@pytest.mark.parametrize("W", [2, 3])
def test_slabs_begin_and_end_inside_a_tile(W):
    """g = 33: a plane is 1089 = 1024 + 65 ids, so every slab but the first begins and every slab but
    the last ends inside a tile (tile_span: j0 > T, j1 < T + 1024); W = 3 has a middle rank with both.
    The tile two slabs share holds entries of both."""
    wd = world(33, W)
    for w in range(W):
        assert (wd.lo[w] % XTILE != 0) == (w > 0) and (wd.bounds[w + 1] % XTILE != 0)
        assert wd.nt[w] == -(-wd.bounds[w + 1] // XTILE) - wd.lo[w] // XTILE
        assert sum(wd.region_tile_counts(w)) == wd.nt[w]
    if W == 3:
        assert wd.lo[1] % XTILE and wd.bounds[2] % XTILE
    used = np.concatenate(used_entries(33, W))
    for w in range(1, W):  # used entries on both sides of the slab bound, inside the shared tile
        T = wd.lo[w] // XTILE * XTILE
        assert np.any((used >= T) & (used < wd.lo[w])) and np.any((used >= wd.lo[w]) & (used < T + XTILE))
    both_phases(33, W)
    run_exact(33, W, "Imp3D")


@pytest.mark.parametrize("g", [5, 3, 2])
def test_one_plane_per_rank(g):
    """W = g: every rank owns one plane -- its lower and its upper boundary plane at once -- inside one
    tile; regions 0-2 hold no tile (no k_list_pack launch), region 3 the slab's one."""
    wd = world(g, g)
    for w in range(g):
        assert wd.n[w] == g * g and wd.nt[w] == 1 and wd.bounds[w + 1] <= XTILE
        assert wd.region_tile_counts(w) == [0, 0, 0, 1]
        assert [xregion(wd.lo[w], wd.n[w], wd.tb[w], 4, h) for h in range(4)] == [(0, 0)] * 3 + [(0, g * g)]
    assert g * g < HALO_CHUNK  # the halo planes travel whole
    both_phases(g, g)
    run_exact(g, g, "Imp3D")


def no_entry_seed(g, W):
    """The first seed of 1..32 for which one rank receives no list entry."""
    for seed in range(1, 33):
        pl = world(g, W, "Imp3D", seed).plan
        into = [sum(int(pl.nw[a, h, b]) for a in range(W) for h in range(4)) for b in range(W)]
        if min(into) == 0 and max(into) > 0:
            return seed, into.index(0)
    return None


def test_rank_without_list_entries():
    """g = 2, W = 2 (slabs of one plane, 4 nodes): for the first seed with no random edge from one slab
    into the other, the receiving rank has no header word and no slot (xnv = 1, an empty vals region;
    k_list_pack's reservation takes its r = 0 path for every destination on the sending side), while
    the other direction carries messages."""
    found = no_entry_seed(2, 2)
    assert found is not None
    seed, b = found
    a = 1 - b
    pl = world(2, 2, "Imp3D", seed).plan
    assert pl.nw[a, :, b].sum() == 0 and pl.cap[:, a, b].sum() == 0  # nothing a -> b: b's xnv = max(1, 0)
    assert pl.nw[b, :, a].sum() > 0 and pl.cap[:, b, a].sum() > 0
    used = np.concatenate(used_entries(2, 2, seed))
    assert len(used) and np.all(pl.slab[used] == b)
    run_exact(2, 2, "Imp3D", seed=seed)


# ---------------------------------------------------------------- B: segment word edges
def test_segments_of_63_64_65_entries():
    """g = 64, W = 16: slabs of 4 planes = 16 aligned tiles, entries per (tile, destination) ~
    Binomial(1024, 1/16).  Among the segments there are some of 63, 64 (one full word) and 65 entries (a
    second word with one bit: rho >> 6 and wb cross into it); in executed rounds bit 63 of a 64- and of
    a 65-segment's first word is used, and the one entry of a 65-segment's second word (rho = 64)."""
    g, W = 64, 16
    wd, t = world(g, W), trace(g, "Imp3D")
    assert all(lo % XTILE == 0 for lo in wd.lo) and wd.nt == [16] * W
    sizes = set(wd.seg_n[wd.remote].tolist())
    assert {63, 64, 65} <= sizes and max(sizes) <= XTILE
    used = np.unique(np.concatenate(used_entries(g, W)[:t.R]))
    hit = lambda n, rho: int(np.sum((wd.seg_n[used] == n) & (wd.rho[used] == rho)))
    assert hit(64, 63) and hit(65, 63) and hit(65, 64) and hit(63, 62)
    # ... and in one round both words of one 65-segment are in use (wb of the second word > 0)
    both = 0
    for u in used_entries(g, W)[:t.R]:
        u65 = u[wd.seg_n[u] == 65]
        second = set(wd.seg[u65[wd.rho[u65] == 64]].tolist())
        both += len(second & set(wd.seg[u65[wd.rho[u65] < 64]].tolist()))
    assert both
    both_phases(g, W)
    run_exact(g, W, "Imp3D")


def empty_segment_positions(g, W, seed):
    """Tiles with an empty (tile, destination) segment in the leading, a middle, the trailing position
    of their words, counted only where an entry of a later segment of the tile (trailing: of an earlier
    one, there is no later) is in use in an executed round."""
    wd, t = world(g, W, "Imp3D", seed), trace(g, "Imp3D", seed)
    pl = wd.plan
    used = np.unique(np.concatenate(used_entries(g, W, seed)[:t.R]))
    seen = {"leading": 0, "middle": 0, "trailing": 0}
    for a in range(W):
        ids = np.arange(wd.lo[a], wd.bounds[a + 1])
        tile = ids // XTILE - wd.lo[a] // XTILE
        dests = [d for d in range(W) if d != a]
        for tt in range(wd.nt[a]):
            sel = ids[(tile == tt) & wd.remote[ids]]
            n = np.bincount(pl.owner[sel], minlength=W)
            u = np.bincount(pl.owner[np.intersect1d(sel, used)], minlength=W)
            if n[dests[0]] == 0 and u[dests[1:]].any():
                seen["leading"] += 1
            if n[dests[-1]] == 0 and u[dests[:-1]].any():
                seen["trailing"] += 1
            for k in range(1, len(dests) - 1):
                if n[dests[k]] == 0 and n[dests[:k]].any() and u[dests[k + 1:]].any():
                    seen["middle"] += 1
    return seen


# (g = 20, the size first meant for this case, shows no leading and no trailing empty segment with a used
# entry beside it for any seed 1..32, nor does g = 18; g = 19 does for seed 1)
EMPTY_G, EMPTY_SEED = 19, 1


def test_empty_segments_leading_middle_trailing():
    """W = 16, slabs of one or two planes cut by the tiles, so some tiles hold a few dozen senders
    and have destinations without an entry.  Shown: a tile whose lowest destination rank has an empty
    segment, one with an empty segment between two non-empty ones, and one whose highest destination
    rank has none (the seg search and the tn / wb scans of k_list_pack see lw[d] == lw[d + 1] in each
    position), each with a used entry behind (trailing: before) it in an executed round."""
    g, W, seed = EMPTY_G, 16, EMPTY_SEED
    wd = world(g, W, "Imp3D", seed)
    assert set(wd.n) <= {g * g, 2 * g * g}
    seen = empty_segment_positions(g, W, seed)
    assert all(seen.values()), seen
    both_phases(g, W, seed)
    run_exact(g, W, "Imp3D", seed=seed)


# ---------------------------------------------------------------- C: eight regions
REGION_ROUNDS = {"GP_XREGIONS": 8, "GP_RREGIONS": 1, "GP_WALK": 3}


@pytest.mark.parametrize("form", ["one_launch", "region_launches"])
@pytest.mark.parametrize("g", [33, 64, 6])
def test_eight_regions_at_two_ranks(g, form, monkeypatch):
    """W = 2 with the eight exchange regions of two large slabs (GP_XREGIONS=8).  g = 64: regions of 4
    planes = 16 tiles; g = 33: of 2 or 3 planes that begin inside tiles; g = 6: 3 planes in 8 regions,
    all inside tile 0 -- five regions hold no plane and seven no tile.  region_launches: the round
    kernel runs region by region, eight launches per round (RREG_MAX), the receive buffer by round
    parity."""
    wd = world(g, 2, NH=8)
    for w in range(2):
        planes = wd.n[w] // (g * g)
        per = [planes * (h + 1) // 8 - planes * h // 8 for h in range(8)]
        cnt = wd.region_tile_counts(w)
        assert len(cnt) == 8 and sum(cnt) == wd.nt[w]
        if g == 64:
            assert per == [4] * 8 and cnt == [16] * 8
        elif g == 33:
            assert set(per) <= {2, 3} and min(cnt) >= 2
        else:
            assert planes == 3 and per.count(0) == 5 and cnt.count(0) == 7 and wd.nt[w] == 1
    pl = wd.plan
    assert pl.nw.shape == (2, 8, 2)
    if g != 6:  # every region's chunk carries entries, both ways
        assert np.all(pl.nw[0, :, 1] > 0) and np.all(pl.nw[1, :, 0] > 0)
    both_phases(g, 2, NH=8)
    if form == "one_launch":
        run_exact(g, 2, "Imp3D", monkeypatch, {"GP_XREGIONS": 8}, regions=1)
    else:
        run_exact(g, 2, "Imp3D", monkeypatch, REGION_ROUNDS, regions=8)


# ---------------------------------------------------------------- D: capacities at M and M - 1
def fullest_list_buffer(g, W):
    """(M, round, (h, a, b)): the most entries one buffer (region h, a -> b) holds in any round 0..R."""
    wd, t = world(g, W), trace(g, "Imp3D")
    pl = wd.plan
    best = (0, None, None)
    for r, u in enumerate(used_entries(g, W)):
        key = (pl.region[u] * W + pl.slab[u]) * W + pl.owner[u]
        cnt = np.bincount(key, minlength=4 * W * W)
        assert np.all(cnt.reshape(4, W, W) <= pl.cap)  # the plan's own buffers hold every round
        if cnt.max() > best[0]:
            k = int(cnt.argmax())
            best = (int(cnt.max()), r, (k // (W * W), k // W % W, k % W))
    assert best[1] < t.R  # reached in an executed round, not only in the lists packed behind the last
    return best


def test_list_capacity_at_M_and_one_below(monkeypatch):
    """g = 33, W = 3: GP_XCAP at the fullest buffer's entries M (slot M - 1, the chunk's last, is
    written and read: k_list_pack's idx < ocap[d]) and at M - 1 (that entry has idx == ocap[d])."""
    g, W = 33, 3
    M, r, (h, a, b) = fullest_list_buffer(g, W)
    pl = world(g, W).plan
    assert 1 < M < pl.cap[h, a, b]  # the override lowers this buffer's capacity
    run_exact(g, W, "Imp3D", monkeypatch, {"GP_XCAP": M})
    run_overflow(g, W, "Imp3D", monkeypatch, {"GP_XCAP": M - 1})


def fullest_halo_chunk(g, W, topo):
    """(M, round, chunk): the most senders toward the neighbouring rank in one HALO_CHUNK-node chunk of a
    slab-boundary plane in any round 0..R (a plane's last, partial chunk is a chunk of its own)."""
    wd, t = world(g, W, topo), trace(g, topo)
    g2 = g * g
    best = (0, None, None)
    for r, d in enumerate(directions(g, topo)):
        for w in range(1, W):
            for start, toward in ((wd.bounds[w] - g2, 1), (wd.bounds[w], 0)):  # last plane up, first plane down
                s = np.nonzero(d[start:start + g2] == toward)[0]
                cnt = np.bincount(s // HALO_CHUNK, minlength=-(-g2 // HALO_CHUNK))
                if cnt.max() > best[0]:
                    best = (int(cnt.max()), r, int(cnt.argmax()))
    assert best[1] < t.R
    return best


@pytest.mark.parametrize("topo", ["Imp3D", "3D"])
def test_halo_capacity_at_M_and_one_below(topo, monkeypatch):
    """g = 33, W = 2: GP_HALO_CAP at the fullest chunk's senders M (k_halo's rank >= a.cap, both
    template sides: slot M - 1 is packed and expanded) and at M - 1."""
    g, W = 33, 2
    assert g * g >= HALO_CHUNK
    M, r, chunk = fullest_halo_chunk(g, W, topo)
    cap = halo_chunk_cap(g, topo == "Imp3D")
    assert 1 < M < cap and cap % 8 == 0
    assert halo_chunk_cap(g, False) > halo_chunk_cap(g, True)  # 3D: no random edge, more senders per plane
    assert chunk == 0  # the full chunk; the 65-node chunk behind it never comes near M
    run_exact(g, W, topo, monkeypatch, {"GP_HALO_CAP": M})
    run_overflow(g, W, topo, monkeypatch, {"GP_HALO_CAP": M - 1})


# ---------------------------------------------------------------- E: the halo compaction switch
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("topo", ["3D", "Imp3D"])
@pytest.mark.parametrize("g", [31, 32, 33])
def test_halo_compaction_switch(g, topo, W):
    """g = 31: the plane (961 nodes) is below HALO_CHUNK and travels whole; g = 32: one full chunk; g =
    33: two chunks, the second of 65 nodes (i < a.n inside a chunk, halo_buf_slots rounding up).  On
    every boundary plane, in some executed round, a sender toward the neighbour sits in the last
    chunk."""
    wd, t = world(g, W, topo), trace(g, topo)
    g2 = g * g
    chunks, last = -(-g2 // HALO_CHUNK), g2 - (g2 - 1) // HALO_CHUNK * HALO_CHUNK
    assert (g2 >= HALO_CHUNK, chunks, last) == {31: (False, 1, 961), 32: (True, 1, 1024), 33: (True, 2, 65)}[g]
    dirs = directions(g, topo)[:t.R]
    for w in range(1, W):
        for start, toward in ((wd.bounds[w] - g2, 1), (wd.bounds[w], 0)):
            tail = slice(start + (chunks - 1) * HALO_CHUNK, start + g2)
            assert any(np.any(d[tail] == toward) for d in dirs)
            assert max(int(np.sum(d[tail] == toward)) for d in dirs) <= halo_chunk_cap(g, topo == "Imp3D")
    run_exact(g, W, topo)
