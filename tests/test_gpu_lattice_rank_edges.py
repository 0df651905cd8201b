"""GPU: the plain lattices -- the line and the 3D grid -- across ranks, with the slab cuts put where the
tile kernels change mechanism: k_ps_tile / wide::k_ps_tile (gp_ps_tile.hip, gp_ps_tile_wide.hip) and
k_gossip_tile (gp_gossip_tile.hip) for LINE and GRID3D, the halo refresh of gp_exchange.hip between them.
In-process virtual ranks against the single-rank C oracle: s and w as raw bits, flags (gossip: c and
flags) and the per-round alerts at every checkpoint (every 64 rounds; every 256 in the 4096-round cases;
and at the end), rounds and alerts_total at the end.  No tolerances.

The line is the one topology whose slab bounds are arbitrary ids (slab_bounds: P w / W, a halo of one
node), while tiles sit on global multiples of 1024, waves on multiples of 64 and the node slots of the
256 x 4 class on k 256 + tid.  The push-sum tile kernel takes a node's j +- 1 neighbour from the next
lane (DPP), from the per-wave end gather L.zb (its index clamped into [ext_lo, ext_hi]) or by a load,
and its sender test from the staged direction bytes, depending on where the neighbour sits; a tile
wholly inside the slab runs the FULL body, every other the general one.

A  line, W = 2, the cut one id short of, on and one id past a tile end (P = 2046, 2048, 2050: at 2048
   each slab is exactly one tile -- FULL body, both halo nodes the clamped ends of zb; at 2050 rank 0
   has a second tile of one node), around the wave end inside tile 1 (P = 2174, 2176, 2178) and on the
   node-slot end k = 1 of the 256 x 4 class (P = 2560).
B  line, one node per rank and nearly so: W = 2, 3, 16 at P = W, W + 1, 2 W - 1.  A one-node slab of a
   middle rank has both neighbours in halos; ranks 0 and W - 1 hold the line's end nodes.
C  line, slabs of several tiles: W = 3 at P = 6141, 6144, 6147 (cuts 2047 / 4094, 2048 / 4096, 2049 /
   4098) and W = 4 at P = 4096 (every slab one tile).
D  line, many slabs in one tile: W = 16 at P = 1024 (each slab one wave) and P = 1040 (65-node slabs).
E  3D, one-plane slabs: g = W for W = 2, 3, 5, 8, 16, and g = 16 at W = 8 (two planes).  Both x
   neighbours of a one-plane slab come from halo planes, which travel uncompacted (g^2 < HALO_CHUNK).
   At g = 8 a plane is one wave, at g = 16 one 256-thread slot.

Kernels per shape: push-sum on the product build (the name and size class the plan chose asserted from
kernel_stats: the wide class at all of these sizes), push-sum on the experiments build forced to the
256 x 4 class (GP_KERNEL=tile GP_WIDE=0) and to the wide one (GP_WIDE=1), gossip on k_gossip_tile
(GP_KERNEL=tile); GP_CHECK_CLOSE=1 on the experiments build.  3D with GP_NO_FULLTILE=1 where a tile lies
wholly inside a slab -- at none of the shapes of E, whose slabs are at most 512 nodes, so that case
skips everywhere, with the reason computed.

Every case first shows on the CPU, before its simulation is created and reading nothing from the
library under test, that it is where it claims to be: the cut ids and their position relative to 1024,
256 and 64 and the tiles wholly inside each slab from tests/multirank_emu.py (slab_bounds, tiles_for;
tests/test_plan.py compares both with gp_plan.hpp at these shapes), and from the oracle's own state and
the senders' Philox draws (Geometry.draw_dir) that within the executed rounds, for every cut b, node
b - 1 -- active, push-sum: with s != 0 -- sent up to b in some round and b sent down to b - 1 in some
round (3D: some node of the plane below the cut sent up and some node of the plane above it down), and
that the cut nodes (3D: every node of both cut planes) are active at the last checkpoint.  For gossip
"active" at the last checkpoint means reached, c >= 1: a gossip node's active flag ends when it has
heard the rumour 11 times, so the nodes at fifteen cuts are never all flagged at once; its senders are
the flagged nodes.  The seeds and round counts below were searched on the CPU with the oracle so that
all of this holds (the line activates at about half a node per round: the seed node must lie near the
cuts); tests/test_plan.py repeats the demonstrations without a GPU.  The oracle is stepped once per
(shape, algorithm, seed) and shared by the kernel variants.
"""
import functools

import numpy as np
import pytest

from tests.multirank_emu import HALO_CHUNK, S_GOSSIP, S_PUSHSUM, XTILE, Geometry, slab_bounds, tiles_for
from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim

pytestmark = pytest.mark.gpu

CHK = 64          # rounds per checkpoint
CHK_LONG = 256    # ... of the cases that may run 4096 rounds
CAP, CAP_LONG = 1024, 4096
UP, DOWN = 1, 0   # the directions j + 1 / x + 1 and j - 1 / x - 1 (Geometry.nbr)

# (topology, size, W) -> {algorithm: (seed, rounds)}; size: P for the line, g for 3D.  Found by the
# search the module docstring describes.  Lines of more than 64 nodes: of the six seeds of 1..4000 whose
# seed node lies nearest the middle of the cuts, the one whose demonstration holds after the fewest whole
# checkpoints; the short lines and 3D: the same among the seeds 1..40 (a run that ends earlier ends
# there: the short lines converge within tens of rounds).
SEEDS = {
    ('line', 2046, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2048, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2050, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2174, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2176, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2178, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2560, 2): {'push-sum': (271, 64), 'gossip': (271, 64)},
    ('line', 2, 2): {'push-sum': (1, 5), 'gossip': (1, 6)},
    ('line', 3, 2): {'push-sum': (20, 5), 'gossip': (30, 8)},
    ('line', 3, 3): {'push-sum': (5, 6), 'gossip': (34, 8)},
    ('line', 4, 3): {'push-sum': (9, 10), 'gossip': (1, 11)},
    ('line', 5, 3): {'push-sum': (31, 27), 'gossip': (1, 14)},
    ('line', 16, 16): {'push-sum': (1, 64), 'gossip': (22, 30)},
    ('line', 17, 16): {'push-sum': (1, 64), 'gossip': (16, 37)},
    ('line', 31, 16): {'push-sum': (1, 64), 'gossip': (5, 60)},
    ('line', 6141, 3): {'push-sum': (3244, 2048), 'gossip': (271, 256)},
    ('line', 6144, 3): {'push-sum': (3244, 2048), 'gossip': (271, 256)},
    ('line', 6147, 3): {'push-sum': (3244, 2048), 'gossip': (271, 256)},
    ('line', 4096, 4): {'push-sum': (3940, 2048), 'gossip': (271, 256)},
    ('line', 1024, 16): {'push-sum': (1198, 896), 'gossip': (271, 128)},
    ('line', 1040, 16): {'push-sum': (919, 896), 'gossip': (271, 128)},
    ('3D', 2, 2): {'push-sum': (1, 64), 'gossip': (34, 13)},
    ('3D', 3, 3): {'push-sum': (1, 64), 'gossip': (36, 49)},
    ('3D', 5, 5): {'push-sum': (1, 64), 'gossip': (1, 64)},
    ('3D', 8, 8): {'push-sum': (1, 64), 'gossip': (1, 64)},
    ('3D', 16, 16): {'push-sum': (1, 64), 'gossip': (1, 64)},
    ('3D', 16, 8): {'push-sum': (1, 64), 'gossip': (1, 64)},
}

LINE_A = [2046, 2048, 2050, 2174, 2176, 2178, 2560]
LINE_B = [(W, P) for W in (2, 3, 16) for P in sorted({W, W + 1, 2 * W - 1})]  # (W = 2: W + 1 = 2 W - 1)
LINE_C = [(3, 6141), (3, 6144), (3, 6147), (4, 4096)]
LINE_D = [(16, 1024), (16, 1040)]
GRID_E = [(2, 2), (3, 3), (5, 5), (8, 8), (16, 16), (16, 8)]  # (g, W)
LINE_SHAPES = [(2, P) for P in LINE_A] + LINE_B + LINE_C + LINE_D  # (W, P)
LONG = set(LINE_C)

VARIANTS = ["product", "tile4", "tile1", "gossip"]
ENV = {"product": None,
       "tile4": {"GP_KERNEL": "tile", "GP_WIDE": "0", "GP_CHECK_CLOSE": "1"},
       "tile1": {"GP_KERNEL": "tile", "GP_WIDE": "1", "GP_CHECK_CLOSE": "1"},
       "gossip": {"GP_KERNEL": "tile", "GP_CHECK_CLOSE": "1"}}


def kernel_name(topo, variant):
    """What kernel_stats must report.  Product: plan_wide (gp_kernel_plan.hpp) gives line / 3D push-sum
    the wide class while a slab has at most two tiles per resident block, so at every size here."""
    t = "LINE" if topo == "line" else "GRID3D"
    if variant == "gossip":
        return "k_gossip_tile<%s>" % t
    return ("k_ps_tile<%s>" if variant == "tile4" else "wide::k_ps_tile<%s>") % t


# ---------------------------------------------------------------- the shape, from the plan's restatements
class Shape:
    def __init__(self, topo, size, W):
        self.topo, self.size, self.W = topo, size, W
        self.g = 0 if topo == "line" else size
        self.P = size if topo == "line" else size ** 3
        self.n = self.P - 1 if topo == "line" else self.P  # num_nodes (the line has P = n + 1)
        self.bounds, self.halo = slab_bounds(self.P, self.g, topo, W)
        assert self.bounds[0] == 0 and self.bounds[-1] == self.P and self.halo == (1 if topo == "line" else self.g ** 2)
        self.cuts = self.bounds[1:-1]
        self.sizes = [hi - lo for lo, hi in zip(self.bounds, self.bounds[1:])]
        assert min(self.sizes) >= self.halo
        self.tiles = [tiles_for(lo, hi - lo) for lo, hi in zip(self.bounds, self.bounds[1:])]
        # global tiles wholly inside each slab: the FULL body's (j0 == T and j1 == T + TILE)
        self.inside = [[t for t in range(lo // XTILE, -(-hi // XTILE)) if lo <= t * XTILE and (t + 1) * XTILE <= hi]
                       for lo, hi in zip(self.bounds, self.bounds[1:])]

    def below(self, b):
        """The senders up across cut b: node b - 1 (3D: the plane below)."""
        return np.arange(b - self.halo, b)

    def above(self, b):
        return np.arange(b, b + self.halo)


@functools.lru_cache(maxsize=None)
def shape(topo, size, W):
    return Shape(topo, size, W)


# ---------------------------------------------------------------- the oracle's run, once per (shape, algorithm)
class Trace:
    """R executed rounds of the oracle: alerts per round, the state after every chk rounds and after R,
    and per cut b the first round in which a node below it sent up (up[b]) and one above it down
    (down[b]) -- senders of round r: the nodes the oracle's state shows active at its start, push-sum
    with s != 0; their direction: Geometry.draw_dir."""


@functools.lru_cache(maxsize=None)
def trace(topo, size, W, alg, seed, rounds, chk):
    sh = shape(topo, size, W)
    t = Trace()
    t.seed, t.P = seed, sh.P
    orc = Oracle(sh.n, topo, alg, seed)
    assert orc.P == sh.P
    geo = Geometry(sh.P, sh.g, topo, seed)
    stream = S_PUSHSUM if alg == "push-sum" else S_GOSSIP
    watch = np.unique(np.concatenate([np.concatenate([sh.below(b), sh.above(b)]) for b in sh.cuts]))
    t.up, t.down = {b: None for b in sh.cuts}, {b: None for b in sh.cuts}
    t.alerts, t.states = [], {}
    r = 0
    while r < rounds and orc.alerts_total < orc.T:
        if any(t.up[b] is None or t.down[b] is None for b in sh.cuts):
            st = orc.state()
            ok = (st["flags"][watch] & 1) != 0
            if alg == "push-sum":
                ok &= st["s"][watch] != 0.0
            ids = watch[ok]
            if len(ids):
                d = geo.draw_dir(ids, stream, r)
                for b in sh.cuts:
                    if t.up[b] is None and np.any(d[(ids >= b - sh.halo) & (ids < b)] == UP):
                        t.up[b] = r
                    if t.down[b] is None and np.any(d[(ids >= b) & (ids < b + sh.halo)] == DOWN):
                        t.down[b] = r
        got = orc.step(1)
        assert len(got) == 1
        t.alerts += got
        r += 1
        if r % chk == 0:
            t.states[r] = orc.state()
    t.R = r
    assert orc.rounds == r
    if r not in t.states:
        t.states[r] = orc.state()
    for st in t.states.values():
        for v in st.values():
            v.setflags(write=False)
    t.alerts_total, t.finished = orc.alerts_total, orc.alerts_total >= orc.T
    orc.close()
    return t


def rounds_cap(topo, size, W):
    return (CAP_LONG, CHK_LONG) if (topo == "line" and (W, size) in LONG) else (CAP, CHK)


def demonstrate(topo, size, W, alg):
    """The CPU demonstration of one case (module docstring); returns its trace."""
    sh = shape(topo, size, W)
    seed, rounds = SEEDS[(topo, size, W)][alg]
    cap, chk = rounds_cap(topo, size, W)
    assert 0 < rounds <= cap
    t = trace(topo, size, W, alg, seed, rounds, chk)
    assert t.R == rounds or t.finished
    for b in sh.cuts:
        assert t.up[b] is not None and t.up[b] < t.R, f"no send up across cut {b} in {t.R} rounds"
        assert t.down[b] is not None and t.down[b] < t.R, f"no send down across cut {b} in {t.R} rounds"
    last = t.states[t.R]
    for b in sh.cuts:
        ids = np.concatenate([sh.below(b), sh.above(b)])
        if alg == "push-sum":
            assert np.all(last["flags"][ids] & 1), f"cut {b}: not active at the last checkpoint"
        else:
            assert np.all(last["c"][ids] >= 1), f"cut {b}: not reached at the last checkpoint"
    return t


def same_bits(alg, got, want):
    if alg == "gossip":
        np.testing.assert_array_equal(got["c"], want["c"])
    else:
        np.testing.assert_array_equal(got["s"].view(np.uint64), want["s"].view(np.uint64))
        np.testing.assert_array_equal(got["w"].view(np.uint64), want["w"].view(np.uint64))
    np.testing.assert_array_equal(got["flags"], want["flags"])


def run_exact(topo, size, W, variant, monkeypatch, extra_env=None):
    """The demonstration, then the library on W virtual ranks against the oracle's trace."""
    sh = shape(topo, size, W)
    alg = "gossip" if variant == "gossip" else "push-sum"
    t = demonstrate(topo, size, W, alg)
    env = dict(ENV[variant] or {}, **(extra_env or {}))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sim = Sim(sh.n, topo, alg, seed=t.seed, virtual_ranks=W, experimental=bool(env))
    try:
        assert sim.info().num_gpus == W and sim.population == sh.P
        assert sim.kernel_stats()[2] == kernel_name(topo, variant)
        done = 0
        for r in sorted(t.states):
            assert sim.step(r - done) == t.alerts[done:r], f"alerts differ in rounds {done}..{r}"
            done = r
            try:
                same_bits(alg, sim.state(), t.states[r])
            except AssertionError as e:
                raise AssertionError(f"state differs after round {r}: {e}") from None
        assert sim.rounds == t.R and sim.alerts_total == t.alerts_total
    finally:
        sim.close()


# ---------------------------------------------------------------- A: the cut against tile, wave and slot
# P: (cut, cut % 1024, cut % 256, cut % 64, tiles per slab, tiles wholly inside each slab)
LINE_A_CLAIMS = {
    2046: (1023, 1023, 255, 63, [1, 2], [[], []]),      # one id short of the tile end: the cut tile is rank 1's first
    2048: (1024, 0, 0, 0, [1, 1], [[0], [1]]),          # on it: each slab exactly one tile, FULL body
    2050: (1025, 1, 1, 1, [2, 2], [[0], []]),           # one past: rank 0 has a second tile of one node
    2174: (1087, 63, 63, 63, [2, 2], [[0], []]),        # the last lane of tile 1's wave 0
    2176: (1088, 64, 64, 0, [2, 2], [[0], []]),         # on the wave end inside tile 1
    2178: (1089, 65, 65, 1, [2, 2], [[0], []]),         # lane 1 of wave 1
    2560: (1280, 256, 0, 0, [2, 2], [[0], []]),         # node slot k = 1 of the 256 x 4 class, thread 0
}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("P", LINE_A)
def test_line_cut_at_tile_wave_and_slot(P, variant, monkeypatch):
    sh = shape("line", P, 2)
    cut, m1024, m256, m64, tiles, inside = LINE_A_CLAIMS[P]
    assert sh.cuts == [cut] and (cut % XTILE, cut % 256, cut % 64) == (m1024, m256, m64)
    assert sh.tiles == tiles and sh.inside == inside
    if P == 2050:
        assert sh.bounds[1] - XTILE == 1
    run_exact("line", P, 2, variant, monkeypatch)


# ---------------------------------------------------------------- B: one node per rank and nearly so
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,P", LINE_B, ids=lambda v: str(v))
def test_line_one_node_per_rank(W, P, variant, monkeypatch):
    sh = shape("line", P, W)
    assert set(sh.sizes) <= {1, 2} and sh.sizes.count(2) == P - W and len(sh.cuts) == W - 1
    assert sh.tiles == [1] * W and sh.inside == [[]] * W
    if P == W:  # every slab one node: a middle rank's node has both neighbours in halos
        assert sh.sizes == [1] * W and sh.cuts == list(range(1, W))
    assert sh.bounds[1] >= 1 and sh.bounds[-2] <= P - 1  # the end nodes 0 and P - 1 on ranks 0 and W - 1
    run_exact("line", P, W, variant, monkeypatch)


# ---------------------------------------------------------------- C: slabs of several tiles
LINE_C_CLAIMS = {
    (3, 6141): ([2047, 4094], [2, 3, 3], [[0], [2], [4]]),
    (3, 6144): ([2048, 4096], [2, 2, 2], [[0, 1], [2, 3], [4, 5]]),
    (3, 6147): ([2049, 4098], [3, 3, 3], [[0, 1], [3], [5]]),
    (4, 4096): ([1024, 2048, 3072], [1, 1, 1, 1], [[0], [1], [2], [3]]),
}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,P", LINE_C, ids=lambda v: str(v))
def test_line_slabs_of_several_tiles(W, P, variant, monkeypatch):
    sh = shape("line", P, W)
    cuts, tiles, inside = LINE_C_CLAIMS[(W, P)]
    assert sh.cuts == cuts and sh.tiles == tiles and sh.inside == inside
    run_exact("line", P, W, variant, monkeypatch)


# ---------------------------------------------------------------- D: many slabs in one tile
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,P", LINE_D, ids=lambda v: str(v))
def test_line_many_slabs_in_one_tile(W, P, variant, monkeypatch):
    sh = shape("line", P, W)
    if P == 1024:  # each slab one wave of tile 0: every cut a wave end
        assert sh.sizes == [64] * W and all(b % 64 == 0 for b in sh.cuts) and sh.tiles == [1] * W
    else:  # 65-node slabs: cut w is lane w of wave w; the last slab crosses into tile 1
        assert sh.sizes == [65] * W and [b % 64 for b in sh.cuts] == list(range(1, W)) and sh.tiles == [1] * (W - 1) + [2]
    assert sh.inside == [[]] * W
    run_exact("line", P, W, variant, monkeypatch)


# ---------------------------------------------------------------- E: 3D, one-plane slabs
def check_planes(g, W):
    sh = shape("3D", g, W)
    planes = g // W
    assert planes in (1, 2) and sh.sizes == [planes * g * g] * W and g * g < HALO_CHUNK
    if g == 8:
        assert g * g == 64  # a plane is one wave
    if g == 16:
        assert g * g == 256  # ... one 256-thread slot
    return sh


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("g,W", GRID_E, ids=lambda v: str(v))
def test_grid_one_plane_slabs(g, W, variant, monkeypatch):
    check_planes(g, W)
    run_exact("3D", g, W, variant, monkeypatch)


@pytest.mark.parametrize("variant", ["tile4", "tile1"])
@pytest.mark.parametrize("g,W", GRID_E, ids=lambda v: str(v))
def test_grid_one_plane_slabs_general_body(g, W, variant, monkeypatch):
    """GP_NO_FULLTILE=1 where the default would run a full-tile body."""
    sh = check_planes(g, W)
    if not any(sh.inside):
        assert max(sh.sizes) < XTILE
        pytest.skip("3D has no full tile at this shape")
    run_exact("3D", g, W, variant, monkeypatch, {"GP_NO_FULLTILE": "1"})
