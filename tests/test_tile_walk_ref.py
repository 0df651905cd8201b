"""The host model of the tile walks (tests/tile_walk_ref.py) at every slab shape of
tests/test_gpu_tile_sequence.py: every walk on every grid visits each tile of the slab exactly once,
and the walk-3 queues are build_walk_list's (gp_plan.hpp, through tests/helpers/plan_check.cpp, as
tests/test_plan.py takes it).  CPU-only: compiles the small host program of test_plan.py.
"""
import pytest

from tests import multirank_emu as emu
from tests import tile_walk_ref as tw
from tests.test_plan import plan  # noqa: F401  (the module-scoped fixture)

# (topology, num_nodes, ranks) of the GPU module; 3D and Imp3D share their slabs
SHAPES = [("Imp3D", g ** 3, 1) for g in (9, 16, 20, 32, 33, 40)] + [("Imp3D", 32 ** 3, 2), ("Imp3D", 33 ** 3, 2),
                                                                   ("Imp3D", 33 ** 3, 3), ("line", 3000, 1)]
GRIDS = (1, 2, 3, 5, 8, 16)
WX = (3, 8, 16)


def slab_list(topo, n, ranks):
    P, _, g = emu.resolve(n, topo)
    b = emu.slab_bounds(P, g, topo, ranks)[0]
    return g * g, [(b[r], b[r + 1] - b[r]) for r in range(ranks)]


@pytest.mark.parametrize("topo,n,ranks", SHAPES)
def test_every_tile_exactly_once(topo, n, ranks):
    g2, sl = slab_list(topo, n, ranks)
    for lo, nloc in sl:
        nt = tw.tiles_for(lo, nloc)
        assert nt == emu.tiles_for(lo, nloc)
        for grid in GRIDS:
            for walk in (0, 1, 2, 3):
                for wx in WX:
                    mode, seq = tw.tile_walk(lo, nloc, g2, grid, walk, wx)
                    # walks 0, 2 and 3 need a multiple of 8 blocks, 2 and 3 a lattice: else one global sweep
                    by8 = grid % 8 == 0
                    assert mode == (walk if by8 and (g2 or walk == 0) else 1)
                    assert len(seq) == (8 if mode == 3 else grid)
                    assert sorted(t for q in seq for t in tw.tiles_of(q)) == list(range(nt)), (lo, grid, walk, wx)
                    if mode != 2:
                        assert all(t is not tw.EMPTY for q in seq for t in q)
        # the ids of the tiles partition the slab
        rng = [tw.tile_range(lo, nloc, t) for t in range(nt)]
        assert rng[0][0] == lo and rng[-1][1] == lo + nloc and all(a[1] == b[0] for a, b in zip(rng, rng[1:]))
        assert all(0 < b - a <= tw.TILE for a, b in rng)


def test_small_grids_run_one_global_sweep():
    """grid < 8 or no multiple of 8: tile t -> block t % grid whatever walk was asked for."""
    for walk in (0, 1, 2, 3):
        for grid in (1, 3, 5, 12):
            assert tw.tile_walk(0, 8000, 400, grid, walk, 3) == (1, [list(range(b, 8, grid)) for b in range(grid)])


@pytest.mark.parametrize("topo,n,ranks", [s for s in SHAPES if s[0] != "line"])
def test_walk3_queues_are_build_walk_list(plan, topo, n, ranks):  # noqa: F811
    g2, sl = slab_list(topo, n, ranks)
    for lo, nloc in sl:
        for wx in WX:
            (ok, woff, tiles), = plan([("walk", lo, nloc, g2, wx, 1)])
            assert ok == [1] and len(woff) == 9
            mode, queues = tw.tile_walk(lo, nloc, g2, 8, 3, wx)
            assert mode == 3 and queues == [tiles[woff[c]:woff[c + 1]] for c in range(8)], (lo, wx)
            # walk 2 on 8 blocks: block c runs XCD c's items, the queue plus the empty ones
            mode2, seq = tw.tile_walk(lo, nloc, g2, 8, 2, wx)
            assert mode2 == 2 and [tw.tiles_of(q) for q in seq] == queues
            # ... and on 16 blocks, blocks c and c + 8 take alternate items
            _, seq16 = tw.tile_walk(lo, nloc, g2, 16, 2, wx)
            assert all(seq16[c] == seq[c][0::2] and seq16[c + 8] == seq[c][1::2] for c in range(8))
