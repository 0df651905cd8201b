"""Host model of the tile walks (TileWalk, gossipprotocol_amd/csrc/gp_tile.hpp), in plain Python.

The tiled round kernels are persistent: a block runs several tiles per launch, in an order its walk
decides from (lo, nloc, g2, grid, walk, wx).  The GPU tests of tests/test_gpu_tile_sequence.py use
this restatement to prove, before anything runs, which tiles a block runs one after the other --
that a prefetched range is consumed, that a staged tile follows an unstaged one, that an empty item
lies between two tiles.  tests/test_tile_walk_ref.py checks the model itself (every tile exactly
once; the walk-3 queues equal build_walk_list of gp_plan.hpp).

    walk 0   XCD-contiguous eighths of the tile range (blocks b, b + 8, .. share XCD b % 8)
    walk 1   one global sweep: tile t -> block t % grid
    walk 2   x-windows: XCD c owns an eighth of the slab's planes, cut into windows of ~wx planes;
             item u of a window -> plane x_w + u % nx_w, k-th tile starting in that plane.  A plane
             with fewer than kp tiles leaves EMPTY items
    walk 3   walk 2's items without the empty ones, one queue per XCD, claimed from a counter;
             a block whose queue is exhausted takes from the queues (b + 1) % 8, (b + 2) % 8, ..
Walks 0, 2 and 3 need a grid that is a multiple of 8 (>= 8), walk 2 and 3 a lattice (g2 > 0); the
kernel otherwise runs walk 1.
"""
TILE = 1024
EMPTY = None  # an item of walk 2 that holds no tile


def tiles_for(lo, nloc):
    """Tiles covering ids [lo, lo + nloc): they sit on global multiples of TILE."""
    return (lo + nloc + TILE - 1) // TILE - lo // TILE


def tile_range(lo, nloc, rel):
    """Ids [j0, j1) of the slab's tile `rel` (relative to lo // TILE): the first and last may be partial."""
    T = (lo // TILE + rel) * TILE
    return max(lo, T), min(lo + nloc, T + TILE)


def effective_walk(g2, grid, walk):
    """The walk the kernel runs (TileWalk's constructor)."""
    by8 = grid >= 8 and grid % 8 == 0
    if walk == 3:  # (without a lattice the host has no tile list to give it)
        return 3 if by8 and g2 else 1
    if walk == 2 and g2 and by8:
        return 2
    if walk == 0 and by8:
        return 0
    return 1


def xcd_items(lo, nloc, g2, wx, c):
    """Walk 2's items of XCD c in item order: the tile (relative to lo // TILE) or EMPTY.  Item ->
    tile by TileWalk::tile's own arithmetic (window search from the item index)."""
    tb, tend = lo // TILE, (lo + nloc + TILE - 1) // TILE
    x0, nx = lo // g2, nloc // g2
    xa = x0 + nx * c // 8
    nxa = x0 + nx * (c + 1) // 8 - xa
    kp = (g2 + TILE - 1) // TILE + 1
    nwin = max(1, (nxa + wx - 1) // wx if wx else 1)

    def first(x):  # first global tile of plane x (the slab's first tile may start below lo)
        return tb if x <= x0 else min((x * g2 + TILE - 1) // TILE, tend)

    items = []
    for t in range(nxa * kp):
        v = min(t // kp * nwin // nxa, nwin - 1)
        xs = nxa * v // nwin
        while v > 0 and xs * kp > t:
            v -= 1
            xs = nxa * v // nwin
        while v + 1 < nwin and nxa * (v + 1) // nwin * kp <= t:
            v += 1
            xs = nxa * v // nwin
        xe = nxa * (v + 1) // nwin
        u, nxv = t - xs * kp, xe - xs
        x, k = xa + xs + u % nxv, u // nxv
        ti = first(x) + k
        items.append(EMPTY if ti >= first(x + 1) else ti - tb)
    return items


def tile_walk(lo, nloc, g2, grid, walk, wx):
    """(mode, seq).  mode: the walk the kernel runs on this grid.  mode 0, 1, 2: seq[b] is block b's
    items in order, EMPTY marking walk 2's empty ones.  mode 3: seq[c] is XCD c's queue (8 queues);
    block b claims from queue b % 8, then from the other queues in turn."""
    mode = effective_walk(g2, grid, walk)
    nt = tiles_for(lo, nloc)
    if mode == 3:
        return 3, [[t for t in xcd_items(lo, nloc, g2, wx, c) if t is not EMPTY] for c in range(8)]
    if mode == 2:
        per_xcd = [xcd_items(lo, nloc, g2, wx, c) for c in range(8)]
        return 2, [per_xcd[b % 8][b // 8::grid // 8] for b in range(grid)]
    if mode == 0:
        return 0, [list(range(nt * (b % 8) // 8 + b // 8, nt * (b % 8 + 1) // 8, grid // 8)) for b in range(grid)]
    return 1, [list(range(b, nt, grid)) for b in range(grid)]


def tiles_of(seq):
    """A sequence without its empty items."""
    return [t for t in seq if t is not EMPTY]
