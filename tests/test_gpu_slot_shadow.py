"""GPU: the push-sum tile kernel's slot ordering (gp_ps_tile.hip) against the CPU
oracle, bit-exact on s, w, flags and per-round alerts.

Between a node slot's load issue and its wait the kernel draws the node's next-round direction --
unconditionally, as a candidate parked in `pend`, which stands only if the node is active after the
fold -- and decides the next slot (in-edge prefix, node byte, mask, lattice senders, coordinate
step), carrying two registers to that slot's issue.  What can go wrong is therefore: an inactive
node keeps its candidate instead of DIR_NONE; a node that turns active in round r does not send in
round r + 1 along the candidate; a converged node stops drawing; the general body lets an invalid
lane's candidate reach the byte, the store or the ballot; the carried words of a tile's last slot
leak into the next tile's first; the slot decided ahead reads another `wide` / `staged` state than
its issue.  Any of these changes who sends to whom in the next round and so the oracle's state.

Every case runs on the product build with the kernel the product chooses, and on the experiments
build with GP_SLOT_SHADOW=0 (the earlier ordering: batch draw at the tile's end, every slot decided
at its start) and =1, the kernel forced with GP_KERNEL=tile.  Overrides exist in the experiments build
only, so the cases that need one (GP_GRID, GP_NO_FULLTILE, GP_STAGE_CAP, the 256 x 4 kernel for 3D
and line) have no product variant.

Every case first shows on the CPU, from the oracle alone, that it reaches the path it names: a round
with an inactive node whose candidate (its Philox draw for the next round, recomputed here) is a
direction; a round with a newly active node; converged nodes in a run that goes on; the block's tile
sequence from tests/tile_walk_ref.py.  Seed 2 throughout, as in tests/test_gpu_tile_sequence.py.
"""
import functools

import numpy as np
import pytest

from tests import oracle_ctypes
from tests import test_gpu_tile_sequence as tsq
from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim

pytestmark = pytest.mark.gpu

SEED = tsq.SEED
S_PUSHSUM, DIR_NONE = 3, 7       # gp_device.hpp
B_ACTIVE, B_CONV = 1, 2          # or_read_state's flag bits
BUILDS = ["product", "shadow0", "shadow1"]
EXP_BUILDS = BUILDS[1:]


# ---------------------------------------------------------------- the CPU side
def candidate(i, rnd, deg):
    """The slot node i's draw for round `rnd` picks among its deg neighbour slots (0-based; deg - 1
    is the Imp3D random edge): floor(((y << 32) | x) * deg / 2^64), SRS v1's uniform."""
    x, y, _, _ = oracle_ctypes.philox((i, rnd, S_PUSHSUM, 0), (SEED & 0xFFFFFFFF, SEED >> 32))
    return (((y << 32) | x) * deg) >> 64


@functools.lru_cache(maxsize=None)
def activation(n, topo, cap=20000):
    """Round by round until every node is active: (rounds, a round with inactive nodes next to active
    ones, an inactive node of that round, a round in which a node turned active)."""
    orc = Oracle(n, topo, "push-sum", SEED)
    P = orc.P
    mixed = newly = node = None
    before = orc.state()["flags"] & B_ACTIVE
    while orc.active_count() < P:
        assert orc.rounds < cap, "activation did not complete"
        orc.step(1)
        now = orc.state()["flags"] & B_ACTIVE
        if newly is None and np.any(now & ~before & 1):
            newly = orc.rounds - 1
        if mixed is None and 0 < np.count_nonzero(now) < P:
            mixed, node = orc.rounds, int(np.flatnonzero(now == 0)[0])
        before = now
    deg = len(orc.neighbors(node))
    rounds = orc.rounds
    orc.close()
    return rounds, mixed, node, deg, newly


def assert_reaches_inactive_and_newly_active(n, topo):
    """Some round holds an inactive node with a candidate that is a direction (the kernel must still
    publish DIR_NONE for it), and some round holds a newly active node (which must send next round)."""
    rounds, mixed, node, deg, newly = activation(n, topo)
    assert mixed is not None and newly is not None and newly < rounds
    assert deg >= 1 and 0 <= candidate(node, mixed + 1, deg) < deg < DIR_NONE + 1
    return rounds


def assert_converged_nodes_keep_running(ref):
    """Some checkpoint before the last holds converged nodes: they go on drawing and sending (D6)."""
    assert any(np.any(st["flags"] & B_CONV) for _, _, st in ref.chunks[:-1])
    assert ref.alerts_total >= ref.T


# ---------------------------------------------------------------- the GPU side
def run(monkeypatch, build, n, topo, ref, kernel=None, ranks=1, wide="0", **extra):
    exp = build != "product"
    if exp:
        monkeypatch.setenv("GP_KERNEL", "tile")
        monkeypatch.setenv("GP_WIDE", wide)
        monkeypatch.setenv("GP_SLOT_SHADOW", build[-1])
        for k, v in extra.items():
            monkeypatch.setenv(k, str(v))
    else:
        assert not extra, "overrides exist in the experiments build only"
    try:
        sim = Sim(n, topo, "push-sum", seed=SEED, virtual_ranks=ranks, experimental=exp)
    except ImportError:
        if exp:
            pytest.skip("the experiments library is not built")
        raise
    assert sim.info().num_gpus == ranks
    name = sim.kernel_stats()[2]
    if kernel and (exp or topo == "Imp3D"):  # Imp3D push-sum: the tile kernel is also the product's choice
        assert name == f"{kernel}@{extra['GP_GRID']}" if "GP_GRID" in extra else name.split("@")[0] == kernel, name
    tsq.check(sim, ref)
    sim.close()


IMP_KERNEL = "k_ps_tile<IMP3D>"


@pytest.mark.parametrize("build", BUILDS)
def test_imp3d_full_tiles_seed_to_convergence(build, monkeypatch):
    """g = 16: four full tiles, from the seed node through activation to convergence."""
    n = tsq.N16
    (s,) = tsq.slabs("Imp3D", n)
    assert s.nt == 4 and not any(s.partial) and max(s.edges) <= tsq.SLOTS and max(s.maxdeg) < 15  # FULL body only
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    ref = tsq.reference(n, "Imp3D", "push-sum", None)
    assert_converged_nodes_keep_running(ref)
    run(monkeypatch, build, n, "Imp3D", ref, IMP_KERNEL)


@pytest.mark.parametrize("build", BUILDS)
def test_imp3d_partial_tile_and_partial_wave(build, monkeypatch):
    """g = 13: 2197 nodes -- two full tiles and one of 149 nodes, whose third wave holds 21 valid
    lanes and whose slots 1..3 hold none: the general body parks candidates for invalid lanes."""
    n = 13 ** 3
    (s,) = tsq.slabs("Imp3D", n)
    assert s.nt == 3 and s.partial == (False, False, True)
    last = s.lo + s.nloc - 2 * 1024
    assert last == 149 and last % 64 == 21 and last < 256
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    ref = tsq.reference(n, "Imp3D", "push-sum", None)
    assert_converged_nodes_keep_running(ref)
    run(monkeypatch, build, n, "Imp3D", ref, IMP_KERNEL)


@pytest.mark.parametrize("build", EXP_BUILDS)
def test_imp3d_one_block_full_then_general_tile(build, monkeypatch):
    """g = 11 on one block (GP_GRID=1): the full tile 0, then the partial tile 1 through the general
    body -- what slot 3 of tile 0 decided ahead or carried must not reach tile 1's slot 0."""
    n = 11 ** 3
    (s, mode, seq), = tsq.walks("Imp3D", n, 1)
    assert [tsq.tw.tiles_of(q) for q in seq] == [[0, 1]] and s.partial == (False, True)
    assert s.edges[0] <= tsq.SLOTS and s.maxdeg[0] < 15  # tile 0 runs the FULL body
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    ref = tsq.reference(n, "Imp3D", "push-sum", None)
    assert_converged_nodes_keep_running(ref)
    run(monkeypatch, build, n, "Imp3D", ref, IMP_KERNEL, GP_GRID=1)


@pytest.mark.parametrize("build", EXP_BUILDS)
def test_imp3d_one_block_bodies_alternate(build, monkeypatch):
    """g = 20 on one block with GP_STAGE_CAP=1031: tiles F F F G G F G G (F: FULL body, G: general --
    unstaged, the last one partial), so both bodies follow each other both ways within one block."""
    (seq,) = tsq.a_seq(1, cap=1031)
    got = "".join("F" if staged and not wide and not partial else "G" for _, staged, wide, partial in seq)
    assert got == "FFFGGFGG"
    ref = tsq.reference(*tsq.IMP, 96)
    run(monkeypatch, build, tsq.N20, "Imp3D", ref, IMP_KERNEL, GP_GRID=1, GP_STAGE_CAP=1031)


@pytest.mark.parametrize("build", BUILDS)
def test_3d_on_the_256x4_kernel(build, monkeypatch):
    """3D at g = 16 (no in-edge pass, no random slot: degree = popcount of the mask, 3..6)."""
    n = tsq.N16
    rounds = assert_reaches_inactive_and_newly_active(n, "3D")
    ref = tsq.reference(n, "3D", "push-sum", rounds + 64)
    run(monkeypatch, build, n, "3D", ref, "k_ps_tile<GRID3D>")


@pytest.mark.parametrize("build", BUILDS)
def test_line_on_the_256x4_kernel(build, monkeypatch):
    """Line at n = 3000 (P = 3001: three tiles, the last of 953 nodes; no gathers at all, NDG = 0; the
    two end nodes have degree 1), through activation and 64 rounds on."""
    (s,) = tsq.slabs("line", 3000)
    assert s.nt == 3 and s.partial == (False, False, True)
    rounds = assert_reaches_inactive_and_newly_active(3000, "line")
    assert rounds == tsq.line_all_active_round(3000)
    ref = tsq.reference(3000, "line", "push-sum", rounds + 64, 256)
    run(monkeypatch, build, 3000, "line", ref, "k_ps_tile<LINE>")


@pytest.mark.parametrize("build", BUILDS)
def test_imp3d_two_virtual_ranks(build, monkeypatch):
    """The REMOTE instantiation: g = 16 as two slabs of two full tiles."""
    n = tsq.N16
    assert [(s.nt, any(s.partial)) for s in tsq.slabs("Imp3D", n, 2)] == [(2, False)] * 2
    assert max(e for s in tsq.slabs("Imp3D", n, 2) for e in s.edges) <= tsq.SLOTS_REMOTE
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    ref = tsq.reference(n, "Imp3D", "push-sum", None)
    run(monkeypatch, build, n, "Imp3D", ref, IMP_KERNEL, ranks=2)


@pytest.mark.parametrize("build", EXP_BUILDS)
def test_imp3d_every_tile_through_the_general_body(build, monkeypatch):
    """GP_NO_FULLTILE=1 at g = 16: staged, not wide, whole tiles in the general body."""
    n = tsq.N16
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    run(monkeypatch, build, n, "Imp3D", tsq.reference(n, "Imp3D", "push-sum", None), IMP_KERNEL, GP_NO_FULLTILE=1)


@pytest.mark.parametrize("build", EXP_BUILDS)
def test_imp3d_unstaged_and_wide_tiles(build, monkeypatch):
    """g = 16 with GP_STAGE_CAP=1024 (tiles 1 and 3 unstaged: in-edges one by one) and GP_IND4_WIDE=6
    (tiles 0 and 1 wide: in_off per node): the slot decided ahead and its issue see one `staged` /
    `wide` state, tile 2 alone runs the FULL body."""
    n = tsq.N16
    (s,) = tsq.slabs("Imp3D", n)
    assert [e <= 1024 for e in s.edges] == [True, False, True, False]
    assert [d >= 6 for d in s.maxdeg] == [True, True, False, False]
    assert_reaches_inactive_and_newly_active(n, "Imp3D")
    run(monkeypatch, build, n, "Imp3D", tsq.reference(n, "Imp3D", "push-sum", None), IMP_KERNEL,
        GP_STAGE_CAP=1024, GP_IND4_WIDE=6)
