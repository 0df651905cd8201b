"""GPU: the push-sum tile kernel's two per-tile bodies (gp_ps_tile.hip, ps_tiles) against the CPU
oracle, bit-exact.

A tile that lies wholly inside the slab and (Imp3D) is staged and not `wide` runs the FULL body
(no range tests, z +- 1 sender bytes by DPP); every other tile -- the slab's partial first / last
tile, tiles above the staging cap, tiles holding a node whose in-degree does not fit the nibble
array -- runs the general body.  The sizes below put tile and wave boundaries where the two
differ: all tiles full (n = 4096), one full and one partial tile in one launch (1331), a single
partial tile (1000), a last wave that is itself partial (9261), slabs of two virtual ranks ending
on and off tile boundaries, and full tiles mixed with unstaged / wide ones (GP_STAGE_CAP,
GP_IND4_WIDE).  The kernel is forced with GP_KERNEL=tile on the experiments build.

Seed 2 at n = 4096 (from the oracle's in-lists): the four tiles hold 999 / 1042 / 1006 / 1049
in-edges -- GP_STAGE_CAP=1000 leaves tile 0 staged (full) and three unstaged, 1024 leaves tiles 0
and 2 -- and their largest in-degrees are 7 / 6 / 5 / 5: GP_IND4_WIDE=6 makes tiles 0 and 1 wide
and leaves 2 and 3 full; at GP_IND4_WIDE=2 every tile is wide (no 1024-node tile is without a node
of in-degree 2), the FULL body never runs.
"""
import functools

import numpy as np
import pytest

from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim, assert_same_state, digest

pytestmark = pytest.mark.gpu

ROUNDS, CHK = 48, 8


@functools.lru_cache(maxsize=None)
def reference(n, topo, seed, rounds=ROUNDS, chk=CHK):
    """The oracle's run, computed once per case: [(alerts of the chunk, state after it)]."""
    orc = Oracle(n, topo, "push-sum", seed)
    out = []
    for _ in range(rounds // chk):
        a = orc.step(chk)
        st = orc.state()
        for v in st.values():
            v.setflags(write=False)
        out.append((a, st))
    orc.close()
    return out


def check(sim, n, topo, seed, name_has="tile"):
    assert name_has in sim.kernel_stats()[2], sim.kernel_stats()[2]
    for i, (oa, ost) in enumerate(reference(n, topo, seed)):
        ga = sim.step(CHK)
        assert ga == oa, f"alerts differ in rounds {i * CHK}..{(i + 1) * CHK}"
        assert_same_state("push-sum", sim.state(), ost)


def tile_env(monkeypatch, wide="0", **extra):
    monkeypatch.setenv("GP_KERNEL", "tile")
    monkeypatch.setenv("GP_WIDE", wide)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("n", [4096, 1331, 1000, 9261])
def test_imp3d_activation_into_steady(n, monkeypatch):
    """Rounds 0..48, through activation into every node active."""
    tile_env(monkeypatch)
    sim = Sim(n, "Imp3D", "push-sum", seed=2, experimental=True)
    check(sim, n, "Imp3D", 2)
    assert sim.info().active == sim.population  # the steady-state in-edge pass ran
    sim.close()


@pytest.mark.parametrize("n", [1331, 1000])
def test_imp3d_to_convergence(n, monkeypatch):
    tile_env(monkeypatch)
    sim, orc = Sim(n, "Imp3D", "push-sum", seed=3, experimental=True), Oracle(n, "Imp3D", "push-sum", 3)
    while orc.alerts_total < orc.T:
        assert orc.rounds < 20000
        ga, oa = sim.step(250), orc.step(250)
        assert ga == oa, f"alerts differ before round {orc.rounds}"
        assert_same_state("push-sum", sim.state(), orc.state())
    assert sim.rounds == orc.rounds and sim.alerts_total == orc.alerts_total >= sim.threshold
    sim.close()
    orc.close()


@pytest.mark.parametrize("var,val", [("GP_STAGE_CAP", "1000"), ("GP_STAGE_CAP", "1024"),
                                     ("GP_IND4_WIDE", "2"), ("GP_IND4_WIDE", "6")])
def test_imp3d_full_and_general_tiles_mixed(var, val, monkeypatch):
    """n = 4096, seed 2: some tiles unstaged / wide, the others full (module docstring)."""
    tile_env(monkeypatch, **{var: val})
    sim = Sim(4096, "Imp3D", "push-sum", seed=2, experimental=True)
    check(sim, 4096, "Imp3D", 2)
    sim.close()


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("n,topo", [(4096, "3D"), (1331, "3D"), (4096, "line"), (1500, "line")])
def test_lattice_topologies(n, topo, wide, monkeypatch):
    """The shared template's 3D and line instantiations, in both size classes."""
    tile_env(monkeypatch, wide=wide)
    sim = Sim(n, topo, "push-sum", seed=2, experimental=True)
    assert sim.kernel_stats()[2].startswith("wide::") == (wide == "1"), sim.kernel_stats()[2]
    check(sim, n, topo, 2)
    sim.close()


@pytest.mark.parametrize("n", [4096, 1331])
def test_imp3d_two_virtual_ranks(n, monkeypatch):
    """The REMOTE instantiation: slabs of 8 planes of 256 nodes (ends on tile boundaries) and of
    5 / 6 planes of 121 (off them)."""
    tile_env(monkeypatch)
    sim = Sim(n, "Imp3D", "push-sum", seed=2, virtual_ranks=2, experimental=True)
    assert sim.info().num_gpus == 2
    check(sim, n, "Imp3D", 2)
    sim.close()


def test_forcing_switch_gives_the_same_digests(monkeypatch):
    """GP_NO_FULLTILE=1 (every tile through the general body) and the default give the same state
    digests, both the oracle's."""
    tile_env(monkeypatch)
    a = Sim(4096, "Imp3D", "push-sum", seed=2, experimental=True)
    monkeypatch.setenv("GP_NO_FULLTILE", "1")
    b = Sim(4096, "Imp3D", "push-sum", seed=2, experimental=True)
    for oa, ost in reference(4096, "Imp3D", 2):
        assert a.step(CHK) == oa and b.step(CHK) == oa
        assert digest("push-sum", a.state()) == digest("push-sum", b.state()) == digest("push-sum", ost)
    a.close()
    b.close()
