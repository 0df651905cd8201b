"""GPU: every round kernel's Philox key with the seed's high word set, against the CPU oracle,
bit-exact (seed node, per-round alerts, and s / w / flags -- gossip: c / flags -- of every node at
every checkpoint; on Imp3D also gp_neighbors of ~50 nodes).

The key is (k0, k1) = (seed & 0xFFFFFFFF, seed >> 32), split once in alloc_slab (gp_setup.hip) and
copied by hand into every kernel's argument block.  Every other non-ensemble GPU test uses a seed
below 2^32, so k1 = 0 there: a kernel that received k1 = 0, or a key schedule that mishandled k1's
carries, would pass them all.  tests/test_oracle.py shows on the CPU that the oracle's run changes
with the high word alone (test_high_seed_word_changes_the_run), so no case here can pass with a
wrong k1 by coincidence.

Seeds: WIDE_SEEDS (tests/test_oracle.py) on the first path of each kernel family, W0 = 2^63 + 3 on
every path.  With 2^64 - 1 the seed node of the g = 20 Imp3D gossip run sends its round-0 rumour along
its random edge (asserted in test_col_seed_init_random_edge): k_col_seed_init must count that delivery.

Every run is the oracle's, computed once per (shape, seed) and shared (`reference`), with its
non-vacuity conditions asserted on the oracle's own state:
  push-sum  until every node is active and at least one node has alerted, at a checkpoint, within
            400 rounds -- the line within 20000: a line of 3001 nodes needs thousands of rounds
            until its last node has heard, and they cost milliseconds;
  gossip    the injector's round-0 pick (recomputed here from the S_INJECT draw) has been delivered
            -- sum(c) = 2 and c[pick] >= 1 after round 0 -- at least half the nodes have heard the
            rumour and at least one has alerted;
  Imp3D     in the first round of every chunk from round 8 on (before it a handful of nodes send),
            some active node's draw picks its random edge (slot deg - 1), recomputed from the
            oracle's state and the Philox draw.
Checkpoints: after rounds 1 (gossip), 8, 16, ... 64, then every 64 (line: 256).

Shapes: line n = 3000 (3 tiles), lattices g = 20 (8 tiles / 8 boxes / 5 y-blocks), full gossip
n = 257 (two 256-thread blocks), full push-sum n = 16384 (P = 16385: two work items of k_fb_send,
five fine tiles).

philox2_batch sites of gp_fullbin.hip and the cases that run them:
  :250 k_fb_send      test_full_pushsum[fused-*] (round 0), test_full_pushsum[three_pass-W0]
  :364 k_fb_split     all test_full_pushsum cases (k_fb_split<true> on 3 ranks)
  :496, :514 k_fbm_send   test_full_pushsum[ranks3-W0] (round 0's send pass)
  :645 k_fb_fold's send phase   test_full_pushsum[fused-*], [ranks3-W0] (k_fb_fold<FOLD_SEND_RANKS>)
  :655 k_fb_fold      all test_full_pushsum cases
"""
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import multirank_emu as emu
from tests import test_gpu_tile_sequence as tsq
from tests.oracle_ctypes import Oracle
from tests.summary_ref import ref_summary
from tests.test_gpu_parity import ROOT, Sim, assert_same_state
from tests.test_oracle import WIDE_SEEDS

pytestmark = pytest.mark.gpu

W0, TOP = 2**63 + 3, 2**64 - 1
assert W0 == WIDE_SEEDS[0]
ALL = [pytest.param(s, id=hex(s)) for s in WIDE_SEEDS]
LINE, G20, FULL_G, FULL_PS = 3000, 8000, 257, 16384
Ref = namedtuple("Ref", "chunks rounds alerts_total T seed_node nbrs")


# ---------------------------------------------------------------- the oracle's runs, once per case
def lattice_degree(i, g):
    x, y, z = i // (g * g), i // g % g, i % g
    return sum((v > 0).astype(np.int64) + (v < g - 1) for v in (x, y, z))


def random_edge_senders(seed, alg, g, rnd, st, seed_node):
    """Active nodes whose round-`rnd` draw picks the Imp3D random edge, the last of their deg slots."""
    if alg == "gossip":
        c = st["c"]
        act = ((c >= 1) | (np.arange(c.size) == seed_node)) & (c <= 10)
    else:
        act = (st["flags"] & 1) != 0
    ids = np.flatnonzero(act)
    deg = lattice_degree(ids, g) + 1
    k = emu.uniform(seed, emu.S_GOSSIP if alg == "gossip" else emu.S_PUSHSUM, ids, rnd, deg)
    return int(np.count_nonzero(k == deg - 1))


@functools.lru_cache(maxsize=None)
def reference(n, topo, alg, seed):
    """chunks = [(rounds asked, alerts of the chunk, state after it)] (the shape tsq.check takes), up to
    the case's stopping rule, its conditions asserted (module docstring)."""
    orc = Oracle(n, topo, alg, seed)
    P, T, g = orc.P, orc.T, emu.resolve(n, topo)[2]
    gossip = alg == "gossip"
    keys = ("c", "flags") if gossip else ("s", "w", "flags")
    late = 256 if topo == "line" else 64
    cap = 5000 if gossip else 20000 if topo == "line" else 400
    nbrs = {i: orc.neighbors(i) for i in list(range(0, P, max(1, P // 49))) + [P - 1]} if topo == "Imp3D" else {}
    chunks, st = [], None
    while True:
        if topo == "Imp3D" and orc.rounds >= 8:
            assert random_edge_senders(seed, alg, g, orc.rounds, st, orc.seed_node) >= 1, f"round {orc.rounds}"
        k = 1 if gossip and not chunks else 8 - orc.rounds % 8 if orc.rounds < 64 else late
        a = orc.step(k)
        full = orc.state()
        st = {key: full[key] for key in keys}
        for v in st.values():
            v.setflags(write=False)
        chunks.append((k, a, st))
        if gossip and len(chunks) == 1 and topo != "full":
            pick = int(emu.uniform(seed, emu.S_INJECT, np.array([0]), 0, T)[0])  # the list is still 0..T-1
            assert orc.injector_live == T and st["c"].sum() == 2 and st["c"][pick] >= 1
        if len(a) < k or orc.alerts_total >= T:
            break
        if gossip and 2 * np.count_nonzero(st["c"] >= 1) >= P and orc.alerts_total >= 1:
            break
        if not gossip and orc.active_count() == P and orc.alerts_total >= 1:
            break
        assert orc.rounds < cap, f"{topo} {alg} seed {seed:#x}: conditions not met after {orc.rounds} rounds"
    if gossip:
        assert 2 * np.count_nonzero(st["c"] >= 1) >= P and orc.alerts_total >= 1
    else:
        assert orc.active_count() == P and orc.alerts_total >= 1
    ref = Ref(chunks, orc.rounds, orc.alerts_total, T, orc.seed_node, nbrs)
    orc.close()
    return ref


def run(monkeypatch, n, topo, alg, seed, name, ranks=1, **env):
    """One handle against the oracle's run; overrides (any: the experiments build) set before create."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ref = reference(n, topo, alg, seed)
    sim = Sim(n, topo, alg, seed=seed, virtual_ranks=ranks, experimental=bool(env))
    try:
        assert sim.info().num_gpus == ranks
        assert sim.kernel_stats()[2] == name, sim.kernel_stats()[2]  # the intended kernel runs
        assert sim.seed_node == ref.seed_node
        for i, nb in ref.nbrs.items():
            assert sim.neighbors(i) == nb, i
        tsq.check(sim, ref)
    finally:
        sim.close()
    return ref


def multi_tile(topo, n, ranks=1):
    """Every slab holds more than one 1024-node tile."""
    assert all(s.nt > 1 for s in tsq.slabs(topo, n, ranks))


# ---------------------------------------------------------------- k_ps_tile
@pytest.mark.parametrize("seed", ALL)
def test_ps_tile_line(seed, monkeypatch):
    """256 x 4 class, <LINE>; all of WIDE_SEEDS (the family's first path)."""
    multi_tile("line", LINE)
    run(monkeypatch, LINE, "line", "push-sum", seed, "k_ps_tile<LINE>", GP_KERNEL="tile", GP_WIDE=0)


@pytest.mark.parametrize("topo", ["3D", "Imp3D"])
def test_ps_tile_lattices(topo, monkeypatch):
    """256 x 4 class, <GRID3D> and <IMP3D>: the staged in-edge sender tests (philox2_batch<F0>, <1>, <FU>)
    and the per-slot next-direction draw."""
    multi_tile(topo, G20)
    run(monkeypatch, G20, topo, "push-sum", W0, tsq.KERNEL["push-sum", topo], GP_KERNEL="tile", GP_WIDE=0)


PS_VARIANTS = {"slot_shadow0": {"GP_SLOT_SHADOW": 0},  # the batch draw at the tile's end
               "general_body": {"GP_NO_FULLTILE": 1},
               "unstaged": {"GP_STAGE_CAP": 0}}        # every tile: uniform() per in-edge


@pytest.mark.parametrize("variant", list(PS_VARIANTS))
def test_ps_tile_imp3d_variants(variant, monkeypatch):
    edges = np.bincount(emu.uniform(W0, emu.S_TOPO, np.arange(G20), 0, G20 - 1) // 1024, minlength=8)
    assert len(edges) == 8 and edges.min() > 0  # GP_STAGE_CAP=0: no tile's in-edges fit, all take the unstaged path
    run(monkeypatch, G20, "Imp3D", "push-sum", W0, "k_ps_tile<IMP3D>", GP_KERNEL="tile", GP_WIDE=0, **PS_VARIANTS[variant])


@pytest.mark.parametrize("n,topo", [(LINE, "line"), (G20, "3D")])
def test_ps_tile_wide_class(n, topo, monkeypatch):
    """The 1024-thread build (gp_ps_tile_wide.hip)."""
    run(monkeypatch, n, topo, "push-sum", W0, "wide::" + tsq.KERNEL["push-sum", topo], GP_KERNEL="tile", GP_WIDE=1)


def test_ps_tile_imp3d_two_virtual_ranks():
    """k_ps_tile<IMP3D, true> (product build), and the multi-rank topology set-up: k_topo_rnd_range
    draws every node's random edge, the in-lists built from it decide the first rounds' state."""
    multi_tile("Imp3D", G20, 2)
    run(None, G20, "Imp3D", "push-sum", W0, "k_ps_tile<IMP3D>", ranks=2)


# ---------------------------------------------------------------- k_gossip_tile (and k_finalize / _pre / _post)
@pytest.mark.parametrize("seed", ALL)
def test_gossip_tile_line(seed):
    """Product build; the injector draw of k_finalize."""
    multi_tile("line", LINE)
    run(None, LINE, "line", "gossip", seed, "k_gossip_tile<LINE>")


@pytest.mark.parametrize("topo", ["3D", "Imp3D"])
def test_gossip_tile_lattices(topo):
    """<GRID3D>, <IMP3D> with its in-edge pass (philox2_batch<FU>); one-rank Imp3D topology set-up."""
    run(None, G20, topo, "gossip", W0, tsq.KERNEL["gossip", topo])


@pytest.mark.parametrize("n,topo", [(LINE, "line"), (G20, "Imp3D")])
def test_gossip_tile_two_virtual_ranks(n, topo):
    """The injector replicated across ranks (k_finalize_pre / _post); Imp3D: the REMOTE instantiation."""
    run(None, n, topo, "gossip", W0, tsq.KERNEL["gossip", topo], ranks=2)


# ---------------------------------------------------------------- k_gossip_col
@pytest.mark.parametrize("seed", ALL)
def test_gossip_col_3d(seed, monkeypatch):
    run(monkeypatch, G20, "3D", "gossip", seed, "k_gossip_col<GRID3D>", GP_KERNEL="col")


@pytest.mark.parametrize("ranks", [1, 2])
def test_gossip_col_imp3d(ranks, monkeypatch):
    """Two ranks: the send bitmap and k_apply_bits."""
    run(monkeypatch, G20, "Imp3D", "gossip", W0, "k_gossip_col<IMP3D>", ranks=ranks, GP_KERNEL="col")


def round0_random_edge(seed):
    """The seed node of the g = 20 Imp3D gossip run of `seed` sends its round-0 rumour on its random edge."""
    node = emu.uniform(seed, emu.S_START, np.array([0]), 0, G20)
    deg = lattice_degree(node, 20) + 1
    return bool(emu.uniform(seed, emu.S_GOSSIP, node, 0, deg)[0] == deg[0] - 1)


def test_col_seed_init_random_edge(monkeypatch):
    """k_col_seed_init: the seed node's round-0 send goes along its random edge."""
    assert TOP in WIDE_SEEDS and round0_random_edge(TOP)
    run(monkeypatch, G20, "Imp3D", "gossip", TOP, "k_gossip_col<IMP3D>", GP_KERNEL="col")


# ---------------------------------------------------------------- k_ps_block
@pytest.mark.parametrize("seed", ALL)
def test_ps_block(seed, monkeypatch):
    """g = 20: eight boxes (the smallest multi-box lattice of test_block_kernel_parity)."""
    run(monkeypatch, G20, "3D", "push-sum", seed, "k_ps_block<GRID3D>", GP_KERNEL="block")


# ---------------------------------------------------------------- full topology
@pytest.mark.parametrize("seed", ALL)
def test_full_gossip_one_rank(seed):
    """k_full_gossip_send (gp_kernels.hip)."""
    run(None, FULL_G, "full", "gossip", seed, "k_full_gossip_send+recv")


def test_full_gossip_three_ranks():
    """k_fullm_gossip_send (gp_full.hip)."""
    run(None, FULL_G, "full", "gossip", W0, "k_full_gossip_send+recv", ranks=3)


FULL_PS_CASES = [pytest.param(s, 1, None, id=f"fused-{s:#x}") for s in WIDE_SEEDS] + \
                [pytest.param(W0, 1, "0", id="three_pass-W0"), pytest.param(W0, 3, None, id="ranks3-W0")]


@pytest.mark.parametrize("seed,ranks,fused", FULL_PS_CASES)
def test_full_pushsum(seed, ranks, fused, monkeypatch):
    """gp_fullbin.hip: the fused form, the three-pass form (GP_FB_FUSED=0) and three ranks (k_fbm_send)."""
    env = {} if fused is None else {"GP_FB_FUSED": fused}
    name = "k_fb_send+split+fold" if fused == "0" else "k_fb_split+fold<send>"
    run(monkeypatch, FULL_PS, "full", "push-sum", seed, name, ranks=ranks, **env)


# ---------------------------------------------------------------- front doors
CLI = os.path.join(ROOT, "gossipprotocol_amd", "gossip")


def test_python_front_door():
    """Simulation(seed=2**64 - 1): the whole range passes through ctypes into gp_config.seed."""
    run(None, LINE, "line", "gossip", TOP, "k_gossip_tile<LINE>")


@functools.lru_cache(maxsize=None)
def converged_line_gossip(seed):
    orc = Oracle(LINE, "line", "gossip", seed)
    orc.run()
    assert orc.alerts_total >= orc.T
    want = ref_summary(orc.state(), 0, orc.P, orc.rounds, 0, orc.seed_node, 1e-10)
    out = (orc.rounds, want["converged"], want["c_max"], want["c_hist"])
    orc.close()
    return out


def cli_run(args, env=None):
    """A fresh `gossip` process; (rounds, converged, c_max, c_hist) from its --stats and --summary lines."""
    r = subprocess.run([CLI, str(LINE), "line", "gossip", "--stats", "--summary"] + args, capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    words = dict(w.split("=", 1) for line in r.stdout.splitlines()[2:] for w in line.split() if "=" in w)
    return int(words["rounds"]), int(words["converged"]), int(words["c_max"]), [int(v) for v in words["c_hist"].split(",")]


def test_cli_seed_option():
    assert converged_line_gossip(TOP) != converged_line_gossip(TOP & 0xFFFFFFFF)  # the high word shows in the result
    assert cli_run(["--seed", str(TOP)]) == converged_line_gossip(TOP)


def test_cli_seed_environment():
    assert str(TOP) == "18446744073709551615"
    assert cli_run([], {"GOSSIP_SEED": str(TOP)}) == converged_line_gossip(TOP)


def test_rccl_rank_processes():
    """Two rank processes over RCCL, 100 rounds: every rank's alerts and slab state equal the
    single-process run's (which test_gossip_tile_line compares with the oracle)."""
    from tests.test_gpu_rccl_multiproc import run_ranks
    recs = run_ranks(2, LINE, "line", "gossip", W0, 100)
    with Sim(LINE, "line", "gossip", seed=W0) as one:
        want, full = one.step(100), one.state()
    orc = [a for k, al, st in reference(LINE, "line", "gossip", W0).chunks for a in al][:100]
    assert len(orc) >= 64 and want[:len(orc)] == orc
    for r, rec in enumerate(recs):
        assert list(rec["alerts"]) == want, f"rank {r}"
        lo, cnt = int(rec["first"]), len(rec["c"])
        assert_same_state("gossip", {k: rec[k] for k in ("c", "flags")}, {k: full[k][lo:lo + cnt] for k in ("c", "flags")})
    assert sorted(int(rec["first"]) for rec in recs)[0] == 0 and sum(len(rec["c"]) for rec in recs) == LINE + 1
