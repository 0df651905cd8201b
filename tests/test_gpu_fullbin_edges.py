"""GPU: full-topology push-sum (gp_fullbin.hip: k_fb_send, k_fbm_send, k_fb_split, k_fb_fold) at its
slab, bin-size and capacity edges, bit-exact against the CPU oracle on s, w, flags and per-round
alerts.  Every case first shows on the CPU -- from the slab bounds (multirank_emu.slab_bounds /
full_region / full_bin_multi_s1 / full_bin_plan, restatements of gp_plan.hpp that test_plan.py compares with it) and from the
Philox draws of the oracle's own senders (multirank_emu.uniform / full_target; the senders of round r
are the nodes whose active flag the oracle shows at its start) -- that it is where it claims to be.

A  slab and region edges across (virtual) ranks, product build: one node per rank (P = W), slabs one
   id short of / on / one id past a fine tile (4096 receivers, counted from the slab's lo), an empty
   exchange region 0 (a slab of one tile), regions of 1 and 2 tiles (three tiles), and multi_key's
   rank step -- a round in which one message goes to bounds[w] and one to bounds[w] - 1.
B  coarse bins larger than a fine tile across ranks (s1 = 13, 14: k_fb_split<true> with nfine = 2, 4,
   multi_key with several tiles per bin), next to the last size with s1 = 12.
C  the several-rank fold walking a second tile: a region of CUs + 1 tiles is folded by CUs blocks, so
   block 0 runs the prefetch of the next tile's messages (n_pf, the fn < t_hi reload) and the per-tile
   LDS re-zeroing once.
D  the capacity comparisons, experiments build: GP_FB_CAP2 / GP_FB_CAP1 put the bins' capacity at the
   largest number of messages M a fine tile / coarse bin receives in any round of the run (bit-exact:
   the last slot is used) and at M - 1 (the step fails with GP_ESTATE "overflow", the simulation closes,
   and a fresh default one is bit-exact again).

The stores the M - 1 cases reach were read before those cases were first run, and each is bounded by the
capacity the run was given: fbr_emit drops a message whose slot is >= cap (or whose bin is >= the bin
count) before it forms the address; MultiOutLds::store drops pos >= cap[b]; the fused fold's write-out
sends a slot >= cap1 to the FB_JUNK slots past the last bin, which alloc_slab allocates behind
nb1 * cap1 with the overridden cap1; the consuming sides read min(count, cap) messages (k_fb_split's
n_bin, the fold's n / n_pf).  The point of D is the designed error path, not a fault.
"""
import functools

import numpy as np
import pytest
# torch is imported before the library is first loaded: it ships a HIP runtime of its own, and group C's
# device query finds no GPU if the process has already loaded another one
import torch

from tests.multirank_emu import (FB_TB, S_PUSHSUM, S_START, full_bin_multi_cap, full_bin_multi_s1, full_bin_plan,
                                 full_region, full_target, slab_bounds, uniform)
from tests.oracle_ctypes import Oracle
from tests.test_gpu_parity import Sim, assert_same_state

pytestmark = pytest.mark.gpu

TILE = 1 << FB_TB
FB_CAP2 = 4992  # gp_fullbin.hpp


def targets(P, seed, rnd, senders):
    """The targets the senders draw in round rnd (Program.fs:211-216; k_fb_send / the fold's send phase)."""
    return full_target(senders, uniform(seed, S_PUSHSUM, senders, rnd, P - 1))


def slabs(P, W):
    bounds, halo = slab_bounds(P, 0, "full", W)
    assert halo == 0 and bounds[0] == 0 and bounds[-1] == P
    return bounds


def tiles_of(n):
    return -(-n // TILE)


def region_tiles(n):
    """Fine tiles of a slab's two exchange regions."""
    out = []
    for h in range(2):
        r0, r1 = full_region(n, 2, h)
        assert r0 % TILE == 0 and (r1 % TILE == 0 or r1 == n)
        out.append(tiles_of(r1) - r0 // TILE)
    return tuple(out)


# ---------------------------------------------------------------- A: slab and region edges
def rank_step_round(P, W, seed, rounds, first_state, first_rounds):
    """Activation replayed from the draws (a node is active from the round after its first message):
    the first round < `rounds` in which, for one inner w, one message goes to bounds[w] and one to
    bounds[w] - 1, or None.  The replay is checked against the oracle: its active set after the
    oracle's first `first_rounds` rounds is the oracle's."""
    bounds = np.array(slabs(P, W)[1:-1])
    active = np.zeros(P, dtype=bool)
    active[int(uniform(seed, S_START, np.array([0]), 0, P - 1)[0])] = True
    found = None
    assert 1 <= first_rounds <= rounds
    for r in range(min(rounds, max(first_rounds, 64))):
        t = targets(P, seed, r, np.nonzero(active)[0])
        if found is None and np.any(np.isin(bounds, t) & np.isin(bounds - 1, t)):
            found = r
        active[t] = True
        if r + 1 == first_rounds:
            np.testing.assert_array_equal(active, (first_state["flags"] & 1) != 0)
        if r + 1 >= first_rounds and found is not None:
            break
    return found


def _even(n, W):
    return [n] * W


EDGE_CASES = [  # (W, P, seed, slab sizes, tiles per slab)
    (2, 2, 1, [1, 1], [1, 1]),
    (2, 3, 1, [1, 2], [1, 1]),
    (2, 8191, 1, [4095, 4096], [1, 1]),
    (2, 8192, 1, [4096, 4096], [1, 1]),
    (2, 8193, 1, [4096, 4097], [1, 2]),       # slab 1: a second tile with one receiver, one tile per region
    (2, 24576, 1, [12288, 12288], [3, 3]),    # regions of 1 and 2 tiles
    (3, 3, 1, [1, 1, 1], [1, 1, 1]),
    (3, 4, 1, [1, 1, 2], [1, 1, 1]),
    (3, 12287, 1, [4095, 4096, 4096], [1, 1, 1]),
    (3, 12288, 1, [4096, 4096, 4096], [1, 1, 1]),
    (3, 12289, 1, [4096, 4096, 4097], [1, 1, 2]),
    (16, 16, 1, _even(1, 16), _even(1, 16)),  # one node per rank
    (16, 17, 1, _even(1, 15) + [2], _even(1, 16)),
    (16, 65536, 1, _even(4096, 16), _even(1, 16)),
    (16, 65537, 1, _even(4096, 15) + [4097], _even(1, 15) + [2]),
]


@pytest.mark.parametrize("W,P,seed,sizes,tiles", EDGE_CASES, ids=[f"W{c[0]}-P{c[1]}" for c in EDGE_CASES])
def test_slab_and_region_edges(W, P, seed, sizes, tiles):
    """Through convergence (at most 400 rounds), state every 25 rounds."""
    bounds = slabs(P, W)
    assert [bounds[w + 1] - bounds[w] for w in range(W)] == sizes
    assert [tiles_of(n) for n in sizes] == tiles
    for n, nt in zip(sizes, tiles):
        # one tile: region 0 is empty; two: one each; three: 1 and 2
        assert region_tiles(n) == {1: (0, 1), 2: (1, 1), 3: (1, 2)}[nt]
        if n % TILE == 1:
            assert full_region(n, 2, 1)[1] - (nt - 1) * TILE == 1  # the last tile holds one receiver
    assert full_bin_multi_s1(bounds) == FB_TB  # coarse bin = fine tile; the larger bins are group B's

    sim, orc = Sim(P - 1, "full", "push-sum", seed=seed, virtual_ranks=W), Oracle(P - 1, "full", "push-sum", seed)
    assert sim.info().num_gpus == W and sim.population == orc.P == P
    done, first = 0, None
    while done < 400:
        ga, oa = sim.step(25), orc.step(25)
        assert ga == oa, f"alerts differ in rounds {done}..{done + 25}"
        ost = orc.state()
        assert_same_state("push-sum", sim.state(), ost)
        if first is None:
            first = (ost, len(oa))
        done += len(oa)
        if len(oa) < 25:
            break
    assert sim.rounds == orc.rounds == done and sim.alerts_total == orc.alerts_total
    sim.close()
    # multi_key's rank step: targets on both sides of an inner slab bound in one round of this run
    assert rank_step_round(P, W, seed, done, *first) is not None
    orc.close()


# ---------------------------------------------------------------- B: coarse bins of several fine tiles
def both_regions_reach_every_fine_tile(P, W, seed, rnd, active, s1):
    """Round rnd, senders = `active`: for every destination rank b, some coarse bin of b gets messages
    for each of its fine tiles from both exchange regions of the next rank."""
    bounds = slabs(P, W)
    nfine = 1 << (s1 - FB_TB)
    for b in range(W):
        a = (b + 1) % W
        lo_a, n_a, lo_b, n_b = bounds[a], bounds[a + 1] - bounds[a], bounds[b], bounds[b + 1] - bounds[b]
        nb = -(-n_b // (1 << s1))
        ok = np.ones(nb, dtype=bool)
        for h in range(2):
            r0, r1 = full_region(n_a, 2, h)
            snd = lo_a + r0 + np.nonzero(active[lo_a + r0:lo_a + r1])[0]
            t = targets(P, seed, rnd, snd)
            t = t[(t >= lo_b) & (t < lo_b + n_b)] - lo_b
            per = np.bincount(t >> FB_TB, minlength=nb * nfine)[:nb * nfine].reshape(nb, nfine)
            assert per.sum(axis=1).max() <= full_bin_multi_cap(r1 - r0, s1, P)  # within the exchange bins
            ok &= np.all(per > 0, axis=1)
        if not ok.any():
            return False
    return True


@pytest.mark.parametrize("W,P,seed,s1", [(2, 786432, 2, 12), (2, 786434, 2, 13), (3, 1600000, 2, 14)],
                         ids=lambda v: str(v))
def test_coarse_bins_of_several_fine_tiles(W, P, seed, s1):
    """Until the oracle shows every node active plus 8 rounds (at most 48), state every 8 rounds.
    786 432: 2 x 96 tiles = 192 keys, the last size with coarse bin = fine tile; 786 434: 2 x 97
    tiles, so bins of two tiles; 1 600 000 over three ranks: 393 tiles, bins of four."""
    bounds = slabs(P, W)
    assert full_bin_multi_s1(bounds) == s1
    keys = sum(-(-(bounds[w + 1] - bounds[w]) // (1 << s1)) for w in range(W))
    assert keys <= 192 and (s1 == FB_TB or sum(tiles_of(bounds[w + 1] - bounds[w]) for w in range(W)) > 192)
    sim, orc = Sim(P - 1, "full", "push-sum", seed=seed, virtual_ranks=W), Oracle(P - 1, "full", "push-sum", seed)
    assert sim.info().num_gpus == W
    done, full, finished = 0, False, False
    while done < 48 and not finished:
        ga, oa = sim.step(8), orc.step(8)
        assert ga == oa, f"alerts differ in rounds {done}..{done + 8}"
        ost = orc.state()
        assert_same_state("push-sum", sim.state(), ost)
        done += 8
        finished = full
        if not full and orc.active_count() == P:
            # the next chunk's first round: every node sends
            active = (ost["flags"] & 1) != 0
            assert active.all()
            assert both_regions_reach_every_fine_tile(P, W, seed, done, active, s1)
            full = True
    assert finished, "the run did not reach 8 rounds with every node active within 48"
    sim.close()
    orc.close()


# ---------------------------------------------------------------- C: the fold's second tile
def test_fold_walks_a_second_tile():
    """W = 2, slabs of 2 (CUs + 1) tiles, the last one partial: each exchange region has CUs + 1
    tiles and launch_full_bin_fold_multi gives it CUs blocks, so block 0 folds tiles 0 and CUs of its
    region (the second one's messages prefetched behind the first one's send phase) and every
    other block one.  State mid-activation (round 16) and two rounds after the last node became
    active.  P = 4 208 768 on 256 CUs: every node is active after 37 rounds, so 39 rounds in all; the
    oracle's share measured 2.7 s on the CPUs of the build host (its threads = all cores), and the whole
    test 0.9 s on the MI355X host -- far below the 10 s at which rounds would have to be cut."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, seed = 2, 3
    P = 4 * (cus + 1) * TILE - 2000
    bounds = slabs(P, W)
    for w in range(W):
        n = bounds[w + 1] - bounds[w]
        assert n == 2 * (cus + 1) * TILE - 1000 and tiles_of(n) == 2 * (cus + 1) and n % TILE != 0
        assert region_tiles(n) == (cus + 1, cus + 1)  # min(tiles, CUs) = CUs blocks: block 0 walks two
    sim, orc = Sim(P - 1, "full", "push-sum", seed=seed, virtual_ranks=W), Oracle(P - 1, "full", "push-sum", seed)
    assert sim.step(16) == orc.step(16)
    assert 0 < orc.active_count() < P
    assert_same_state("push-sum", sim.state(), orc.state())
    while orc.active_count() < P:
        assert orc.rounds < 46, "activation did not complete"
        assert sim.step(1) == orc.step(1)
    assert sim.step(2) == orc.step(2)
    assert sim.info().active == P
    assert_same_state("push-sum", sim.state(), orc.state())
    sim.close()
    orc.close()


# ---------------------------------------------------------------- D: capacity edges
D_SEED = 4


def plan_of(P, fused):
    """(s1, nb1, cap1) of one rank's coarse bins."""
    nb1, cap1, nb2, cap2 = full_bin_plan(P, fused=fused)
    assert nb2 == tiles_of(P) and cap2 == FB_CAP2
    (s1,) = [s for s in range(FB_TB, 25) if -(-P // (1 << s)) == nb1]
    return s1, nb1, cap1


@functools.lru_cache(maxsize=None)
def stepped(P, seed=D_SEED):
    """The oracle stepped one round at a time for R = (rounds until every node is active) + 6 rounds:
    (R, alerts per round, the senders of rounds 0..R, state after R rounds)."""
    orc = Oracle(P - 1, "full", "push-sum", seed)
    alerts, senders, full = [], [], None
    while full is None or len(alerts) < full + 6:
        flags = orc.state()["flags"]
        senders.append(np.nonzero(flags & 1)[0])
        if full is None and len(senders[-1]) == P:
            full = len(alerts)
        assert len(alerts) < 200
        alerts += orc.step(1)
    senders.append(np.nonzero(orc.state()["flags"] & 1)[0])  # round R's: the fused fold of R - 1 bins them
    st = orc.state()
    for v in st.values():
        v.setflags(write=False)
    assert orc.alerts_total < orc.T  # the run is still going: gp_step executes all R rounds
    orc.close()
    return len(alerts), alerts, senders, st


def fullest(P, bounds, shift, rounds, seed=D_SEED):
    """The largest number of messages one bin of 2^shift receivers (counted from its slab's lo) gets
    in any of the rounds."""
    _, _, senders, _ = stepped(P, seed)
    b = np.array(bounds)
    most = 0
    for r in rounds:
        t = targets(P, seed, r, senders[r])
        w = np.searchsorted(b, t, side="right") - 1
        key = w * (1 << 32) + ((t - b[w]) >> shift)
        most = max(most, int(np.unique(key, return_counts=True)[1].max()))
    return most


def run_exact(P, W, monkeypatch, env, seed=D_SEED):
    """R rounds in one step, with the overrides of env (none: the product build): bit-exact."""
    R, alerts, _, st = stepped(P, seed)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    sim = Sim(P - 1, "full", "push-sum", seed=seed, virtual_ranks=W, experimental=bool(env))
    if W == 1:
        assert sim.kernel_stats()[2] == ("k_fb_send+split+fold" if env.get("GP_FB_FUSED") == "0" else "k_fb_split+fold<send>")
    assert sim.step(R) == alerts
    assert_same_state("push-sum", sim.state(), st)
    sim.close()
    for k in env:
        monkeypatch.delenv(k)


def run_overflow(P, W, monkeypatch, env, seed=D_SEED):
    """The same run one slot short: the step fails, the simulation closes, and a fresh default one is
    bit-exact (nothing was written past a bin)."""
    from gossipprotocol_amd._lib import GossipError
    R = stepped(P, seed)[0]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    sim = Sim(P - 1, "full", "push-sum", seed=seed, virtual_ranks=W, experimental=True)
    with pytest.raises(GossipError) as e:
        sim.step(R)
    assert e.value.code == -5 and "overflow" in str(e.value)
    sim.close()
    for k in env:
        monkeypatch.delenv(k)
    run_exact(P, W, monkeypatch, {}, seed)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("which", ["cap2", "cap1"])
def test_one_rank_capacity_edges(which, fused, monkeypatch):
    """P = 20 481: six fine tiles, the last with one receiver; fused s1 = 13, three coarse bins (three
    passes: s1 = 14, two).  cap2: pos >= cap in k_fb_split's fbr_emit, min(cnt2, cap2) in the fold.
    cap1: pos >= cap in k_fb_send's fbr_emit (round 0, and every round of the three-pass form),
    slot >= cap1 in the fused fold's write-out, min(cnt1, cap1) in k_fb_split.  The fused fold of round
    R - 1 bins round R's messages, so the fused form's M1 includes round R."""
    P = 20481
    s1, nb1, cap1 = plan_of(P, fused == "1")
    assert (s1, nb1) == ((13, 3) if fused == "1" else (14, 2))
    assert tiles_of(P) == 6 and P % TILE == 1
    R = stepped(P)[0]
    M2 = fullest(P, [0, P], FB_TB, range(R))
    M1 = fullest(P, [0, P], s1, range(R + 1) if fused == "1" else range(R))
    assert M2 < FB_CAP2 and M1 < cap1  # the overrides below lower the capacities
    assert M2 > TILE // 2 and M1 > (1 << s1) // 2  # a round with (nearly) every node sending is in the run
    var, M = ("GP_FB_CAP2", M2) if which == "cap2" else ("GP_FB_CAP1", M1)
    run_exact(P, 1, monkeypatch, {"GP_FB_FUSED": fused, var: M})
    run_overflow(P, 1, monkeypatch, {"GP_FB_FUSED": fused, var: M - 1})


def test_two_rank_fine_tile_capacity_edge(monkeypatch):
    """W = 2, P = 24 577: slabs of 12 288 (three tiles) and 12 289 (four, the last with one receiver),
    fine tiles counted from each slab's lo; GP_FB_CAP2 at the fullest tile of either slab and one
    below (k_fb_split<true>'s fbr_emit, the fold's min(cnt2, cap2))."""
    P, W = 24577, 2
    bounds = slabs(P, W)
    assert bounds == [0, 12288, 24577] and full_bin_multi_s1(bounds) == FB_TB
    R, _, senders, _ = stepped(P)
    M2 = fullest(P, bounds, FB_TB, range(R))
    assert TILE // 2 < M2 < FB_CAP2
    # the exchange bins themselves (not overridden) hold every round's messages, round R's included
    for w in range(W):
        n = bounds[w + 1] - bounds[w]
        for h in range(2):
            r0, r1 = full_region(n, 2, h)
            for r in range(R + 1):
                snd = senders[r][(senders[r] >= bounds[w] + r0) & (senders[r] < bounds[w] + r1)]
                t = targets(P, D_SEED, r, snd)
                own = np.searchsorted(np.array(bounds), t, side="right") - 1
                key = own * (1 << 32) + ((t - np.array(bounds)[own]) >> FB_TB)
                if len(key):
                    assert np.unique(key, return_counts=True)[1].max() <= full_bin_multi_cap(r1 - r0, FB_TB, P)
    run_exact(P, W, monkeypatch, {"GP_FB_CAP2": M2})
    run_overflow(P, W, monkeypatch, {"GP_FB_CAP2": M2 - 1})
