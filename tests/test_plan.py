"""The multi-rank run plan (gossipprotocol_amd/csrc/gp_plan.hpp), evaluated on the host, against
its Python restatements.

The GPU edge tests (test_gpu_fullbin_edges.py, test_gpu_gossip_edges.py, test_gpu_multirank.py)
derive on the CPU which path each of their cases reaches -- slab bounds, regions, bin sizes,
capacities -- from the functions of tests/multirank_emu.py.  Here the header itself, compiled with
the host compiler into tests/helpers/plan_check.cpp, gets the same inputs as those functions and
must give the same results, exactly: the inputs are the cases the edge tests rely on plus the large
configurations.  The byte layout of every rank's exchange buffers is checked for all ranks before
anything runs (no overlap; what a sends is what b expects; a addresses b's vals region where b
reads it), which the library otherwise checks only at run time between in-process ranks
(run_transfers, gp_exchange.hip).  CPU-only: compiles a small host program.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import multirank_emu as emu
from tests.test_gpu_lattice_rank_edges import GRID_E, LINE_SHAPES, demonstrate, shape

HERE = os.path.dirname(os.path.abspath(__file__))
XMAXH = 8


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "helpers", "plan_check.cpp")])

    def ask(queries):
        """One line of integers per query; ' ; ' separates the groups of a result."""
        text = "".join(" ".join(str(x) for x in q) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(queries)
        res = []
        for q, line in zip(queries, out):
            name, _, rest = line.partition(" ")
            assert name == q[0] and rest.strip() != "?", line
            groups = [[int(x) for x in grp.split()] for grp in rest.split(";")]
            res.append(groups[0] if len(groups) == 1 else groups)
        return res
    return ask


def test_constants(plan):
    (k,) = plan([("K",)])
    assert k == [16, 8, emu.XTILE, emu.HALO_CHUNK, 8, emu.XREGIONS, emu.RREG_MIN_NODES, 1024, emu.FB_TB, 4992, 64,
                 emu.FB_REGIONS, 4096, 1024, emu.FBM_KEYS]
    assert emu.full_bin_plan(10**6)[3] == 4992  # FB_CAP2


# full topology: one node per rank; slabs one id short of, on and one past a fine tile; coarse bins
# larger than a fine tile; the large configuration (C4 at W = 8)
FULL_CASES = [(W, P) for W in (2, 3, 16) for P in (W, W + 1, 4096 * W - 1, 4096 * W, 4096 * W + 1)] + \
    [(2, 24576), (2, 24577), (2, 786432), (2, 786434), (3, 1600000), (8, 10**8)]


@pytest.mark.parametrize("W,n", FULL_CASES)
def test_full_topology_plan(plan, W, n):
    P, _, g = emu.resolve(n, "full")
    bounds, halo = emu.slab_bounds(P, g, "full", W)
    (got,) = plan([("bounds", P, g, W, 1)])
    assert got == [0, halo] + bounds
    s1 = emu.full_bin_multi_s1(bounds)
    assert plan([("multi_s1", W, *bounds)]) == [[s1]]
    q, want = [], []
    for a in range(W):
        na = bounds[a + 1] - bounds[a]
        nb = -(-na // (1 << s1))
        q.append(("coarse_bins", a, s1, W, *bounds))
        want.append([nb])
        for h in range(2):
            s_lo, s_hi = emu.full_region(na, 2, h)
            nt = -(-na // 4096)
            q.append(("full_region", na, 2, h))
            want.append([nt * h // 2, nt * (h + 1) // 2, s_lo, s_hi])
            cap = emu.full_bin_multi_cap(s_hi - s_lo, s1, P)
            q.append(("multi_cap", s_hi - s_lo, s1, P))
            want.append([cap])
            q.append(("bins_bytes", nb, cap))
            want.append([(nb * 4 + 15) // 16 * 16, (nb * 4 + 15) // 16 * 16 + (nb * cap * 4 + 15) // 16 * 16,
                         emu.fb_bins_bytes(nb, cap)])
            for b in range(W):  # gossip: the pair capacities
                q.append(("pair_cap", s_hi - s_lo, bounds[b + 1] - bounds[b], P))
                want.append([emu.full_capacity(s_hi - s_lo, bounds[b + 1] - bounds[b], P)])
    assert plan(q) == want


# the shapes of tests/test_gpu_lattice_rank_edges.py: (topology, size, W), size = P for the line, g for 3D
LATTICE_RANK_EDGE_SHAPES = [("line", P, W) for W, P in LINE_SHAPES] + [("3D", g, W) for g, W in GRID_E]


@pytest.mark.parametrize("topo,size,W", LATTICE_RANK_EDGE_SHAPES, ids=lambda v: str(v))
def test_lattice_rank_edge_shapes(plan, topo, size, W):
    """Slab bounds, halo and tiles per slab of the line and 3D edge cases: the header's against the
    restatements the cases derive their cut positions from."""
    sh = shape(topo, size, W)
    bounds, halo = emu.slab_bounds(sh.P, sh.g, topo, W)
    q = [("bounds", sh.P, sh.g, W, 0 if topo == "line" else 2)]
    q += [("tiles_for", lo, hi - lo) for lo, hi in zip(bounds, bounds[1:])]
    got = plan(q)
    assert got[0] == [0, halo] + bounds and sh.bounds == bounds
    assert [t for (t,) in got[1:]] == sh.tiles == [emu.tiles_for(lo, hi - lo) for lo, hi in zip(bounds, bounds[1:])]


@pytest.mark.parametrize("alg", ["push-sum", "gossip"])
@pytest.mark.parametrize("topo,size,W", LATTICE_RANK_EDGE_SHAPES, ids=lambda v: str(v))
def test_lattice_rank_edge_demonstrations(topo, size, W, alg):
    """The CPU demonstration of every case of tests/test_gpu_lattice_rank_edges.py with its committed
    seed and round count (oracle and Philox draws only): a send up and a send down across every cut
    within the executed rounds, the cut nodes active (gossip: reached) at the last checkpoint."""
    t = demonstrate(topo, size, W, alg)
    assert sorted(t.states)[-1] == t.R == len(t.alerts)


def test_bounds_rejections_and_cuts(plan):
    got = plan([("bounds", 1000, 0, 1, 1), ("bounds", 1000, 0, 17, 0), ("bounds", 3, 0, 4, 1), ("bounds", 3, 0, 4, 0),
                ("bounds", 27, 3, 4, 2), ("bounds", 1001, 0, 3, 0), ("bounds", 8000, 20, 3, 2)])
    assert got[0] == [0, 0, 0, 1000]
    assert [g[0] for g in got[1:5]] == [1, 2, 2, 3]  # too many ranks; fewer nodes; fewer planes than ranks
    assert got[5] == [0, 1] + emu.slab_bounds(1001, 0, "line", 3)[0]
    assert got[6] == [0, 400] + emu.slab_bounds(8000, 20, "3D", 3)[0]


@pytest.mark.parametrize("P", [2, 4097, 20481, 10**6, 100000001, 2**31 + 5, 2**32 - 1])
def test_full_bin_plan(plan, P):
    for fused in (False, True):
        (got,) = plan([("bin_plan", P, int(fused))])
        nb1, cap1, nb2, cap2 = emu.full_bin_plan(P, fused=fused)
        assert (got[1], got[3], got[2], got[4]) == (nb1, cap1, nb2, cap2)
        assert nb1 == -(-P // (1 << got[0]))


def imp3d_slabs(g, W):
    return emu.slab_bounds(g ** 3, g, "Imp3D", W)[0]


# g = 40 / W = 8 (the emulation's plan); g = 20: slabs plane-aligned but tile-unaligned; a line slab
# (no planes: equal tile counts); g = 1000: the large configuration and the eight-region rule; then the
# shapes of tests/test_gpu_list_edges.py (groups A-E; NH = 8 at W = 2 is its group C)
LIST_EDGE_SHAPES = [(32, 2), (64, 4), (64, 2), (64, 8), (64, 16), (48, 2), (48, 3), (33, 2), (33, 3), (5, 5), (3, 3),
                    (2, 2), (19, 16), (20, 16), (6, 2), (31, 2), (31, 3), (32, 3)]


@pytest.mark.parametrize("g,W", [(40, 8), (20, 2), (20, 3), (0, 3), (1000, 2), (1000, 8)] + LIST_EDGE_SHAPES)
@pytest.mark.parametrize("NH", [4, 8])
def test_tiles_and_regions(plan, g, W, NH):
    bounds = imp3d_slabs(g, W) if g else emu.slab_bounds(100001, 0, "line", W)[0]
    q, want = [], []
    for a in range(W):
        lo, nloc = bounds[a], bounds[a + 1] - bounds[a]
        nt = emu.tiles_for(lo, nloc)
        tb = emu.region_tiles(lo, nloc, g * g, NH, nt)
        q.append(("tiles_for", lo, nloc))
        want.append([nt])
        q.append(("list_region_tiles", lo, nloc, g * g, NH))
        want.append(tb + [nt] * (XMAXH - NH))
        q.append(("region_tiles", lo, nloc, g * g, NH))
        want.append([1] + tb if g else [0] * (NH + 2))
        assert tb[0] == 0 and tb[NH] == nt and all(x <= y for x, y in zip(tb, tb[1:]))
        for h in range(NH):
            q.append(("xregion", lo, nloc, 1, NH, h, *(tb + [nt] * (XMAXH - NH))))
            want.append(list(emu.xregion(lo, nloc, tb, NH, h)))
        regions = [emu.xregion(lo, nloc, tb, NH, h) for h in range(NH)]  # consecutive, covering the slab
        assert regions[0][0] == 0 and regions[-1][1] == nloc and all(r[1] == s[0] for r, s in zip(regions, regions[1:]))
    assert plan(q) == want


def test_exchange_regions_and_the_eight_region_rule(plan):
    M = emu.RREG_MIN_NODES
    cases = [("Imp3D", 2, imp3d_slabs(1000, 2)), ("Imp3D", 8, imp3d_slabs(1000, 8)), ("Imp3D", 2, imp3d_slabs(20, 2)),
             ("Imp3D", 2, [0, M, 2 * M]), ("Imp3D", 2, [0, M - 4096, 2 * M]), ("Imp3D", 2, [0, M + 4096, 2 * M + 4095]),
             ("Imp3D", 3, [0, M, 2 * M, 3 * M]), ("full", 2, [0, M, 2 * M]), ("full", 3, [0, 4096, 8192, 12289])]
    q = [("exchange_regions", int(push), int(topo == "Imp3D"), W, *b) for topo, W, b in cases for push in (0, 1)]
    want = [[emu.exchange_regions(bool(push), topo, W, b)] for topo, W, b in cases for push in (0, 1)]
    assert plan(q) == want
    assert [w[0] for w in want[1::2]] == [8, 4, 4, 8, 4, 4, 4, 2, 2]
    # region rounds: every slab at least RREG_MIN_NODES, whole planes, 2..8 regions
    got = plan([("round_regions", 10**6, 8, 2, *imp3d_slabs(1000, 2)), ("round_regions", 10**6, 4, 8, *imp3d_slabs(1000, 8)),
                ("round_regions", 400, 4, 2, *imp3d_slabs(20, 2)), ("round_regions", 4096, 8, 2, 0, M, 2 * M),
                ("round_regions", 4096, 8, 2, 0, M - 4096, 2 * M - 4096), ("round_regions", 4096, 1, 2, 0, M, 2 * M),
                ("round_regions", 4096, 4, 2, 0, M + 1, 2 * M + 2)])
    assert got == [[1, 1], [1, 1], [0, 1], [1, 1], [0, 1], [1, 0], [1, 0]]


@pytest.mark.parametrize("g", [100, 465, 1000, 1625, 31, 32, 33, 2, 3, 5, 6, 19, 48, 64])
def test_halo_chunk_cap(plan, g):
    got = plan([("halo_cap", g, 0), ("halo_cap", g, 1)])
    caps = [emu.halo_chunk_cap(g, False), emu.halo_chunk_cap(g, True)]
    assert got == [[caps[0]], [caps[1]]]
    assert plan([("halo_slots", g * g, caps[0])]) == [[-(-g * g // 1024) * caps[0]]]
    assert plan([("halo_slots", g * g, caps[1])]) == [[-(-g * g // 1024) * caps[1]]]


def make_list_plan(g, W, seed, NH=4):
    P = g ** 3
    bounds, _ = emu.slab_bounds(P, g, "Imp3D", W)
    rnd = emu.uniform(seed, emu.S_TOPO, np.arange(P), 0, P - 1)
    return emu.ListPlan(P, g, W, bounds, rnd, emu.Geometry(P, g, "Imp3D", seed), NH=NH), rnd, g


@pytest.fixture(scope="module")
def list_plan():
    """The plan test_multigpu_plan.py draws: P = 64000 (g = 40), W = 8, seed 5."""
    return make_list_plan(40, 8, 5)


# the plans of tests/test_gpu_list_edges.py, its seeds: (g, W, seed, NH)
LIST_EDGE_PLANS = [(32, 2, 1, 4), (64, 4, 1, 4), (64, 8, 1, 4), (64, 16, 1, 4), (48, 2, 1, 4), (48, 3, 1, 4), (33, 2, 1, 4),
                   (33, 3, 1, 4), (5, 5, 1, 4), (3, 3, 1, 4), (2, 2, 1, 4), (2, 2, 6, 4), (19, 16, 1, 4), (33, 2, 1, 8),
                   (64, 2, 1, 8), (6, 2, 1, 8)]


def test_list_tables_and_chunk_offsets(plan, list_plan):
    check_list_tables_and_chunk_offsets(plan, *list_plan)


@pytest.mark.parametrize("case", LIST_EDGE_PLANS, ids=lambda c: "g%d-W%d-s%d-NH%d" % c)
def test_list_tables_and_chunk_offsets_at_list_edges(plan, case):
    check_list_tables_and_chunk_offsets(plan, *make_list_plan(*case))


def check_list_tables_and_chunk_offsets(plan, lp, rnd, g):
    W, NH, bounds = lp.W, lp.NH, lp.bounds
    q, want = [], []
    for b in range(W):
        for h in range(NH):
            for a in range(W):
                if a == b:
                    continue
                q.append(("chunk", W, NH, b, h, a, *[int(lp.nw[aa, hh, b]) for hh in range(NH) for aa in range(W)]))
                want.append([lp.hw(b, h, a)])
                q.append(("chunk", W, NH, b, h, a, *[int(lp.cap[hh, aa, b]) for hh in range(NH) for aa in range(W)]))
                want.append([lp.vo(b, h, a)])
    assert plan(q) == want
    # the header-word tables of every slab from its per-(tile, destination) counts
    for a in range(W):
        lo, hi = bounds[a], bounds[a + 1]
        nt = emu.tiles_for(lo, hi - lo)
        tb = emu.region_tiles(lo, hi - lo, g * g, NH, nt)
        t_of = np.arange(lo, hi) // emu.XTILE - lo // emu.XTILE
        hc = np.zeros((nt, W), dtype=np.int64)
        remote = lp.owner[lo:hi] != a
        np.add.at(hc, (t_of[remote], lp.owner[lo:hi][remote]), 1)
        (ok, gw, lwt, nw), = plan([("list_tables", nt, W, NH, *(tb + [nt] * (XMAXH - NH)), *hc.ravel())])
        assert ok == [1, 0, 0]
        assert nw == [int(lp.nw[a, h, d]) for h in range(NH) for d in range(W)]
        words = (hc + 63) // 64
        assert lwt == np.concatenate([np.zeros((nt, 1), dtype=np.int64), np.cumsum(words, axis=1)], axis=1).ravel().tolist()
        # a sender's key in its chunk = 64 * its tile's first header word + its rank in the tile's list
        sel = np.nonzero(remote)[0]
        first = np.array(gw).reshape(nt, W)[t_of[sel], lp.owner[lo:hi][sel]] * 64
        assert np.all(lp.key_local[lo + sel] // 64 * 64 - first < 64 * words[t_of[sel], lp.owner[lo:hi][sel]])
        assert np.all(lp.key_local[lo + sel] >= first)


def layouts(plan, kind, W, NH, bounds, caps, nw, rregions, push):
    """Every rank's XLayout as a dict of lists."""
    names = ("cap_out", "cap_in", "soff", "sbytes", "roff", "rbytes", "ooff", "lhdr", "lval", "rhdr", "rval", "vbase")
    out = []
    for a, res in enumerate(plan([("layout", kind, W, NH, a, rregions, int(push), *bounds, *caps, *nw) for a in range(W)])):
        L = dict(zip(("ok", "send", "recv", "own", "hdr_in", "xr_stride", "xnv"), res[0]))
        L.update(zip(names, res[1:]))
        assert L["ok"] == 1
        out.append(L)
    return out


def disjoint(chunks, total):
    """Chunks (offset, bytes) in one buffer: none overlap, and the last one ends at `total`."""
    chunks = sorted(c for c in chunks if c[1])
    assert all(a[0] + a[1] <= b[0] for a, b in zip(chunks, chunks[1:]))
    assert (chunks[-1][0] + chunks[-1][1] if chunks else 0) == total


@pytest.mark.parametrize("rregions", [1, 4])
def test_list_layout_pairs_every_rank(plan, list_plan, rregions):
    lp = list_plan[0]
    W, NH = lp.W, lp.NH
    caps = [int(lp.cap[h, a, b]) for h in range(NH) for a in range(W) for b in range(W)]
    nw = [int(lp.nw[a, h, b]) for a in range(W) for h in range(NH) for b in range(W)]
    Ls = layouts(plan, 0, W, NH, lp.bounds, caps, nw, rregions, True)
    for a, L in enumerate(Ls):
        i = lambda h, b: h * W + b
        peers = [(h, b) for h in range(NH) for b in range(W) if b != a]
        disjoint([(L["lhdr"][i(h, b)], 16 * int(lp.nw[a, h, b])) for h, b in peers] +
                 [(L["lval"][i(h, b)], 16 * L["cap_out"][i(h, b)]) for h, b in peers], L["send"])
        one = L["hdr_in"] + 16 * sum(L["cap_in"])  # one round parity's receive buffer
        disjoint([(L["rhdr"][i(h, b)], 16 * int(lp.nw[b, h, a])) for h, b in peers] +
                 [(L["rval"][i(h, b)], 16 * L["cap_in"][i(h, b)]) for h, b in peers], one)
        assert L["xr_stride"] == ((one + 255) // 256 * 256 if rregions > 1 else 0)
        assert L["recv"] == (2 * L["xr_stride"] if rregions > 1 else one)
        assert L["xnv"] == max(1, sum(L["cap_in"]))
        for h, b in peers:
            B = Ls[b]
            assert L["cap_out"][i(h, b)] == B["cap_in"][i(h, a)] == int(lp.cap[h, a, b])  # bytes sent = bytes expected
            assert L["rhdr"][i(h, b)] == 16 * lp.hw(a, h, b)
            # a addresses b's vals region where b's own rval puts the chunk
            assert L["vbase"][i(h, b)] == (B["rval"][i(h, a)] - B["hdr_in"]) // 16 == lp.vo(b, h, a)


@pytest.mark.parametrize("kind,push", [(2, True), (1, False), (1, True)])
def test_slot_and_bin_layout_pairs_every_rank(plan, kind, push):
    """Full topology, W = 3 at P = 12289 (slabs of 4096, 4096 and 4097 ids): push-sum's coarse bins,
    and gossip's slot buffers (with and without the vals part)."""
    W, P = 3, 12289
    bounds, _ = emu.slab_bounds(P, 0, "full", W)
    NH = 2 if kind == 2 else 1
    s1 = emu.full_bin_multi_s1(bounds)
    caps = []
    for h in range(NH):
        for a in range(W):
            r0, r1 = emu.full_region(bounds[a + 1] - bounds[a], NH, h)
            for b in range(W):
                caps.append(emu.full_bin_multi_cap(r1 - r0, s1, P) if kind == 2 else
                            0 if a == b else emu.full_capacity(r1 - r0, bounds[b + 1] - bounds[b], P))
    Ls = layouts(plan, kind, W, NH, bounds, caps, [], 1, push)
    nb = [-(-(bounds[b + 1] - bounds[b]) // (1 << s1)) for b in range(W)]
    xbuf = lambda cap: 0 if not cap else 16 + (cap * 4 + 15) // 16 * 16 + (16 * cap if push else 0)
    for a, L in enumerate(Ls):
        disjoint(list(zip(L["soff"], L["sbytes"])), L["send"])
        disjoint(list(zip(L["roff"], L["rbytes"])), L["recv"])
        for h in range(NH):
            for b in range(W):
                i, j = h * W + b, h * W + a
                assert L["cap_out"][i] == Ls[b]["cap_in"][j] == caps[(h * W + a) * W + b]
                want = emu.fb_bins_bytes(nb[b], L["cap_out"][i]) if kind == 2 else xbuf(L["cap_out"][i])
                assert Ls[b]["rbytes"][j] == want  # what b expects from a ...
                assert L["sbytes"][i] == (0 if a == b else want)  # ... is what a sends (own messages do not travel)
        if kind == 2:  # the own share's second parity
            own = [L["rbytes"][h * W + a] for h in range(NH)]
            assert L["ooff"] == [0, own[0]] and L["own"] == sum(own)
            assert (own[0] > 0) == (a == 2)  # a one-tile slab has an empty region 0
    q = [("xbuf", c, int(push)) for c in (0, 1, 4, 5, 1000)]
    assert plan(q) == [[16 + (c * 4 + 15) // 16 * 16, xbuf(c)] for c in (0, 1, 4, 5, 1000)]


def test_bits_layout(plan):
    n = [[0, 5, 1024, 0], [1025, 0, 7, 3000], [1, 2, 0, 3], [0, 0, 0, 0]]
    for me in range(4):
        (head, bo, bn, ro, rn), = plan([("bits", me, 4, *[x for row in n for x in row])])
        pad = lambda x: -(-x // 1024) * 1024
        assert bn == [0 if d == me else n[me][d] for d in range(4)] and rn == [0 if d == me else n[d][me] for d in range(4)]
        disjoint([(bo[d], pad(bn[d])) for d in range(4)], head[1])
        disjoint([(ro[d], pad(rn[d])) for d in range(4)], head[2])
        assert head[0] == 1 and all(x % 1024 == 0 for x in bo + ro)
    (head, *_), = plan([("bits", 0, 2, 0, 2**31 - 1024, 0, 0)])
    assert head[0] == 1
    (head, *_), = plan([("bits", 0, 2, 0, 2**31 - 1023, 0, 0)])
    assert head[0] == 0  # beyond 2^31 bits


@pytest.mark.parametrize("g,W,NR,wx", [(64, 1, 1, 16), (128, 2, 4, 16), (130, 2, 8, 16), (130, 2, 1, 8)])
def test_walk_list_covers_the_slab_once(plan, g, W, NR, wx):
    bounds = imp3d_slabs(g, W)
    for a in range(W):
        lo, nloc = bounds[a], bounds[a + 1] - bounds[a]
        (ok, woff, tiles), = plan([("walk", lo, nloc, g * g, wx, NR)])
        nt = emu.tiles_for(lo, nloc)
        assert ok == [1] and sorted(tiles) == list(range(nt))  # every tile exactly once
        assert len(woff) == 9 * NR and woff[0] == 0 and woff[-1] == nt
        assert all(x <= y for x, y in zip(woff, woff[1:]))  # monotone, regions back to back
        tb = emu.region_tiles(lo, nloc, g * g, NR, nt)
        for h in range(NR):  # launch h visits region h's tiles
            assert sorted(tiles[woff[9 * h]:woff[9 * h + 8]]) == list(range(tb[h], tb[h + 1]))
    (ok, *_), = plan([("walk", 5, 4096, 4096, 16, 1)])
    assert ok == [0]  # not plane-aligned


# ---- the kernel plan (gp_kernel_plan.hpp) against the decisions recorded before the rules moved there
KERNELS = {"tile": 1, "col": 2, "block": 3}  # KernelVariant; any other text: 0
# (name in the golden file, how read_overrides (gp_setup.hip) parses its text)
OVERRIDES = [("GP_KERNEL", lambda t: KERNELS.get(t, 0)), ("GP_XSEGS", lambda t: max(1, int(t))), ("GP_WALK", int),
             ("GP_WX", lambda t: max(1, int(t))), ("GP_WIDE", lambda t: int(t[:1] == "1")), ("GP_RREGIONS", int),
             ("GP_XREGIONS", int), ("GP_FUSE", lambda t: ord(t[0]) - ord("0")), ("GP_STAGE_CAP", lambda t: max(0, int(t))),
             ("GP_NO_FULLTILE", lambda t: int(t[:1] == "1")), ("GP_GRID", str)]
PLAN_FIELDS = ("kernel", "col_xsegs", "walk", "wx", "wide", "grid", "rregions", "fuse_finalize", "stage_cap", "no_full",
               "xregions", "grid_override")


@pytest.fixture(scope="module")
def kernel_plan_golden():
    """The cases of tests/golden/kernel_plan.json as (shape, facts, overrides, decision)."""
    import json
    with open(os.path.join(HERE, "golden", "kernel_plan.json")) as f:
        return [tuple(c) for c in json.load(f)["cases"]]


def test_kernel_plan_replays_the_recorded_decisions(plan, kernel_plan_golden):
    """Every case of tests/golden/kernel_plan.json (recorded from choose_kernel / round_regions as they
    stood in gp_setup.hip, see the file's header): kernel_plan gives the same plan, field for field, or
    the same GP_GRID error; and gather_kernel_facts asks the device exactly what was asked then."""
    cases = kernel_plan_golden
    assert all(set(ov) <= {name for name, _ in OVERRIDES} for _, _, ov, _ in cases)
    q = [("kernel_plan", *shape, *facts, *[parse(ov[name]) if name in ov else "-" for name, parse in OVERRIDES])
         for shape, facts, ov, _ in cases]
    bad = []
    for (shape, facts, ov, want), (err, fields, bplan, asked) in zip(cases, plan(q)):
        got = "GP_GRID=%s: not a grid of 1..%d blocks" % (ov["GP_GRID"], err[1]) if err[0] else fields + bplan + asked
        if got != want:
            bad.append((shape, facts, ov, want, got))
    assert not bad, "%d of %d cases differ, the first: %r" % (len(bad), len(cases), bad[0])


def test_kernel_plan_golden_holds_the_cases_where_a_rule_flips(kernel_plan_golden):
    """The sweep crosses every threshold of the rules (both sides present among the recorded decisions)."""
    ok = [(s, f, ov, dict(zip(PLAN_FIELDS, w))) for s, f, ov, w in kernel_plan_golden if not isinstance(w, str)]

    def seen(pred):
        return {key for c in ok for key in [pred(*c)] if key is not None}
    # gossip on a 3D / Imp3D lattice at g = 199 / 200: tile / column
    assert seen(lambda s, f, ov, w: (s[0], s[3], w["kernel"]) if s[1] == 0 and s[3] in (199, 200) and not ov else None) == \
        {(2, 199, 1), (2, 200, 2), (3, 199, 1), (3, 200, 2)}
    # g / world = 63 / 64: walk 0 / walks 2 (gossip) and 3 (push-sum)
    assert seen(lambda s, f, ov, w: (s[3] // s[4], s[1], w["walk"]) if s[0] == 3 and s[3] // s[4] in (63, 64) and not ov
                and f[2] >= 8 else None) == {(63, 0, 0), (63, 1, 0), (64, 0, 2), (64, 1, 3)}
    # walk 3 with 7 / 8 resident blocks: back to walk 2 (one CU: the 64-per-CU cap) / the resident grid
    assert seen(lambda s, f, ov, w: (f[2], w["walk"], w["grid"]) if s[:2] == [3, 1] and s[3] // s[4] == 64 and f[2] in (7, 8)
                and not ov else None) == {(7, 2, 64), (8, 3, 8)}
    # the wide class up to two tiles per resident block (line push-sum, 256 CUs: 2560 tiles)
    assert seen(lambda s, f, ov, w: (-(-s[2] // 1024) + 1, w["wide"]) if s[:2] == [0, 1] and s[4] == 1 and f[2] == 1280
                and s[2] > 10**6 and not ov else None) == {(2560, 1), (2561, 0)}
    # a 3D push-sum lattice with / without a resident box grid
    assert seen(lambda s, f, ov, w: (f[4], w["kernel"]) if s[:2] == [2, 1] and s[3:5] == [100, 1] and f[0] == 256 and not ov
                else None) == {(0, 1), (1, 3)}
    # Imp3D push-sum at W = 2, slabs below / from RREG_MIN_NODES on: one launch per round / eight regions
    assert seen(lambda s, f, ov, w: (s[3], w["rregions"]) if s[:2] == [3, 1] and s[3] in (322, 323) and s[4] == 2 and not ov
                else None) == {(322, 1), (323, 8)}
    # a GP_GRID that region rounds ignore still marks the name
    assert seen(lambda s, f, ov, w: (w["grid"] == 12, w["grid_override"]) if w["rregions"] > 1 and ov.get("GP_GRID") == "12"
                else None) == {(False, 1)}
    errors = {ov["GP_GRID"] for _, _, ov, w in kernel_plan_golden if isinstance(w, str)}
    assert {"abc", "0", "-8", "8x", "99999999999999999999", "41"} <= errors


# ---- the exchange kind (exchange_kind, gp_kernel_plan.hpp): XKind's integers
X_NONE, X_LISTS, X_BITS, X_SLOTS, X_BINS = range(5)
# (topology, algorithm): the kind for world > 1 by kernel variant (tile, col, block); world 1: none
EXCHANGE_KINDS = {
    ("line", "gossip"): (X_NONE, X_NONE, X_NONE),
    ("line", "push-sum"): (X_NONE, X_NONE, X_NONE),
    ("full", "gossip"): (X_SLOTS, X_SLOTS, X_SLOTS),
    ("full", "push-sum"): (X_BINS, X_BINS, X_BINS),
    ("3D", "gossip"): (X_NONE, X_NONE, X_NONE),
    ("3D", "push-sum"): (X_NONE, X_NONE, X_NONE),
    ("Imp3D", "gossip"): (X_SLOTS, X_BITS, X_SLOTS),
    ("Imp3D", "push-sum"): (X_LISTS, X_LISTS, X_LISTS),
}


def test_exchange_kind_table(plan):
    """One exchange kind per run: every topology x algorithm x world in {1, 2, 16} x kernel variant.
    Halo-only runs and single ranks exchange nothing; only Imp3D gossip depends on the kernel (the
    column kernel sets bits, the tile kernel reads in-edge tags)."""
    topos = {"line": 0, "full": 1, "3D": 2, "Imp3D": 3}
    algs = {"gossip": 0, "push-sum": 1}
    cases = [(t, a, W, k) for t in topos for a in algs for W in (1, 2, 16) for k in ("tile", "col", "block")]
    assert len(cases) == 4 * 2 * 3 * 3
    got = plan([("xkind", topos[t], algs[a], W, KERNELS[k]) for t, a, W, k in cases])
    for (t, a, W, k), (kind,) in zip(cases, got):
        want = X_NONE if W == 1 else EXCHANGE_KINDS[t, a][("tile", "col", "block").index(k)]
        assert kind == want, (t, a, W, k, kind, want)
