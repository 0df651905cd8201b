// gp_plan.hpp -- the plan of a run over several ranks: slab bounds, exchange regions, message
// capacities, the byte layout of every send and receive buffer, the lists' header-word tables
// and the bitmaps' chunk offsets -- the integer and double arithmetic that decides what the host
// units allocate and the kernels address (gp_setup.hip, gp_topology.hip, gp_xlayout.hip,
// gp_exchange.hip).  Host-only and free of HIP headers, like gp_block_plan.hpp, so that a plain
// C++ program can evaluate it (tests/helpers/plan_check.cpp): tests/test_plan.py compares it with
// the restatements in tests/multirank_emu.py that the GPU edge tests derive their cases from.
// Which round kernel, walk and grid the run gets is decided beside it, in gp_kernel_plan.hpp.
// The experiments build's GP_* overrides (ExpOverrides, gp_host.hpp) are applied to this plan's
// results by the host units.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace gp {

// ---- the constants the plan is bounded by
constexpr int XMAXW = 16;          // ranks supported by the exchange (one node: 8 GPUs)
constexpr int XMAXH = 8;           // exchange regions of a slab (push-sum), at most
constexpr uint32_t XTILE = 1024;   // the lists' tiles: the tiled round kernels' TILE (gp_internal.hpp)
constexpr uint32_t HALO_CHUNK = 1024;  // nodes per chunk of a compacted halo plane (HaloArgs, gp_xchg.hpp)
constexpr int RREG_MAX = 8;        // round kernel launches per round, at most (DevState::rregions)
constexpr int XREGIONS = 4;        // Imp3D push-sum exchange regions (see exchange_regions)
constexpr uint32_t RREG_MIN_NODES = 1u << 24;  // region rounds from this slab size on (round_regions_ok)
constexpr uint32_t BITS_ALIGN = 1024;  // bitmap chunks start on 128-byte boundaries

// full-topology push-sum (gp_fullbin.hip).  Fine tile = 2^FB_TB receivers (one fold block); 4096
// (measured: 10 / 11 / 12 -> 3.65 / 3.63 / 3.60 ms at P = 1e8)
constexpr int FB_TB = 12;
// messages per fine tile: expected 2^FB_TB + 12 sigma + 128 (4992 at 4096 receivers)
constexpr int FB_CAP2 = ((1 << FB_TB) + 12 * (1 << (FB_TB / 2)) * (FB_TB % 2 ? 1414 : 1000) / 1000 + 128 + 63) / 64 * 64;
// one rank: slots past the last coarse bin (hdr1 / pay1) that the fused fold's write-out sends
// its lanes without a message to, so that every thread issues the same stores (k_fb_fold)
constexpr size_t FB_JUNK = 64;
constexpr int FB_REGIONS = 2;         // exchange regions of a slab (full push-sum)
constexpr int FB_MAXBINS = 4096;      // LDS counters of the send pass and the split
constexpr uint32_t FBF_MAXB1 = 1024;  // keys (coarse bins) the fold's send phase can bin into (LDS reservation slots)
// Several ranks: all ranks' coarse bins together, at most -- about the one-rank fused fold's 191
// bins at C4, whose runs (~21 messages per (tile, key)) measured best there; larger bins also
// carry less 12-sigma padding through the exchange (C4 at W = 8: 2^19 receivers, 24 bins per
// rank, +6.8 %).
constexpr uint32_t FBM_KEYS = 192;

static_assert(XMAXH >= 8 && RREG_MAX >= 8, "eight regions for two ranks");

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- slab bounds and halo width
// 3D / Imp3D: whole x-planes (Program.fs:246-257 id = x g^2 + y g + z); line and the full
// topology: contiguous ids (full: no halo, every message goes through the exchange).
enum class SlabCut { Line, Full, Planes };
enum class BoundsError { None, TooManyRanks, FewerNodesThanRanks, FewerPlanesThanRanks };

inline BoundsError slab_bounds(int64_t P, int64_t g, int W, SlabCut cut, std::vector<uint32_t>& bounds, uint32_t& halo) {
    bounds.assign(W + 1, 0);
    halo = 0;
    if (W == 1) {
        bounds[1] = (uint32_t)P;
        return BoundsError::None;
    }
    if (W > XMAXW) return BoundsError::TooManyRanks;
    if (cut == SlabCut::Planes) {
        if (g < W) return BoundsError::FewerPlanesThanRanks;
        for (int w = 0; w <= W; ++w) bounds[w] = (uint32_t)((g * w / W) * g * g);
        halo = (uint32_t)(g * g);
    } else {
        if (P < W) return BoundsError::FewerNodesThanRanks;
        for (int w = 0; w <= W; ++w) bounds[w] = (uint32_t)(P * w / W);
        halo = cut == SlabCut::Line ? 1u : 0u;
    }
    return BoundsError::None;
}

// ---- tiles and regions
// Tiles covering the ids [lo, lo + nloc) (tiles sit on global multiples of XTILE).
inline uint32_t tiles_for(uint32_t lo, uint32_t nloc) {
    return (uint32_t)(((uint64_t)lo + nloc + XTILE - 1) / XTILE - lo / XTILE);
}

// First plane (relative to the slab's) of region h of NR equal regions over nx planes.  (A last
// region half the size of the others measured within noise, profiles/r05/rejected/rlast.txt.)
inline uint32_t region_plane(uint32_t nx, int NR, int h) {
    if (h >= NR) return nx;
    return (uint32_t)((uint64_t)nx * h / NR);
}

// A plane-aligned slab [lo, lo + nloc) in tiles and planes: a tile belongs to the plane it
// starts in (the slab's first tile to the first plane).
struct PlaneSlab {
    uint64_t g2;
    uint32_t tb, tend;  // its tiles [tb, tend), global
    uint32_t x0, nx;    // its planes [x0, x0 + nx)
    bool init(uint32_t lo, uint32_t nloc, uint64_t g2_) {  // false if the slab is not plane-aligned
        if (!g2_ || nloc % g2_ || lo % g2_) return false;
        g2 = g2_;
        tb = lo / XTILE;
        tend = (uint32_t)(((uint64_t)lo + nloc + XTILE - 1) / XTILE);
        x0 = (uint32_t)(lo / g2);
        nx = (uint32_t)(nloc / g2);
        return true;
    }
    uint32_t first(uint64_t x) const {  // first tile (global) of plane x
        return x <= x0 ? tb : (uint32_t)std::min<uint64_t>((x * g2 + XTILE - 1) / XTILE, tend);
    }
};

// Region h of NR of a plane-aligned slab: planes [x0 + region_plane(h), x0 + region_plane(h + 1)),
// whose tiles (relative to lo / XTILE) are [rb[h], rb[h + 1]).  False if the slab is not
// plane-aligned.
inline bool region_tiles(uint32_t lo, uint32_t nloc, uint64_t g2, int NR, uint32_t* rb) {
    PlaneSlab s;
    if (NR < 1 || !s.init(lo, nloc, g2)) return false;
    for (int h = 0; h <= NR; ++h) rb[h] = s.first((uint64_t)s.x0 + region_plane(s.nx, NR, h)) - s.tb;
    return true;
}

// The lists' regions of a slab, tb[0 .. XMAXH]: whole planes (region_tiles: the round kernel's
// regions when it runs region by region), else equal tile counts; entries past NH: the slab's end.
inline void list_region_tiles(uint32_t lo, uint32_t nloc, uint64_t g2, int NH, uint32_t* tb) {
    const uint32_t nt = tiles_for(lo, nloc);
    if (!region_tiles(lo, nloc, g2, NH, tb))
        for (int h = 0; h <= NH; ++h) tb[h] = (uint32_t)((uint64_t)nt * h / NH);
    for (int h = NH + 1; h <= XMAXH; ++h) tb[h] = nt;
}

// Full-topology push-sum over several ranks: region h of NH of a slab is its fine tiles
// [t0, t1) (2^FB_TB local ids each, counted from lo) -- the fold of those tiles bins their
// next-round messages into region h's exchange buffers -- whose senders are the local ids
// [s0, s1).
inline void full_region(uint32_t nloc, int NH, int h, uint32_t& t0, uint32_t& t1, uint32_t& s0, uint32_t& s1) {
    const uint32_t nt = (uint32_t)(((uint64_t)nloc + (1u << FB_TB) - 1) >> FB_TB);
    t0 = (uint32_t)((uint64_t)nt * h / NH);
    t1 = (uint32_t)((uint64_t)nt * (h + 1) / NH);
    s0 = (uint32_t)std::min<uint64_t>(nloc, (uint64_t)t0 << FB_TB);
    s1 = (uint32_t)std::min<uint64_t>(nloc, (uint64_t)t1 << FB_TB);
}

// Local sender ids [s_lo, s_hi) of region h of an Imp3D slab: with lists the tiles
// [tb[h], tb[h + 1]), else the slab's halves.
inline void xregion(uint32_t lo, uint32_t nloc, bool lists, const uint32_t* tb, int NH, int h, uint32_t& s_lo,
                    uint32_t& s_hi) {
    if (lists) {
        auto at = [&](uint32_t t) {
            const int64_t b = (int64_t)(lo / XTILE + t) * XTILE - lo;
            return (uint32_t)std::min<int64_t>(nloc, std::max<int64_t>(0, b));
        };
        s_lo = at(tb[h]);
        s_hi = h + 1 == NH ? nloc : at(tb[h + 1]);
        return;
    }
    const uint32_t split = nloc / 2;
    s_lo = NH == 1 || h == 0 ? 0u : split;
    s_hi = NH == 1 || h == 1 ? nloc : split;
}

// Exchange regions of a slab's senders: push-sum runs several (one's transfer overlaps the
// others' packing), gossip one.  Imp3D push-sum cuts them at a tile boundary (the lists'
// tiles): XREGIONS regions of the slab's tiles (the last one's transfer is what the round cannot
// hide); the full topology at a fine-tile boundary (full_region), its two halves.  Two ranks with
// large slabs: eight regions, where one link carries half of every rank's messages -- C5, region
// rounds, same box (profiles/r05/rregions/reg8.txt): W = 2 10.72 -> 10.21 ms at 128 GB/s,
// 12.53 -> 11.50 at 64; at W = 4 and 8 eight were slower (5.50 -> 5.69, 2.82 -> 3.00 ms at
// 128 GB/s).
inline int exchange_regions(bool push, bool imp3d, int W, const std::vector<uint32_t>& bounds) {
    if (!push) return 1;
    if (imp3d && W == 2 && bounds.size() == 3 && std::min(bounds[1] - bounds[0], bounds[2] - bounds[1]) >= RREG_MIN_NODES)
        return 8;
    return imp3d ? XREGIONS : FB_REGIONS;
}

// Imp3D push-sum across ranks with NH exchange regions: may the round kernel run region by
// region (DevState::rregions = NH)?  `on`: every slab holds at least RREG_MIN_NODES nodes (small
// slabs move little and keep one launch per round; see round_regions, gp_kernel_plan.hpp).
inline bool round_regions_on(int W, const std::vector<uint32_t>& bounds) {
    for (int w = 0; w < W; ++w)
        if (bounds[w + 1] - bounds[w] < RREG_MIN_NODES) return false;
    return true;
}
inline bool round_regions_fit(int W, const std::vector<uint32_t>& bounds, uint64_t g2, int NH) {
    if (NH < 2 || NH > RREG_MAX) return false;
    uint32_t rb[RREG_MAX + 1];
    for (int w = 0; w < W; ++w)
        if (!region_tiles(bounds[w], bounds[w + 1] - bounds[w], g2, NH, rb)) return false;
    return true;
}

// ---- walk 3's visiting order (host, at create): walk 2's items (TileWalk, gp_tile.hpp) for each
// of the 8 XCDs, empty items dropped -- every tile of the slab exactly once.
// list: tiles relative to lo / XTILE; woff[0][c]..woff[0][c + 1]: XCD c's items.
// NR > 1 (launch_round_regions): the planes of region h (region_tiles) dealt to the
// 8 XCDs in the same way, XCD c's items at woff[h][c]..woff[h][c + 1].  wx: planes per x-window.
inline bool build_walk_list(uint32_t lo, uint32_t nloc, uint64_t g2, uint32_t wx, int NR, std::vector<uint32_t>& list,
                            uint32_t woff[][9]) {
    PlaneSlab s;
    if (NR < 1 || NR > RREG_MAX || !s.init(lo, nloc, g2)) return false;
    const uint32_t kp = (uint32_t)((g2 + XTILE - 1) / XTILE + 1);
    list.clear();
    for (int h = 0; h < NR; ++h) {
        const uint32_t r0 = s.x0 + region_plane(s.nx, NR, h);
        const uint32_t nr = s.x0 + region_plane(s.nx, NR, h + 1) - r0;
        for (uint32_t c = 0; c < 8; ++c) {
            woff[h][c] = (uint32_t)list.size();
            const uint32_t xa = r0 + (uint32_t)((uint64_t)nr * c / 8);
            const uint32_t nxa = r0 + (uint32_t)((uint64_t)nr * (c + 1) / 8) - xa;
            uint32_t nwin = wx ? (nxa + wx - 1) / wx : 1u;
            if (nwin == 0) nwin = 1;
            for (uint32_t v = 0; v < nwin && nxa; ++v) {
                const uint32_t xs = (uint32_t)((uint64_t)nxa * v / nwin), xe = (uint32_t)((uint64_t)nxa * (v + 1) / nwin);
                for (uint32_t k = 0; k < kp; ++k)
                    for (uint32_t x = xa + xs; x < xa + xe; ++x) {
                        const uint32_t ti = s.first(x) + k;
                        if (ti < s.first(x + 1)) list.push_back(ti - s.tb);
                    }
            }
        }
        woff[h][8] = (uint32_t)list.size();
    }
    return list.size() == (size_t)(s.tend - s.tb);
}

// ---- capacities
// Fixed message capacity of an exchange buffer: the expected messages per round m + 12 sigma
// + 64, never more than `limit` (the senders or edges that could fill it).
inline uint32_t msg_capacity(double m, double limit) {
    return (uint32_t)std::min(std::ceil(m + 12.0 * std::sqrt(m) + 64.0), limit);
}

// Full-topology gossip: messages a -> b are at most Binomial(na, nb / (P - 1)).
inline uint32_t full_pair_cap(uint32_t na, uint32_t nb, uint32_t P) {
    return msg_capacity((double)na * (double)nb / (double)(P - 1), (double)na);
}

struct FullBinPlan {
    uint32_t s1;    // coarse bin = target >> s1
    uint32_t nb1;   // coarse bins
    uint32_t nb2;   // fine tiles
    uint32_t cap1;  // message capacity per coarse bin
    uint32_t cap2;  // message capacity per fine tile
};

// Full-topology push-sum: bins for the nrecv receivers of a rank (one rank: nrecv = P).
// fused: one rank, the fold bins the next round.
inline FullBinPlan full_bin_plan(uint32_t P, bool fused) {
    FullBinPlan p{};
    uint32_t bits = 1;
    while (bits < 32 && ((uint64_t)1 << bits) < P) ++bits;
    // coarse bins ~ sqrt(P / TILE) so both passes write runs of ~10-20 messages;
    // at most FB_MAXBINS coarse bins and FB_MAXBINS fine tiles per coarse bin.  The
    // fused fold (one rank) takes coarse bins half that size: the split's runs get
    // longer and the fold's shorter; P = 1e8, same box: rule 3.37, -1 3.26, -2 3.25,
    // -3 3.38-3.40 ms/round (profiles/r04/c4_fused/s1_sweep.txt)
    uint32_t s1 = (bits + FB_TB + 1) / 2 - (fused ? 1u : 0u);
    if (s1 < FB_TB) s1 = FB_TB;
    while (((uint64_t)P >> s1) >= FB_MAXBINS) ++s1;
    while (fused && (((uint64_t)P + (1ull << s1) - 1) >> s1) > FBF_MAXB1) ++s1;
    while (s1 - FB_TB > 12) --s1;
    p.s1 = s1;
    p.nb1 = (uint32_t)(((uint64_t)P + (1ull << s1) - 1) >> s1);
    p.nb2 = (uint32_t)(((uint64_t)P + (1u << FB_TB) - 1) >> FB_TB);
    const double m1 = (double)(1ull << s1) * ((double)P / (double)(P > 1 ? P - 1 : 1));
    p.cap1 = (uint32_t)(m1 + 12.0 * std::sqrt(m1) + 1024.0);
    p.cap2 = FB_CAP2;
    return p;
}

// Several ranks: the coarse-bin shift every rank uses -- the smallest size (>= a fine tile) that
// keeps the keys of all ranks' bins together at most FBM_KEYS (within the fold's LDS reservation
// slots).
inline uint32_t full_bin_multi_s1(const uint32_t* bounds, int W) {
    uint32_t s1 = FB_TB;
    for (;; ++s1) {
        uint64_t keys = 0;
        for (int b = 0; b < W; ++b) keys += ((uint64_t)(bounds[b + 1] - bounds[b]) + (1ull << s1) - 1) >> s1;
        if (keys <= FBM_KEYS || s1 - FB_TB >= 12) break;
    }
    return s1;
}

// Several ranks: the per-bin capacity of the messages a region of n senders sends to one
// rank's coarse bin (2^s1 receivers; a rank's messages to itself included, they pass through its
// own receive buffer): at most Binomial(n, 2^s1 / (P - 1)).
inline uint32_t full_bin_multi_cap(uint32_t n, uint32_t s1, uint32_t P) {
    return msg_capacity((double)n * (double)(1ull << s1) / (double)(P > 1 ? P - 1 : 1), (double)n);
}

// Coarse bins of rank p's receivers, 2^s1 each (full push-sum over several ranks, FbBins).
inline uint32_t full_coarse_bins(const std::vector<uint32_t>& bounds, int p, uint32_t s1) {
    return (uint32_t)(((uint64_t)bounds[p + 1] - bounds[p] + (1ull << s1) - 1) >> s1);
}

// Slots per HALO_CHUNK-node chunk of a slab-boundary plane (HaloArgs): the senders toward one x
// neighbour in a chunk are a sum of Bernoulli(1 / deg) over its nodes (Program.fs:246-260: a
// boundary plane's nodes have both x neighbours, y / z ones unless on the lattice's edge, and
// Imp3D's random edge); the largest mean + 12 sigma over the plane's chunks, rounded up to 8.
// g = 1000: 3D 360 (the chunk of row y = 0), Imp3D 320.
inline uint32_t halo_chunk_cap(uint32_t g, bool imp3d) {
    const uint64_t n = (uint64_t)g * g;
    double best = 0.0, mu = 0.0, var = 0.0;
    for (uint64_t i = 0; i <= n; ++i) {
        if (i == n || (i % HALO_CHUNK == 0 && i > 0)) {
            best = std::max(best, mu + 12.0 * std::sqrt(var));
            mu = var = 0.0;
            if (i == n) break;
        }
        const uint32_t y = (uint32_t)(i / g), z = (uint32_t)(i % g);
        const uint32_t deg = 2u + (y > 0) + (y + 1 < g) + (z > 0) + (z + 1 < g) + (imp3d ? 1u : 0u);
        const double p = 1.0 / deg;
        mu += p;
        var += p * (1.0 - p);
    }
    const uint32_t c = (uint32_t)std::ceil(best);
    return std::min<uint32_t>(HALO_CHUNK, std::max<uint32_t>(8u, (c + 7u) & ~7u));
}
inline size_t halo_buf_slots(uint32_t n, uint32_t cap) { return (size_t)((n + HALO_CHUNK - 1) / HALO_CHUNK) * cap; }

// ---- buffer shapes
// One rank pair's slot buffer (XPeer, gp_xchg.hpp): [count u32 | pad to 16 B][slots: cap u32 |
// pad][vals: cap (s, w), with `push` only -- no run asks for it: the slot buffers carry gossip
// alone since push-sum went to lists and bins, and setup_exchange passes push = false].
constexpr size_t XBUF_SLOTS_OFF = 16;
inline size_t xbuf_vals_off(uint32_t cap) { return XBUF_SLOTS_OFF + align16((size_t)cap * 4); }
inline size_t xbuf_bytes(uint32_t cap, bool push) { return cap ? xbuf_vals_off(cap) + (push ? (size_t)cap * 16 : 0) : 0; }

// A set of nb coarse bins of cap messages each (FbBins, gp_fullbin.hpp): [counts: nb u32 | pad]
// [sender ids: nb * cap u32 | pad][payloads: nb * cap (s / 2, w / 2)].
inline size_t fb_bins_hdr_off(uint32_t nb) { return align16((size_t)nb * 4); }
inline size_t fb_bins_pay_off(uint32_t nb, uint32_t cap) { return fb_bins_hdr_off(nb) + align16((size_t)nb * cap * 4); }
inline size_t fb_bins_bytes(uint32_t nb, uint32_t cap) {
    return nb && cap ? fb_bins_pay_off(nb, cap) + (size_t)nb * cap * 16 : 0;
}

// Offset of chunk (h, a) in rank b's receive buffer, in units of size(hh, aa): the chunks lie
// in (h, a) order, a != b (every rank lays out its receive buffer this way, and every sender
// addresses it this way).  Header words: list_hw; slots of the vals region: exchange_layout.
template <typename F>
uint64_t chunk_offset(int W, int NH, int b, int h, int a, F size) {
    uint64_t o = 0;
    for (int hh = 0; hh < NH; ++hh)
        for (int aa = 0; aa < W; ++aa) {
            if (aa == b) continue;
            if (hh == h && aa == a) return o;
            o += size(hh, aa);
        }
    return o;
}

// ---- Imp3D push-sum lists (gp_xchg.hpp).  list_nw[(a * NH + h) * W + b]: header words of chunk
// (h, a -> b), every slab's.
// First header word of chunk (h, a) in rank b's header region.
inline uint32_t list_hw(const std::vector<uint32_t>& list_nw, int W, int NH, int b, int h, int a) {
    return (uint32_t)chunk_offset(W, NH, b, h, a, [&](int hh, int aa) { return list_nw[((size_t)aa * NH + hh) * W + b]; });
}

// One slab's list tables from hc[tile * W + d], its list entries per (tile, destination), and
// its region boundaries tb: gw[tile * W + d], the first header word of the tile's segment in
// chunk (region, d); lwt[tile * (W + 1) + d], the prefix over d of the tile's segments' words
// (<= 16 + W); nw[h * W + d], the header words of chunk (h, d) -- the slab's row of list_nw.
// False if a chunk reaches 2^26 header words: that destination and its word count in bad_d /
// bad_words.
inline bool list_tables(const std::vector<uint32_t>& hc, uint32_t nt, int W, int NH, const uint32_t* tb,
                        std::vector<uint32_t>& gw, std::vector<uint8_t>& lwt, uint32_t* nw, int& bad_d,
                        uint64_t& bad_words) {
    gw.assign((size_t)nt * W, 0);
    lwt.assign((size_t)nt * (W + 1), 0);
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t w = 0;
        for (int d = 0; d < W; ++d) {
            lwt[(size_t)t * (W + 1) + d] = (uint8_t)w;
            w += (hc[(size_t)t * W + d] + 63u) / 64u;
        }
        lwt[(size_t)t * (W + 1) + W] = (uint8_t)w;
    }
    for (int d = 0; d < W; ++d) {
        uint64_t run[XMAXH] = {};
        for (uint32_t t = 0, h = 0; t < nt; ++t) {
            while ((int)h + 1 < NH && t >= tb[h + 1]) ++h;
            gw[(size_t)t * W + d] = (uint32_t)run[h];
            run[h] += (hc[(size_t)t * W + d] + 63u) / 64u;
        }
        for (int h = 0; h < NH; ++h) {
            if (run[h] >= (1ull << 26)) {
                bad_d = d;
                bad_words = run[h];
                return false;
            }
            nw[(size_t)h * W + d] = (uint32_t)run[h];
        }
    }
    return true;
}

// ---- Imp3D gossip bitmaps (gp_xchg.hpp): rank `me`'s chunks from the edge counts n[a][b]
// (edges a -> b), each chunk padded to BITS_ALIGN bits.
struct BitsLayout {
    std::vector<uint32_t> bo, bn, ro, rn;  // [peer]: chunk bit offset / bits, send and receive side
    uint32_t nbits_out = 0, nbits_in = 0;  // bitmap sizes (multiples of BITS_ALIGN)
};
inline bool bits_layout(const std::vector<std::vector<uint32_t>>& n, int me, BitsLayout& L) {  // false: beyond 2^31 bits
    const int W = (int)n.size();
    auto pad = [](uint64_t x) { return (x + BITS_ALIGN - 1) / BITS_ALIGN * BITS_ALIGN; };
    L.bo.assign(W, 0);
    L.bn.assign(W, 0);
    L.ro.assign(W, 0);
    L.rn.assign(W, 0);
    uint64_t so = 0, ri = 0;
    for (int d = 0; d < W; ++d) {
        if (d == me) continue;
        L.bo[d] = (uint32_t)so;
        L.bn[d] = n[me][d];
        so += pad(n[me][d]);
        L.ro[d] = (uint32_t)ri;
        L.rn[d] = n[d][me];
        ri += pad(n[d][me]);
    }
    if (so >= (1ull << 31) || ri >= (1ull << 31)) return false;
    L.nbits_out = (uint32_t)so;
    L.nbits_in = (uint32_t)ri;
    return true;
}

// ---- the exchange buffers of one rank.  Index [h * W + b]: region h, peer b.
struct XLayout {
    std::vector<uint32_t> cap_out, cap_in;  // message capacity of the buffer to / from rank b
    size_t send_bytes = 0, recv_bytes = 0;  // xsend / xrecv
    // slot buffers (gossip) and coarse bins (full push-sum): byte offset and size of each buffer
    std::vector<size_t> soff, sbytes, roff, rbytes;
    // full push-sum: the own share's second parity (Slab::xown), region h's at ooff[h]
    size_t ooff[FB_REGIONS] = {};
    size_t own_bytes = 0;
    // Imp3D push-sum lists
    std::vector<size_t> lhdr, lval;  // send buffer: byte offsets of chunk (h, d)'s header words / slots
    std::vector<size_t> rhdr, rval;  // receive buffer: byte offsets of chunk (h, p)'s header words / slots
    std::vector<uint32_t> vbase;     // index of my chunk's first slot in d's vals region
    size_t hdr_in = 0;               // bytes of the receive buffer's header region (the vals region follows)
    size_t xr_stride = 0;            // the receive buffer of odd rounds at xrecv + xr_stride (region-by-region
                                     // rounds: the next round's lists arrive during this one), else 0
    uint32_t xnv = 0;                // message slots in the vals region (at least 1)
};

// The form in which a run's random-edge / full-topology messages cross ranks, decided once per run
// (exchange_kind, gp_kernel_plan.hpp -> KernelPlan::xkind):
//   None      one rank, and line / 3D at any world: halo planes only
//   Lists     Imp3D push-sum: sender-ordered lists, read in place (k_list_pack)
//   Bits      Imp3D gossip on the column kernel: one bit per remote edge (k_gossip_col, k_apply_bits)
//   Slots     Imp3D gossip on the tile kernel (k_pack / k_unpack) and full gossip (gp_full.hip):
//             in-edge slots / receiver ids in per-pair buffers with an in-band count
//   FullBins  full push-sum: every destination's coarse bins (gp_fullbin.hip)
enum class XKind { None, Lists, Bits, Slots, FullBins };

// Rank a's layout from caps[(h * W + a) * W + b], the capacity of region h's buffer a -> b
// (every rank's); kind: Lists, Slots or FullBins (None and Bits have no such buffers).  Lists:
// list_nw; rregions > 1: one receive buffer per round parity.  Slots: push adds the vals part
// (xbuf_bytes; unused by the runs).  FullBins: the coarse bins of every destination, 2^s1
// receivers each (bounds, full_bin_multi_s1).  False (lists): a vals region beyond 2^32 slots.
inline bool exchange_layout(XKind kind, const std::vector<uint32_t>& caps, const std::vector<uint32_t>& list_nw,
                            const std::vector<uint32_t>& bounds, int W, int NH, int a, uint32_t rregions, bool push,
                            XLayout& L) {
    auto cap = [&](int h, int s, int d) { return caps[((size_t)h * W + s) * W + d]; };
    const size_t R = (size_t)NH * W;
    L = XLayout{};
    L.cap_out.assign(R, 0);
    L.cap_in.assign(R, 0);
    if (kind == XKind::Lists) {
        auto nw = [&](int h, int s, int d) { return list_nw[((size_t)s * NH + h) * W + d]; };
        // slot offset of chunk (h, s) in rank d's vals region (the order of list_hw)
        auto vo = [&](int d, int h, int s) {
            return chunk_offset(W, NH, d, h, s, [&](int hh, int ss) { return cap(hh, ss, d); });
        };
        L.lhdr.assign(R, 0);
        L.lval.assign(R, 0);
        L.rhdr.assign(R, 0);
        L.rval.assign(R, 0);
        L.vbase.assign(R, 0);
        size_t so = 0, hdr_in = 0;
        uint64_t nv_in = 0;
        for (int h = 0; h < NH; ++h)
            for (int b = 0; b < W; ++b) {
                if (b == a) continue;
                const size_t i = (size_t)h * W + b;
                L.cap_out[i] = cap(h, a, b);
                L.cap_in[i] = cap(h, b, a);
                L.lhdr[i] = so;
                so += (size_t)nw(h, a, b) * 16;
                L.lval[i] = so;
                so += (size_t)L.cap_out[i] * 16;
                L.rhdr[i] = (size_t)list_hw(list_nw, W, NH, a, h, b) * 16;
                hdr_in += (size_t)nw(h, b, a) * 16;
                nv_in += L.cap_in[i];
                const uint64_t vb = vo(b, h, a);
                if (vb >= (1ull << 32) || nv_in >= (1ull << 32)) return false;
                L.vbase[i] = (uint32_t)vb;
            }
        for (int h = 0; h < NH; ++h)
            for (int b = 0; b < W; ++b)
                if (b != a) L.rval[(size_t)h * W + b] = hdr_in + (size_t)vo(a, h, b) * 16;
        const size_t ro = hdr_in + (size_t)nv_in * 16;
        L.xr_stride = rregions > 1 ? (ro + 255) & ~(size_t)255 : 0;
        L.send_bytes = so;
        L.recv_bytes = L.xr_stride ? 2 * L.xr_stride : ro;
        L.hdr_in = hdr_in;
        L.xnv = (uint32_t)std::max<uint64_t>(1, nv_in);
        return true;
    }
    const bool bins = kind == XKind::FullBins;
    const uint32_t fs1 = bins ? full_bin_multi_s1(bounds.data(), W) : 0;
    L.soff.assign(R, 0);
    L.sbytes.assign(R, 0);
    L.roff.assign(R, 0);
    L.rbytes.assign(R, 0);
    size_t so = 0, ro = 0;
    for (int h = 0; h < NH; ++h)
        for (int b = 0; b < W; ++b) {
            const size_t i = (size_t)h * W + b;
            L.cap_out[i] = cap(h, a, b);
            L.cap_in[i] = cap(h, b, a);
            L.soff[i] = so;
            // (own messages: straight to xrecv; full push-sum: b's coarse bins, FbBins)
            L.sbytes[i] = b == a ? 0
                          : bins ? fb_bins_bytes(full_coarse_bins(bounds, b, fs1), L.cap_out[i])
                                 : xbuf_bytes(L.cap_out[i], push);
            so += L.sbytes[i];
            L.roff[i] = ro;
            L.rbytes[i] = bins ? fb_bins_bytes(full_coarse_bins(bounds, a, fs1), L.cap_in[i]) : xbuf_bytes(L.cap_in[i], push);
            ro += L.rbytes[i];
        }
    L.send_bytes = so;
    L.recv_bytes = ro;
    if (bins)
        for (int h = 0; h < NH && h < FB_REGIONS; ++h) {
            L.ooff[h] = L.own_bytes;
            L.own_bytes += L.rbytes[(size_t)h * W + a];
        }
    return true;
}

}  // namespace gp
