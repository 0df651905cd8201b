// gp_setup.hip -- everything a simulation needs before round 0 (create_common / build_sim): the
// slab plan and kernel choice, every slab's device state, the Imp3D topology build (in-lists;
// random-edge lists / bitmaps / slots across ranks) and the exchange-buffer layout.
#include "gp_host.hpp"

// Full-topology push-sum over several ranks: region h of NH of a slab is its fine tiles
// [t0, t1) (2^FB_TB local ids each, counted from lo) -- the fold of those tiles bins their
// next-round messages into region h's exchange buffers -- whose senders are the local ids
// [s0, s1).
void full_region(uint32_t nloc, int NH, int h, uint32_t& t0, uint32_t& t1, uint32_t& s0, uint32_t& s1) {
    const uint32_t nt = (uint32_t)(((uint64_t)nloc + (1u << FB_TB) - 1) >> FB_TB);
    t0 = (uint32_t)((uint64_t)nt * h / NH);
    t1 = (uint32_t)((uint64_t)nt * (h + 1) / NH);
    s0 = (uint32_t)std::min<uint64_t>(nloc, (uint64_t)t0 << FB_TB);
    s1 = (uint32_t)std::min<uint64_t>(nloc, (uint64_t)t1 << FB_TB);
}

// Local sender ids [s_lo, s_hi) of region h.
void xregion(const Slab& sl, int NH, int h, uint32_t& s_lo, uint32_t& s_hi) {
    const DevState& S = sl.S;
    uint32_t split = S.nloc / 2;
    if (sl.lists) {  // tiles [tb[h], tb[h + 1])
        auto at = [&](uint32_t t) {
            const int64_t b = (int64_t)(S.lo / XTILE + t) * XTILE - S.lo;
            return (uint32_t)std::min<int64_t>(S.nloc, std::max<int64_t>(0, b));
        };
        s_lo = at(sl.tb[h]);
        s_hi = h + 1 == NH ? S.nloc : at(sl.tb[h + 1]);
        return;
    }
    s_lo = NH == 1 || h == 0 ? 0u : split;
    s_hi = NH == 1 || h == 1 ? S.nloc : split;
}

namespace {

constexpr uint32_t BITS_ALIGN = 1024;  // bitmap chunks start on 128-byte boundaries

size_t xbuf_bytes(uint32_t cap, bool push) {
    if (!cap) return 0;
    const size_t slots = ((size_t)cap * 4 + 15) & ~(size_t)15;
    return 16 + slots + (push ? (size_t)cap * 16 : 0);
}

uint32_t bits_for(uint64_t maxval) {
    uint32_t b = 1;
    while (b < 32 && (maxval >> b) != 0) ++b;
    return b;
}

// Slab boundaries: 3D / Imp3D whole x-planes (Program.fs:246-257 id = x g^2 + y g + z),
// line contiguous ids; full topology is single-rank.
int make_bounds(gp_sim* s) {
    const int W = s->world;
    s->bounds.assign(W + 1, 0);
    const int topo = s->cfg.topology;
    if (W == 1) {
        s->bounds[1] = (uint32_t)s->P;
        s->halo = 0;
        return GP_OK;
    }
    if (W > XMAXW) {
        set_err("at most %d ranks are supported (got %d)", XMAXW, W);
        return GP_EINVAL;
    }
    if (topo == GP_FULL) {  // contiguous ids, no halo: every message goes through the exchange
        if (s->P < W) {
            set_err("full topology with %lld nodes cannot be split over %d ranks", (long long)s->P, W);
            return GP_EINVAL;
        }
        for (int w = 0; w <= W; ++w) s->bounds[w] = (uint32_t)(s->P * w / W);
        s->halo = 0;
    } else if (topo == GP_LINE) {
        if (s->P < W) {
            set_err("line with %lld nodes cannot be split over %d ranks", (long long)s->P, W);
            return GP_EINVAL;
        }
        for (int w = 0; w <= W; ++w) s->bounds[w] = (uint32_t)(s->P * w / W);
        s->halo = 1;
    } else {
        if (s->g < W) {
            set_err("a %lld^3 lattice has fewer planes than ranks (%d)", (long long)s->g, W);
            return GP_EINVAL;
        }
        for (int w = 0; w <= W; ++w) s->bounds[w] = (uint32_t)((s->g * w / W) * s->g * s->g);
        s->halo = (uint32_t)(s->g * s->g);
    }
    return GP_OK;
}

// Device state of slab `r` (rank r): ids [bounds[r], bounds[r+1]) plus halos.
int alloc_slab(gp_sim* s, Slab& sl, int r) {
    DevState& S = sl.S;
    const int W = s->world;
    sl.rank = r;
    const uint32_t lo = s->bounds[r], hi = s->bounds[r + 1];
    sl.hi = hi;
    S.topo = s->cfg.topology;
    S.alg = s->cfg.algorithm;
    S.G.P = (uint32_t)s->P;
    S.G.T = (uint32_t)s->T;
    S.G.g = (uint32_t)s->g;
    S.G.g2 = (uint32_t)(s->g * s->g);
    S.G.div_g = make_fastdiv(S.G.g ? S.G.g : 1);
    S.G.div_g2 = make_fastdiv(S.G.g2 ? S.G.g2 : 1);
    S.k0 = (uint32_t)s->cfg.seed;
    S.k1 = (uint32_t)(s->cfg.seed >> 32);
    // choice = Random().Next(0, nodes) (Program.fs:193,221,263)
    S.seed_node = uniform(S.k0, S.k1, S_START, 0, 0, (uint32_t)s->T);
    S.lo = lo;
    S.nloc = hi - lo;
    S.ext_lo = r > 0 ? lo - s->halo : lo;
    S.ext_hi = r < W - 1 ? hi + s->halo : hi;
    S.base = S.ext_lo & ~3u;  // 4-aligned: the tile kernels move node bytes as words
    S.rtag = nullptr;
    S.rmsg = nullptr;
    S.rk = nullptr;
    S.rtg = nullptr;
    S.sbits = nullptr;
    S.xhdr[0] = S.xhdr[1] = nullptr;
    S.xvals[0] = S.xvals[1] = nullptr;
    S.xnv = 0;
    int rc;
    const size_t next = (size_t)(S.ext_hi - S.base) + 1024;  // node arrays (+ word-I/O padding)
    const size_t nl = S.nloc;
    if ((rc = dev_alloc_t(s, &S.ctl, 1))) return rc;
    if ((rc = dev_alloc_t(s, &S.tq, 2 * 8 * TQ_STRIDE))) return rc;
    HIP_TRY(hipMemsetAsync(S.tq, 0, sizeof(uint32_t) * 2 * 8 * TQ_STRIDE, s->stream));
    if (S.alg == PUSHSUM) {
        if ((rc = dev_alloc_t(s, &S.sw[0], next)) || (rc = dev_alloc_t(s, &S.sw[1], next)) ||
            (rc = dev_alloc_t(s, &S.nb[0], next)))
            return rc;
        if (S.topo != FULL && (rc = dev_alloc_t(s, &S.nb[1], next))) return rc;
        // zero sentinel just past the ids the slab holds: the tile kernels gather it for
        // lattice directions without a sender (never written by any round)
        for (int bb = 0; bb < 2; ++bb)
            HIP_TRY(hipMemsetAsync(S.sw[bb] + (S.ext_hi - S.base), 0, sizeof(double2), s->stream));
    } else {
        if ((rc = dev_alloc_t(s, &S.c, nl))) return rc;
        if (S.topo == FULL) {
            if ((rc = dev_alloc_t(s, &S.inc, nl))) return rc;
        } else {
            if ((rc = dev_alloc_t(s, &S.nb[0], next)) || (rc = dev_alloc_t(s, &S.nb[1], next))) return rc;
            S.nchunks = (uint32_t)((s->T + INJ_CHUNK - 1) / INJ_CHUNK);
            if ((rc = dev_alloc_t(s, &S.live_bits, (size_t)S.nchunks * (INJ_CHUNK / 32))) ||
                (rc = dev_alloc_t(s, &S.chunk_live, S.nchunks)))
                return rc;
        }
    }
    if (S.topo == FULL && S.alg == PUSHSUM) {  // LDS-binned message staging of this rank's receivers (gp_fullbin.hip)
        const FullBinPlan fp = full_bin_plan(S.nloc, W == 1);
        S.fb_nb2 = fp.nb2;
        S.fb_cap2 = fp.cap2;
        // (GP_FB_CAP2 / GP_FB_CAP1, experiments: smaller bins, to put a round's fullest fine tile /
        // coarse bin exactly at and one past its capacity; tests/test_gpu_fullbin_edges.py)
        if (const char* e = exp_env("GP_FB_CAP2")) S.fb_cap2 = std::min<uint32_t>(FB_CAP2, (uint32_t)std::max(1, std::atoi(e)));
        const size_t m2 = (size_t)fp.nb2 * S.fb_cap2;
        if ((rc = dev_alloc_t(s, &S.fb_cnt2, fp.nb2)) || (rc = dev_alloc_t(s, &S.fb_hdr2, m2)) ||
            (rc = dev_alloc_t(s, &S.fb_pay2, m2)))
            return rc;
        if (W == 1) {
            // one rank: coarse bins hdr1 / pay1; the fold of round r bins round r+1's messages
            // into them (k_fb_fold<FOLD_SEND>; GP_FB_FUSED=0, experiments: three passes)
            bool fused = true;
            if (const char* e = exp_env("GP_FB_FUSED")) fused = e[0] == '1';
            const FullBinPlan f1 = full_bin_plan(S.nloc, fused);
            S.fb_s1 = f1.s1;
            S.fb_nb1 = f1.nb1;
            S.fb_cap1 = f1.cap1;
            if (const char* e = exp_env("GP_FB_CAP1")) S.fb_cap1 = std::min<uint32_t>(f1.cap1, (uint32_t)std::max(1, std::atoi(e)));
            S.fb_fused = fused && f1.nb1 <= full_bin_fused_max_bins() ? 1u : 0u;
            const size_t m1 = (size_t)f1.nb1 * S.fb_cap1;
            // (+ FB_JUNK: the fold's write-out sends lanes without a message to the slots past the
            // last bin, so every thread issues the same number of stores)
            if ((rc = dev_alloc_t(s, &S.fb_cnt1, f1.nb1)) || (rc = dev_alloc_t(s, &S.fb_hdr1, m1 + FB_JUNK)) ||
                (rc = dev_alloc_t(s, &S.fb_pay1, m1 + FB_JUNK)))
                return rc;
        } else {
            // several ranks (round 6): the coarse bins are the exchange buffers (setup_exchange) --
            // the fold bins the next round's messages by destination rank and coarse bin into them,
            // and each rank's split reads them where they arrive (k_fb_fold<FOLD_SEND_RANKS>)
            S.fb_s1 = full_bin_multi_s1(s->bounds.data(), W);
            S.fb_nb1 = (uint32_t)(((uint64_t)S.nloc + (1ull << S.fb_s1) - 1) >> S.fb_s1);
            S.fb_cap1 = 0;
            S.fb_fused = 1;
            S.fb_cnt1 = S.fb_hdr1 = nullptr;
            S.fb_pay1 = nullptr;
        }
    }
    if (col_gossip_counts(S)) {  // senders count their random-edge deliveries at the target (k_gossip_col)
        // byte counters, four per word (C3: 0.632 -> 0.600 ms per round, reads 16.5 -> 11.7 and
        // writes 11.2 -> 9.8 B/node; profiles/r04/c3_byte_counters.txt)
        S.rq8 = 1;
        if (const char* e = exp_env("GP_RQ8")) S.rq8 = e[0] == '1' ? 1u : 0u;
        for (int q = 0; q < 2; ++q) {
            if ((rc = dev_alloc_t(s, &S.rq[q], (size_t)S.nloc + 64))) return rc;
            HIP_TRY(hipMemsetAsync(S.rq[q], 0, sizeof(uint32_t) * ((size_t)S.nloc + 64), s->stream));
        }
    }
    // random-edge bitmaps of the tile kernels (the column kernel counts deliveries instead)
    if (S.topo == IMP3D && !col_gossip_counts(S)) {
        S.rbits_words = rbits_words_for(S.lo, S.nloc);
        if ((rc = dev_alloc_t(s, &S.rbits[0], S.rbits_words)) || (rc = dev_alloc_t(s, &S.rbits[1], S.rbits_words)))
            return rc;
    }
    return GP_OK;
}

// Push-sum on a 3D / Imp3D lattice over several ranks: the halo planes' (s, w) travel compacted
// (only the senders toward the neighbour, HaloArgs in gp_xchg.hpp): C5 at W = 8, 16 MB -> 3.9 MB
// per direction and round.
int setup_halo(gp_sim* s) {
    s->halo_slots = 0;
    const bool lattice = s->cfg.topology == GP_3D || s->cfg.topology == GP_IMP3D;
    if (!lattice || s->cfg.algorithm != GP_PUSHSUM || s->world < 2 || s->halo < HALO_CHUNK) return GP_OK;
    s->halo_cap = halo_chunk_cap((uint32_t)s->g, s->cfg.topology == GP_IMP3D);
    s->halo_slots = halo_buf_slots(s->halo, s->halo_cap);
    int rc;
    for (Slab& sl : s->slab) {
        for (int k = 0; k < 2; ++k) {
            const bool has = k == 0 ? sl.rank > 0 : sl.rank < s->world - 1;
            if (!has) continue;
            if ((rc = dev_alloc_t(s, &sl.hsend[k], s->halo_slots)) || (rc = dev_alloc_t(s, &sl.hrecv[k], s->halo_slots)))
                return rc;
        }
    }
    return GP_OK;
}

constexpr int XREGIONS = 4;  // Imp3D push-sum exchange regions (see exchange_regions)
constexpr uint32_t RREG_MIN_NODES = 1u << 24;  // region rounds from this slab size on (round_regions)

// Exchange regions of a slab's senders: push-sum runs two (one's transfer overlaps the
// other's packing), gossip one.  Imp3D push-sum cuts them at a tile boundary (the lists'
// tiles); the full topology at a fine-tile boundary (full_region).
int exchange_regions(const gp_sim* s) {
    const bool push = s->cfg.algorithm == GP_PUSHSUM;
    // Imp3D push-sum lists: XREGIONS regions of the slab's tiles (the last one's transfer is what
    // the round cannot hide); the full topology's two halves.  Two ranks with large slabs: eight
    // regions, where one link carries half of every rank's messages -- C5, region rounds, same box
    // (profiles/r05/rregions/reg8.txt): W = 2 10.72 -> 10.21 ms at 128 GB/s, 12.53 -> 11.50 at
    // 64; at W = 4 and 8 eight were slower (5.50 -> 5.69, 2.82 -> 3.00 ms at 128 GB/s)
    int NH = push ? (s->cfg.topology == GP_IMP3D ? XREGIONS : FB_REGIONS) : 1;
    if (push && s->cfg.topology == GP_IMP3D && s->world == 2 && s->bounds.size() == 3 &&
        std::min(s->bounds[1] - s->bounds[0], s->bounds[2] - s->bounds[1]) >= RREG_MIN_NODES)
        NH = 8;
    static_assert(XMAXH >= 8 && RREG_MAX >= 8, "eight regions for two ranks");
    return NH;
}

// Round kernel launches per round (DevState::rregions).  Imp3D push-sum across ranks runs the
// round kernel region by region (launch_round_regions): region h's lists are packed and travel
// while the later regions compute.  C5 modelled from virtual ranks, same box, against one launch
// per round with the lists packed and sent after it (profiles/r05/rregions/): W = 2 12.92 ->
// 10.50 ms at 128 GB/s per link and direction, 17.97 -> 12.48 at 64; W = 4 5.46 -> 5.48 and
// 6.76 -> 5.81; W = 8 2.75 -> 2.74 and 2.96 -> 2.83 (the round kernel itself +2-5 %: four launch
// tails).  Small slabs (< RREG_MIN_NODES) move little and keep one launch per round: their rounds
// are launch-bound, and rank processes sharing one GPU (the tests) run them several times slower
// with four persistent launches per round.  The experiments build's GP_RREGIONS=0/1 overrides.
uint32_t round_regions(const gp_sim* s, int kernel, uint32_t walk) {
    if (s->world < 2 || s->cfg.topology != GP_IMP3D || s->cfg.algorithm != GP_PUSHSUM || kernel != KERNEL_TILE ||
        walk != 3)
        return 1;
    int on = 1;
    for (int w = 0; w < s->world; ++w)
        if (s->bounds[w + 1] - s->bounds[w] < RREG_MIN_NODES) on = 0;
    if (const char* e = exp_env("GP_RREGIONS")) on = std::atoi(e);
    const int NH = exchange_regions(s);
    if (!on || NH < 2 || NH > RREG_MAX) return 1;
    uint32_t rb[RREG_MAX + 1];
    for (int w = 0; w < s->world; ++w)
        if (!region_tiles(s->bounds[w], s->bounds[w + 1] - s->bounds[w], (uint64_t)s->g * s->g, NH, rb)) return 1;
    return (uint32_t)NH;
}

uint32_t slab_tiles(uint32_t lo, uint32_t nloc) {
    return (uint32_t)(((uint64_t)lo + nloc + XTILE - 1) / XTILE - lo / XTILE);
}

// Offset of chunk (h, a) in rank b's receive buffer, in units of size(hh, aa): the chunks lie
// in (h, a) order, a != b (every rank lays out its receive buffer this way, and every sender
// addresses it this way).  Header words: list_hw below; slots of the vals region: setup_exchange.
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

uint32_t list_hw(const gp_sim* s, int b, int h, int a) {
    const int W = s->world, NH = s->xhalves;
    return (uint32_t)chunk_offset(W, NH, b, h, a, [&](int hh, int aa) { return s->list_nw[((size_t)aa * NH + hh) * W + b]; });
}

// Imp3D push-sum over several ranks: the static list plan (gp_xchg.hpp) of every slab
// from the global random edges, the header-word counts of every chunk, and for this
// rank's slabs the tile table gw and every remote in-edge's list key (rk).  kk: a
// P-word scratch array; src: senders in receiver order (global); edge0: first global
// in-edge of every rank.
int build_lists(gp_sim* s, const uint32_t* rnd_all, uint32_t* kk, const uint32_t* src,
                const std::vector<uint32_t>& edge0) {
    const int W = s->world;
    const int NH = s->xhalves = exchange_regions(s);
    s->list_nw.assign((size_t)W * NH * W, 0);
    std::vector<std::vector<uint32_t>> gw_all(W);
    std::vector<std::vector<uint8_t>> lwt_all(W);
    std::vector<std::array<uint32_t, XMAXH + 1>> tb(W);  // per slab: region tile boundaries
    Scratch tmp_mem;
    for (int a = 0; a < W; ++a) {
        const uint32_t lo = s->bounds[a], nloc = s->bounds[a + 1] - lo;
        const uint32_t nt = slab_tiles(lo, nloc);
        // regions of whole planes (region_tiles: the round kernel's regions when it runs region by
        // region), else of equal tile counts
        if (!region_tiles(lo, nloc, (uint64_t)s->g * s->g, NH, tb[a].data()))
            for (int h = 0; h <= NH; ++h) tb[a][h] = (uint32_t)((uint64_t)nt * h / NH);
        for (int h = NH + 1; h <= XMAXH; ++h) tb[a][h] = nt;
        uint32_t* cnt = nullptr;
        HIP_TRY(tmp_mem.alloc(&cnt, (size_t)nt * W + 1));
        ListCountArgs ca{};
        ca.rnd = rnd_all;
        ca.lo = lo;
        ca.nloc = nloc;
        ca.W = W;
        ca.a = a;
        for (int w = 0; w <= W; ++w) ca.bounds[w] = s->bounds[w];
        ca.cnt = cnt;
        HIP_TRY(launch_list_count(ca, s->stream));
        std::vector<uint32_t> hc((size_t)nt * W);
        HIP_TRY(hipMemcpyAsync(hc.data(), cnt, sizeof(uint32_t) * hc.size(), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::vector<uint32_t>& gw = gw_all[a];
        gw.assign((size_t)nt * W, 0);
        std::vector<uint8_t>& lwt = lwt_all[a];  // per tile: prefix over d of its segments' words
        lwt.assign((size_t)nt * (W + 1), 0);
        for (uint32_t t = 0; t < nt; ++t) {
            uint32_t w = 0;
            for (int d = 0; d < W; ++d) {
                lwt[(size_t)t * (W + 1) + d] = (uint8_t)w;
                w += (hc[(size_t)t * W + d] + 63u) / 64u;
            }
            lwt[(size_t)t * (W + 1) + W] = (uint8_t)w;  // <= 16 + W words
        }
        for (int d = 0; d < W; ++d) {
            uint64_t run[XMAXH] = {};
            for (uint32_t t = 0, h = 0; t < nt; ++t) {
                while ((int)h + 1 < NH && t >= tb[a][h + 1]) ++h;
                gw[(size_t)t * W + d] = (uint32_t)run[h];
                run[h] += (hc[(size_t)t * W + d] + 63u) / 64u;
            }
            for (int h = 0; h < NH; ++h) {
                if (run[h] >= (1ull << 26)) {
                    set_err("internal: random-edge list %d -> %d has %llu header words (limit 2^26)", a, d,
                            (unsigned long long)run[h]);
                    return GP_EINVAL;
                }
                s->list_nw[((size_t)a * NH + h) * W + d] = (uint32_t)run[h];
            }
        }
    }
    // every sender's key at its destination, then this rank's in-edges' keys
    for (int a = 0; a < W; ++a) {
        const uint32_t lo = s->bounds[a], nloc = s->bounds[a + 1] - lo;
        uint32_t* gw = nullptr;
        HIP_TRY(tmp_mem.alloc(&gw, gw_all[a].size() + 1));
        HIP_TRY(hipMemcpyAsync(gw, gw_all[a].data(), sizeof(uint32_t) * gw_all[a].size(), hipMemcpyHostToDevice,
                               s->stream));
        ListKeyArgs ka{};
        ka.rnd = rnd_all;
        ka.gw = gw;
        ka.lo = lo;
        ka.nloc = nloc;
        for (int h = 0; h <= XMAXH; ++h) ka.tb[h] = tb[a][h];
        ka.NH = NH;
        ka.W = W;
        ka.a = a;
        for (int w = 0; w <= W; ++w) ka.bounds[w] = s->bounds[w];
        for (int h = 0; h < NH; ++h)
            for (int b = 0; b < W; ++b) ka.hw[h][b] = b == a ? 0u : list_hw(s, b, h, a);
        ka.key = kk;
        ka.xdr = nullptr;
        for (Slab& sl : s->slab) {
            if (sl.rank != a) continue;
            int rc;
            if ((rc = dev_alloc_t(s, &sl.xdr, (size_t)nloc + 64))) return rc;
            ka.xdr = sl.xdr;
        }
        HIP_TRY(launch_list_key(ka, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));  // (gw is freed at scope end; keep it simple)
    }
    int rc;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        const int r = sl.rank;
        sl.lists = true;
        sl.nt = slab_tiles(S.lo, S.nloc);
        for (int h = 0; h <= XMAXH; ++h) sl.tb[h] = tb[r][h];
        if ((rc = dev_alloc_t(s, &sl.gw, gw_all[r].size() + 1)) || (rc = dev_alloc_t(s, &sl.lwt, lwt_all[r].size() + 16)))
            return rc;
        HIP_TRY(hipMemcpyAsync(sl.gw, gw_all[r].data(), sizeof(uint32_t) * gw_all[r].size(), hipMemcpyHostToDevice,
                               s->stream));
        HIP_TRY(hipMemcpyAsync(sl.lwt, lwt_all[r].data(), lwt_all[r].size(), hipMemcpyHostToDevice, s->stream));
        const uint32_t ne = edge0[r + 1] - edge0[r];
        if ((rc = dev_alloc_t(s, &S.rk, (size_t)ne + 4))) return rc;
        HIP_TRY(launch_gather_keys(kk, src + edge0[r], ne, S.rk, s->grid, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}

// Imp3D gossip on the column kernel over several ranks: the bitmap plan (gp_xchg.hpp).
// For every source slab a, the edges with a sender on a get their rank among the
// same receiver slab's edges from a (exclusive scan of a flag over the global
// receiver order); this rank's senders learn their bit (rtg) and its receivers
// the target of every received bit (tgt).  flag / scan / pos: P + 1 words of scratch.
int build_bits(gp_sim* s, const uint32_t* src, const uint32_t* recv, const uint32_t* inv,
               const std::vector<uint32_t>& edge0, uint32_t* flag, uint32_t* scan, uint32_t* pos) {
    const int W = s->world;
    const uint32_t P = (uint32_t)s->P;
    Scratch tmp_mem;
    size_t scan_bytes = 0;
    HIP_TRY(exclusive_scan_u32(nullptr, scan_bytes, flag, scan, P + 1, s->stream));
    uint8_t* scan_tmp = nullptr;
    HIP_TRY(tmp_mem.alloc(&scan_tmp, scan_bytes ? scan_bytes : 4));
    std::vector<std::vector<uint32_t>> n(W, std::vector<uint32_t>(W, 0));  // edges a -> b
    for (int a = 0; a < W; ++a) {
        HIP_TRY(launch_src_flag(src, P, s->bounds.data(), W, a, flag, s->grid, s->stream));
        HIP_TRY(exclusive_scan_u32(scan_tmp, scan_bytes, flag, scan, P + 1, s->stream));
        BitsSetupArgs ba{};
        ba.src = src;
        ba.recv = recv;
        ba.scan = scan;
        ba.pos = pos;
        ba.n = P;
        ba.W = W;
        ba.a = a;
        for (int w = 0; w <= W; ++w) {
            ba.bounds[w] = s->bounds[w];
            ba.edge0[w] = edge0[w];
        }
        HIP_TRY(launch_bits_pos(ba, s->grid, s->stream));
        std::vector<uint32_t> at(W + 1);
        for (int b = 0; b <= W; ++b)
            HIP_TRY(hipMemcpyAsync(&at[b], scan + edge0[b], sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (int b = 0; b < W; ++b) n[a][b] = a == b ? 0u : at[b + 1] - at[b];
    }
    auto pad = [](uint64_t x) { return (x + BITS_ALIGN - 1) / BITS_ALIGN * BITS_ALIGN; };
    int rc;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        const int me = sl.rank;
        sl.bits = true;
        sl.bo.assign(W, 0);
        sl.bn.assign(W, 0);
        sl.ro.assign(W, 0);
        sl.rn.assign(W, 0);
        uint64_t so = 0, ri = 0;
        for (int d = 0; d < W; ++d) {
            if (d == me) continue;
            sl.bo[d] = (uint32_t)so;
            sl.bn[d] = n[me][d];
            so += pad(n[me][d]);
            sl.ro[d] = (uint32_t)ri;
            sl.rn[d] = n[d][me];
            ri += pad(n[d][me]);
        }
        if (so >= (1ull << 31) || ri >= (1ull << 31)) {
            set_err("internal: random-edge bitmaps beyond 2^31 bits");
            return GP_EINVAL;
        }
        sl.nbits_out = (uint32_t)so;
        sl.nbits_in = (uint32_t)ri;
        if ((rc = dev_alloc_t(s, &S.rtg, (size_t)S.nloc + 64)) || (rc = dev_alloc_t(s, &S.sbits, so / 32 + 1)) ||
            (rc = dev_alloc_t(s, &sl.rbits_in, ri / 32 + 1)) || (rc = dev_alloc_t(s, &sl.tgt, ri + 1)))
            return rc;
        HIP_TRY(hipMemsetAsync(S.sbits, 0, (so / 32 + 1) * 4, s->stream));
        HIP_TRY(hipMemsetAsync(sl.rbits_in, 0, (ri / 32 + 1) * 4, s->stream));
        BitsEndsArgs ea{};
        ea.rnd = S.rnd;
        ea.inv = inv;
        ea.src = src;
        ea.recv = recv;
        ea.pos = pos;
        ea.rtg = S.rtg;
        ea.tgt = sl.tgt;
        ea.lo = S.lo;
        ea.nloc = S.nloc;
        ea.e0 = edge0[me];
        ea.e1 = edge0[me + 1];
        ea.W = W;
        ea.me = me;
        for (int w = 0; w <= W; ++w) ea.bounds[w] = s->bounds[w];
        for (int w = 0; w < W; ++w) {
            ea.bo[w] = sl.bo[w];
            ea.ro[w] = sl.ro[w];
        }
        HIP_TRY(launch_bits_ends(ea, s->grid, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}

// Imp3D: draw rnd[] for every node (Program.fs:258-260), then a stable sort of
// (key(rnd[i]), i) by key gives every receiver's senders in ascending id order,
// and the exclusive scan of the per-receiver in-degrees the CSR offsets (in_off,
// in_src in id order).  Every rank builds the global order (it is
// deterministic; ranks own consecutive id ranges) and keeps its
// receivers' slice; with several ranks, each local sender also learns the
// position of its message in the destination's in-edge array (pos).

int build_imp3d(gp_sim* s) {
    const uint32_t P = (uint32_t)s->P;
    const int W = s->world;
    DevState& S0 = s->slab[0].S;
    Scratch tmp_mem;  // setup temporaries, freed on every exit path
    uint32_t *rnd_all = nullptr, *iota = nullptr, *keys_sorted = nullptr, *src_sorted = nullptr, *counts = nullptr,
             *off_all = nullptr, *inv = nullptr;
    const uint64_t nkeys = P;
    HIP_TRY(tmp_mem.alloc(&rnd_all, P));
    HIP_TRY(tmp_mem.alloc(&iota, P));
    HIP_TRY(tmp_mem.alloc(&keys_sorted, P));
    HIP_TRY(tmp_mem.alloc(&src_sorted, P));
    HIP_TRY(tmp_mem.alloc(&counts, (size_t)nkeys + 1));
    HIP_TRY(tmp_mem.alloc(&off_all, (size_t)nkeys + 1));
    HIP_TRY(launch_topo_rnd_range(S0.k0, S0.k1, P, 0, P, rnd_all, s->grid, s->stream));
    HIP_TRY(launch_iota(iota, P, s->grid, s->stream));
    const uint32_t bits = bits_for(nkeys > 1 ? nkeys - 1 : 0);
    size_t tmp_bytes = 0;
    HIP_TRY(sort_pairs(nullptr, tmp_bytes, rnd_all, keys_sorted, iota, src_sorted, P, bits, s->stream));
    uint8_t* tmp = nullptr;
    HIP_TRY(tmp_mem.alloc(&tmp, tmp_bytes ? tmp_bytes : 4));
    HIP_TRY(sort_pairs(tmp, tmp_bytes, rnd_all, keys_sorted, iota, src_sorted, P, bits, s->stream));
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(uint32_t) * ((size_t)nkeys + 1), s->stream));
    HIP_TRY(launch_histogram(rnd_all, P, counts, s->grid, s->stream));
    size_t scan_bytes = 0;
    HIP_TRY(exclusive_scan_u32(nullptr, scan_bytes, counts, off_all, (uint32_t)nkeys + 1, s->stream));
    uint8_t* scan_tmp = nullptr;
    HIP_TRY(tmp_mem.alloc(&scan_tmp, scan_bytes ? scan_bytes : 4));
    HIP_TRY(exclusive_scan_u32(scan_tmp, scan_bytes, counts, off_all, (uint32_t)nkeys + 1, s->stream));
    if (W > 1) {
        HIP_TRY(tmp_mem.alloc(&inv, P));
        HIP_TRY(launch_inverse(src_sorted, P, inv, s->grid, s->stream));
    }
    // first global edge of every rank
    std::vector<uint32_t> edge0(W + 1);
    for (int w = 0; w <= W; ++w)
        HIP_TRY(hipMemcpyAsync(&edge0[w], off_all + s->bounds[w], sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    int rc;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        const int r = sl.rank;
        const uint32_t ne = edge0[r + 1] - edge0[r];
        sl.nedges = ne;
        S.nedges = ne;
        if ((rc = dev_alloc_t(s, &S.rnd, S.nloc))) return rc;
        HIP_TRY(hipMemcpyAsync(S.rnd, rnd_all + S.lo, sizeof(uint32_t) * S.nloc, hipMemcpyDeviceToDevice, s->stream));
        // in-lists padded by 4 words: the tile kernels stage them with 16-byte LDS-DMA
        if ((rc = dev_alloc_t(s, &S.in_off, (size_t)S.nloc + 1 + 4)) ||
            (rc = dev_alloc_t(s, &S.in_src, (size_t)ne + 4)))
            return rc;
        HIP_TRY(hipMemcpyAsync(S.in_off, off_all + S.lo, sizeof(uint32_t) * ((size_t)S.nloc + 1),
                               hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(launch_sub(S.in_off, S.nloc + 1, edge0[r], s->grid, s->stream));
        if (ne)
            HIP_TRY(hipMemcpyAsync(S.in_src, src_sorted + edge0[r], sizeof(uint32_t) * ne,
                                   hipMemcpyDeviceToDevice, s->stream));
        S.in_srcd = nullptr;
        bool pack = true;
        if (const char* np = exp_env("GP_NO_PACK")) pack = np[0] != '1';  // force the unpacked (P > 2^30) path
        if (S.alg == PUSHSUM && S.kernel == KERNEL_TILE && s->P <= (1ll << 30) && s->g >= 2 && pack) {
            if ((rc = dev_alloc_t(s, &S.in_srcd, (size_t)ne + 4))) return rc;
            if (ne) HIP_TRY(launch_pack_src_deg(S.in_src, S.in_srcd, ne, S.G, s->grid, s->stream));
        }
        S.ind4 = nullptr;
        if (S.alg == PUSHSUM && S.kernel == KERNEL_TILE) {
            if ((rc = dev_alloc_t(s, &S.ind4, ind4_bytes_for(S.lo, S.nloc)))) return rc;
            uint32_t wide_at = 15;  // in-degree >= 15: the tile reads in_off (gp_ps_tile.hip)
            if (const char* e = exp_env("GP_IND4_WIDE")) wide_at = (uint32_t)std::max(1, std::atoi(e));
            HIP_TRY(launch_pack_ind4(S, wide_at, s->grid, s->stream));
        }
        if (W > 1 && !col_gossip_counts(S)) {  // (the gossip column kernel's bitmaps: build_bits)
            // push-sum: sender-ordered lists (build_lists), no slots or tags; gossip tile kernel:
            // {slot} entries and round tags (k_pack / k_unpack)
            const bool slots = S.alg != PUSHSUM;
            if ((rc = dev_alloc_t(s, &sl.xdst, (size_t)S.nloc + 64))) return rc;
            if (slots && ((rc = dev_alloc_t(s, &sl.pos, S.nloc)) || (rc = dev_alloc_t(s, &S.rtag, ne))))
                return rc;
            if (slots) HIP_TRY(hipMemsetAsync(S.rtag, 0xFF, sizeof(uint32_t) * (ne ? ne : 1), s->stream));
            PosArgs pa{};
            pa.rnd = S.rnd;
            pa.inv = inv;
            pa.pos = slots ? sl.pos : nullptr;
            pa.xdst = sl.xdst;
            pa.lo = S.lo;
            pa.nloc = S.nloc;
            pa.W = W;
            pa.me = r;
            for (int w = 0; w <= W; ++w) pa.bounds[w] = s->bounds[w];
            for (int w = 0; w < W; ++w) pa.edge0[w] = edge0[w];
            HIP_TRY(launch_make_pos(pa, s->grid, s->stream));
        }
    }
    // (iota, the sort's value input, is free again: the lists' key scratch)
    if (W > 1 && s->cfg.algorithm == GP_PUSHSUM && (rc = build_lists(s, rnd_all, iota, src_sorted, edge0))) return rc;
    // (counts, off_all -- copied into the slabs' in_off -- and iota are free again: the bitmaps'
    // scratch, in stream order after those copies)
    if (W > 1 && col_gossip_counts(S0) && (rc = build_bits(s, src_sorted, keys_sorted, inv, edge0, counts, off_all, iota)))
        return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}

// Fixed-capacity exchange buffers per rank pair: capacity = expected messages
// per round + 12 sigma + 64 (never more than the pair's random edges).  Push-sum
// exchanges have two regions per pair, one per half of the sender's senders
// (s->xhalves), moved separately on the exchange stream so that one half's
// transfer overlaps the other half's packing / unpacking (full topology:
// launch_round_full_multi; Imp3D: exchange).
int setup_exchange(gp_sim* s) {
    const int W = s->world;
    const bool push = s->cfg.algorithm == GP_PUSHSUM;
    const bool full = s->cfg.topology == GP_FULL;
    if (!s->slab.empty() && s->slab[0].bits) {  // gossip column kernel: fixed-size bitmaps (build_bits)
        s->xhalves = 1;
        for (Slab& sl : s->slab) sl.overflow = &sl.S.ctl->overflow;
        return GP_OK;
    }
    const int NH = exchange_regions(s);
    s->xhalves = NH;
    std::vector<uint32_t> caps((size_t)NH * W * W, 0);  // caps[(h * W + a) * W + b]: a -> b, region h
    Scratch tmp_mem;
    double* mu = nullptr;
    unsigned long long* n = nullptr;
    HIP_TRY(tmp_mem.alloc(&mu, XMAXW));
    HIP_TRY(tmp_mem.alloc(&n, XMAXW));
    // full push-sum: the coarse bins of every destination travel as the exchange buffers
    // (FbBins, gp_fullbin.hpp); the coarse-bin size every rank uses, and a rank's bin count
    const uint32_t fs1 = full && push ? full_bin_multi_s1(s->bounds.data(), W) : 0;
    if (full) {
        // every active sender picks a uniform target among P-1: a function of the slab bounds
        // only, so every rank computes the whole table
        for (int a = 0; a < W; ++a) {
            const uint32_t na = s->bounds[a + 1] - s->bounds[a];
            for (int h = 0; h < NH; ++h) {
                uint32_t t0, t1, s0, s1;
                full_region(na, NH, h, t0, t1, s0, s1);
                const double nah = (double)(s1 - s0);
                for (int b = 0; b < W; ++b) {
                    if (push) {
                        // push-sum: messages from a's region h to one coarse bin of b (2^fs1
                        // receivers; a rank's messages to itself included, they pass through its
                        // own receive buffer) are at most Binomial(na_h, 2^fs1 / (P-1))
                        caps[((size_t)h * W + a) * W + b] = full_bin_multi_cap(s1 - s0, fs1, (uint32_t)s->P);
                        continue;
                    }
                    // gossip: messages a -> b at most Binomial(na, nb / (P-1))
                    if (b == a) continue;
                    const double nb = (double)(s->bounds[b + 1] - s->bounds[b]);
                    const double m = nah * nb / (double)(s->P - 1);
                    const double c = std::ceil(m + 12.0 * std::sqrt(m) + 64.0);
                    caps[((size_t)h * W + a) * W + b] = (uint32_t)std::min(c, nah);
                }
            }
        }
    }
    for (Slab& sl : s->slab) {
        if (full) break;
        DevState& S = sl.S;
        for (int h = 0; h < NH; ++h) {  // region h: senders [s_lo, s_hi) of the slab (xregion)
            HIP_TRY(hipMemsetAsync(mu, 0, sizeof(double) * XMAXW, s->stream));
            HIP_TRY(hipMemsetAsync(n, 0, sizeof(unsigned long long) * XMAXW, s->stream));
            ExpectArgs ea{};
            ea.rnd = S.rnd;
            ea.lo = S.lo;
            ea.nloc = S.nloc;
            xregion(sl, NH, h, ea.s_lo, ea.s_hi);
            ea.W = W;
            ea.me = sl.rank;
            for (int w = 0; w <= W; ++w) ea.bounds[w] = s->bounds[w];
            ea.G = S.G;
            ea.mu = mu;
            ea.n = n;
            HIP_TRY(launch_expect(ea, s->grid, s->stream));
            double hmu[XMAXW];
            unsigned long long hn[XMAXW];
            HIP_TRY(hipMemcpyAsync(hmu, mu, sizeof hmu, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipMemcpyAsync(hn, n, sizeof hn, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            for (int b = 0; b < W; ++b) {
                if (b == sl.rank || hn[b] == 0) continue;
                const double c = std::ceil(hmu[b] + 12.0 * std::sqrt(hmu[b]) + 64.0);
                caps[((size_t)h * W + sl.rank) * W + b] = (uint32_t)std::min<double>(c, (double)hn[b]);
            }
        }
    }
    if (const char* e = exp_env("GP_XCAP")) {  // tests: force tiny buffers (overflow handling)
        const uint32_t cap = (uint32_t)std::max(1, std::atoi(e));
        for (auto& c : caps) c = std::min(c, cap);
    }
    if (s->mode == MODE_RCCL && !full) {
        // every rank learns the capacities of the buffers it will receive (per region)
        uint32_t* d = nullptr;
        HIP_TRY(tmp_mem.alloc(&d, (size_t)W * W));
        for (int h = 0; h < NH; ++h) {
            uint32_t* row = caps.data() + (size_t)h * W * W;
            HIP_TRY(hipMemcpyAsync(d + (size_t)s->rank * W, row + (size_t)s->rank * W, sizeof(uint32_t) * W,
                                   hipMemcpyHostToDevice, s->stream));
            NCCL_TRY(ncclAllGather(d + (size_t)s->rank * W, d, W, ncclUint32, s->comm, s->stream));
            HIP_TRY(hipMemcpyAsync(row, d, sizeof(uint32_t) * W * W, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
        }
    }
    int rc;
    if (!s->slab.empty() && s->slab[0].lists) {  // Imp3D push-sum: sender-ordered lists (gp_xchg.hpp)
        auto cap = [&](int h, int a, int b) { return caps[((size_t)h * W + a) * W + b]; };
        auto nw = [&](int h, int a, int b) { return s->list_nw[((size_t)a * NH + h) * W + b]; };
        // slot offset of chunk (h, a) in rank b's vals region (the order of list_hw)
        auto vo = [&](int b, int h, int a) {
            return chunk_offset(W, NH, b, h, a, [&](int hh, int aa) { return cap(hh, aa, b); });
        };
        for (Slab& sl : s->slab) {
            const int a = sl.rank;
            const size_t R = (size_t)NH * W;
            sl.cap_out.assign(R, 0);
            sl.cap_in.assign(R, 0);
            sl.lhdr.assign(R, 0);
            sl.lval.assign(R, 0);
            sl.rhdr.assign(R, 0);
            sl.rval.assign(R, 0);
            sl.vbase.assign(R, 0);
            size_t so = 0, hdr_in = 0;
            uint64_t nv_in = 0;
            for (int h = 0; h < NH; ++h)
                for (int b = 0; b < W; ++b) {
                    if (b == a) continue;
                    const size_t i = (size_t)h * W + b;
                    sl.cap_out[i] = cap(h, a, b);
                    sl.cap_in[i] = cap(h, b, a);
                    sl.lhdr[i] = so;
                    so += (size_t)nw(h, a, b) * 16;
                    sl.lval[i] = so;
                    so += (size_t)sl.cap_out[i] * 16;
                    sl.rhdr[i] = (size_t)list_hw(s, a, h, b) * 16;
                    hdr_in += (size_t)nw(h, b, a) * 16;
                    nv_in += sl.cap_in[i];
                    const uint64_t vb = vo(b, h, a);
                    if (vb >= (1ull << 32) || nv_in >= (1ull << 32)) {
                        set_err("internal: exchange vals region beyond 2^32 slots");
                        return GP_EINVAL;
                    }
                    sl.vbase[i] = (uint32_t)vb;
                }
            for (int h = 0; h < NH; ++h)
                for (int b = 0; b < W; ++b)
                    if (b != a) sl.rval[(size_t)h * W + b] = hdr_in + (size_t)vo(a, h, b) * 16;
            const size_t ro = hdr_in + (size_t)nv_in * 16;
            sl.xr_stride = sl.S.rregions > 1 ? (ro + 255) & ~(size_t)255 : 0;  // one buffer per round parity
            const size_t rt = sl.xr_stride ? 2 * sl.xr_stride : ro;
            if ((rc = dev_alloc_t(s, &sl.xsend, so)) || (rc = dev_alloc_t(s, &sl.xrecv, rt)) ||
                (rc = dev_alloc_t(s, &sl.xcnt, R)))
                return rc;
            HIP_TRY(hipMemsetAsync(sl.xsend, 0, so ? so : 16, s->stream));
            HIP_TRY(hipMemsetAsync(sl.xrecv, 0, rt ? rt : 16, s->stream));
            for (int k = 0; k < 2; ++k) {
                sl.S.xhdr[k] = reinterpret_cast<const XHdr*>(sl.xrecv + k * sl.xr_stride);
                sl.S.xvals[k] = reinterpret_cast<const double2*>(sl.xrecv + k * sl.xr_stride + hdr_in);
            }
            sl.S.xnv = (uint32_t)std::max<uint64_t>(1, nv_in);
            sl.overflow = &sl.S.ctl->overflow;
        }
    }
    for (Slab& sl : s->slab) {
        if (sl.lists) break;
        const int a = sl.rank;
        const size_t R = (size_t)NH * W;
        sl.cap_out.assign(R, 0);
        sl.cap_in.assign(R, 0);
        sl.soff.assign(R, 0);
        sl.sbytes.assign(R, 0);
        sl.roff.assign(R, 0);
        sl.rbytes.assign(R, 0);
        size_t so = 0, ro = 0;
        for (int h = 0; h < NH; ++h)
            for (int b = 0; b < W; ++b) {
                const size_t i = (size_t)h * W + b;
                sl.cap_out[i] = caps[((size_t)h * W + a) * W + b];
                sl.cap_in[i] = caps[((size_t)h * W + b) * W + a];
                sl.soff[i] = so;
                // (own messages: straight to xrecv; full push-sum: b's coarse bins, FbBins)
                sl.sbytes[i] = b == a ? 0 : full && push ? fb_bins_bytes(full_coarse_bins(s->bounds, b, fs1), sl.cap_out[i]) : xbuf_bytes(sl.cap_out[i], push);
                so += sl.sbytes[i];
                sl.roff[i] = ro;
                sl.rbytes[i] = full && push ? fb_bins_bytes(full_coarse_bins(s->bounds, a, fs1), sl.cap_in[i]) : xbuf_bytes(sl.cap_in[i], push);
                ro += sl.rbytes[i];
            }
        if ((rc = dev_alloc_t(s, &sl.xsend, so)) || (rc = dev_alloc_t(s, &sl.xrecv, ro))) return rc;
        HIP_TRY(hipMemsetAsync(sl.xsend, 0, so ? so : 16, s->stream));
        HIP_TRY(hipMemsetAsync(sl.xrecv, 0, ro ? ro : 16, s->stream));
        if (full && push) {  // the own share's second parity (Slab::xown)
            size_t oo = 0;
            for (int h = 0; h < NH && h < FB_REGIONS; ++h) {
                sl.ooff[h] = oo;
                oo += sl.rbytes[(size_t)h * W + a];
            }
            if ((rc = dev_alloc_t(s, &sl.xown, oo))) return rc;
            HIP_TRY(hipMemsetAsync(sl.xown, 0, oo ? oo : 16, s->stream));
        }
        sl.overflow = &sl.S.ctl->overflow;
    }
    if (NH > 1) {  // the second stream and the events that order it with the compute stream
        HIP_TRY(hipStreamCreateWithFlags(&s->xstream, hipStreamNonBlocking));
        for (int h = 0; h < NH; ++h) {
            HIP_TRY(hipEventCreateWithFlags(&s->ev_send[h], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&s->ev_xfer[h], hipEventDisableTiming));
        }
    }
    return GP_OK;
}

// Kernel variant and grid for this run (measured defaults; GP_KERNEL / GP_XSEGS / GP_WALK /
// GP_WX / GP_WIDE override them in the experiments build).
void choose_kernel(gp_sim* s, int64_t nloc_max, int& kernel, uint32_t& col_xsegs, uint32_t& walk, uint32_t& wx,
                   uint32_t& wide) {
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, s->device);
    s->cus = std::max(1, prop.multiProcessorCount);
    const gp_config* cfg = &s->cfg;
    const int64_t g = s->g;
    int64_t blocks = (nloc_max + BULK_THREADS - 1) / BULK_THREADS;
    // 64 workgroups per CU: measured best for the tiled round kernels (tools/ablate.py:
    // 2048 -> 27.5, 8192 -> 22.1, 16384 -> 21.2 ms/round at P = 1e9)
    int64_t cap = (int64_t)prop.multiProcessorCount * 64;
    // (measured: gossip on a large lattice -> column march, profiles/r01; push-sum and
    // small lattices and line -> tiled; the push-sum column march was measured slower,
    // profiles/r03 and DESIGN.md §5.1)
    kernel = KERNEL_TILE;
    const bool lattice = cfg->topology == GP_3D || cfg->topology == GP_IMP3D;
    const bool push = cfg->algorithm == GP_PUSHSUM;
    if (lattice && g >= 200 && !push) kernel = KERNEL_COL;
    // 3D push-sum on one rank whose lattice fits the chip's LDS (C2: g = 100): one cooperative
    // launch per batch, the state resident in LDS (gp_block.hip)
    BlockPlan bp{};
    const bool block_ok = cfg->topology == GP_3D && push && s->world == 1 && g >= 2 &&
                          block_plan((uint32_t)g, prop.multiProcessorCount, bp) &&
                          block_plan_resident(bp, prop.multiProcessorCount);
    if (block_ok) kernel = KERNEL_BLOCK;
    if (const char* e = exp_env("GP_KERNEL")) {
        if (!std::strcmp(e, "tile")) kernel = KERNEL_TILE;
        else if (!std::strcmp(e, "col") && lattice && !push) kernel = KERNEL_COL;
        else if (!std::strcmp(e, "block") && block_ok) kernel = KERNEL_BLOCK;
    }
    s->bplan = bp;
    col_xsegs = 1;
    if (cfg->topology != GP_FULL && kernel == KERNEL_COL) {
        // gossip: exactly the resident grid (a persistent sweep), a multiple of the 8 XCDs
        cap = (int64_t)prop.multiProcessorCount * col_blocks_per_cu(cfg->topology, cfg->algorithm);
        // x segments per patch: enough work items for every resident wave, >= 16 planes each
        const int64_t patches = ((g + 63) / 64) * ((g + 3) / 4);
        const int64_t slots = cap * (BULK_THREADS / 64);
        const int64_t planes = std::max<int64_t>(1, g / s->world);
        int64_t xs = std::max<int64_t>(1, slots / std::max<int64_t>(1, patches));
        xs = std::min<int64_t>(xs, std::max<int64_t>(1, planes / 16));
        col_xsegs = (uint32_t)xs;
    }
    if (kernel == KERNEL_TILE)  // 1024-node tiles (+1: a slab may start mid-tile), a multiple of the 8 XCDs
        blocks = ((nloc_max + 1023) / 1024 + 1 + 7) / 8 * 8;
    if (const char* e = exp_env("GP_XSEGS")) col_xsegs = (uint32_t)std::max(1, std::atoi(e));
    s->grid = (int)std::max<int64_t>(1, std::min(kernel == KERNEL_COL ? cap : blocks, cap));
    // tile walk: x-windows of 8 planes once every XCD gets a few windows (measured,
    // profiles/r01: 18.2 -> 17.2 ms/round at P = 1e9), else XCD-contiguous eighths
    walk = (lattice && g / s->world >= 64) ? 2u : 0u;
    // push-sum: the same x-windows claimed from per-XCD counters on exactly the
    // resident grid (walk 3; measured, profiles/r02/walk3.txt)
    if (walk == 2 && kernel == KERNEL_TILE && cfg->algorithm == GP_PUSHSUM) walk = 3;
    // x-window of 8 planes (walk 2); 16 for walk 3 since round 4, where the wave priority
    // of the tile kernel moved the optimum: P = 1e9, same box, 8 / 12 / 16 / 24 / 32 planes
    // 13.34-13.36 / 13.17-13.28 / 13.17-13.22 / 13.22-13.25 / 13.15-13.17 ms/round
    // (profiles/r04/walk_window_nt.txt)
    wx = walk == 3 ? 16 : 8;
    if (const char* e = exp_env("GP_WALK")) walk = (uint32_t)std::atoi(e);
    if (const char* e = exp_env("GP_WX")) wx = (uint32_t)std::max(1, std::atoi(e));
    // size class of the tiled kernels: line / 3D push-sum on a slab with at most two tiles per
    // resident block of the 4-nodes-per-thread kernel (~2500 tiles, P <~ 2.6e6 per slab) runs the
    // 1024-thread, one-node-per-thread build (gp_ps_tile_wide.hip): its node phase is one memory
    // round trip per tile instead of four, which is what bounds a round with few tiles per block
    // (C2, 3D push-sum P = 1e6: 26.5 -> 20.7 us per round; line push-sum n = 1000: 10.2 -> 8.8).
    // Imp3D push-sum (its in-edge pass spills at 8 waves) and the gossip tile kernel measured
    // slower in that build at every size (profiles/r04/tile_size_class.txt)
    wide = 0;
    if (kernel == KERNEL_TILE && push && cfg->topology != GP_IMP3D) {
        const int topo = cfg->topology == GP_LINE ? LINE : cfg->topology == GP_3D ? GRID3D : IMP3D;
        const int64_t tiles = (nloc_max + 1023) / 1024 + 1;
        const int64_t res4 = ps_tile_resident_blocks(topo, s->world > 1 && topo == IMP3D, s->device);
        wide = res4 > 0 && tiles <= 2 * res4 ? 1u : 0u;
        if (const char* e = exp_env("GP_WIDE")) wide = e[0] == '1' ? 1u : 0u;
    }
    if (walk == 3) {
        const int topo = cfg->topology == GP_LINE ? LINE : cfg->topology == GP_3D ? GRID3D : IMP3D;
        const bool rem = s->world > 1 && topo == IMP3D;
        const int64_t res = (wide ? wide::ps_tile_resident_blocks(topo, rem, s->device)
                                  : ps_tile_resident_blocks(topo, rem, s->device)) / 8 * 8;
        if (res >= 8) s->grid = (int)std::min<int64_t>(s->grid, res);
        else walk = 2;
    }
}

// Everything after the handle exists: slabs, topology, initial state, round 0.
int build_sim(gp_sim* s) {
    int rc;
    if ((rc = make_bounds(s))) return rc;
    int64_t nloc_max = 0;
    for (int w = 0; w < s->world; ++w) nloc_max = std::max<int64_t>(nloc_max, s->bounds[w + 1] - s->bounds[w]);
    int kernel;
    uint32_t col_xsegs, walk, wx, wide;
    choose_kernel(s, nloc_max, kernel, col_xsegs, walk, wx, wide);
    const uint32_t rreg = round_regions(s, kernel, walk);
    if (s->mode == MODE_VIRTUAL) {
        s->slab.resize(s->world);
        for (int w = 0; w < s->world; ++w) s->slab[w].rank = w;
    } else {
        s->slab.resize(1);
        s->slab[0].rank = s->rank;
    }
    for (Slab& sl : s->slab) {
        sl.S.kernel = kernel;
        sl.S.tile_wide = wide;
        sl.S.col_xsegs = col_xsegs;
        sl.S.tile_walk = walk;
        sl.S.tile_wx = wx;
        sl.S.tile_stage_cap = 0xFFFFFFFFu;
        // single-rank lattice push-sum: the round kernel's last block closes the
        // round (no injector, nothing to exchange), saving a k_finalize launch per round
        // (2: arrivals sharded over 8 counters; a single counter -- 1, experiments
        // only -- serialises ~16k returning atomics per round: measured 1.93 vs
        // 0.40 ms/round at P = 2.7e7, profiles/r02/round_close.txt)
        sl.S.fuse_finalize = (s->mode == MODE_SINGLE && s->cfg.algorithm == GP_PUSHSUM &&
                              s->cfg.topology != GP_FULL) ? 2u : 0u;
        sl.S.bplan = s->bplan;
        sl.S.bface = sl.S.bscratch = nullptr;
        if (kernel == KERNEL_BLOCK) {  // face exchange buffers + barrier / accumulator scratch
            if ((rc = dev_alloc(s, &sl.S.bface, block_face_bytes(s->bplan))) || (rc = dev_alloc(s, &sl.S.bscratch, BLOCK_SCRATCH_BYTES)))
                return rc;
            HIP_TRY(block_kernel_setup(s->bplan));
        }
        if (const char* e = exp_env("GP_FUSE")) sl.S.fuse_finalize = sl.S.fuse_finalize ? (uint32_t)(e[0] - '0') : 0u;
        if (const char* e = exp_env("GP_STAGE_CAP")) sl.S.tile_stage_cap = (uint32_t)std::max(0, std::atoi(e));
#ifdef GP_EXPERIMENTS
        sl.S.tile_no_full = 0u;
        if (const char* e = exp_env("GP_NO_FULLTILE")) sl.S.tile_no_full = e[0] == '1' ? 1u : 0u;
#endif
        if ((rc = alloc_slab(s, sl, sl.rank))) return rc;
        sl.S.rregions = rreg;
        if (sl.S.tile_walk == 3) {  // the tile list of the per-XCD queues
            std::vector<uint32_t> list;
            if (!build_walk_list(sl.S, (int)sl.S.rregions, list, sl.S.woff)) {
                set_err("internal: walk-3 tile list does not cover the slab");
                return GP_EINVAL;
            }
            if ((rc = dev_alloc_t(s, &sl.S.wtiles, list.size() + 1))) return rc;
            HIP_TRY(hipMemcpy(sl.S.wtiles, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice));
        }
    }
    if (s->cfg.topology == GP_IMP3D && (rc = build_imp3d(s))) return rc;
    if ((s->cfg.topology == GP_IMP3D || s->cfg.topology == GP_FULL) && s->world > 1 && (rc = setup_exchange(s)))
        return rc;
    if ((rc = setup_halo(s))) return rc;
    if (s->world > 1) build_transfers(s);
    if (hipHostMalloc((void**)&s->host_ctl, sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
        set_err("hipHostMalloc failed");
        return GP_ENOMEM;
    }
    Ctl& init = *s->host_ctl;
    std::memset(&init, 0, sizeof init);
    init.active_total = 1;  // the seed
    init.all_active = s->P <= 1 ? 1u : 0u;
    init.inj_target = -1;
    init.inj_pick = -1;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        HIP_TRY(hipMemcpyAsync(S.ctl, &init, sizeof(Ctl), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(launch_init(S, s->grid, s->stream));
        if (S.topo == IMP3D)
            HIP_TRY(col_gossip_counts(S) ? launch_col_seed_init(S, s->stream) : launch_rbits_init(S, s->grid, s->stream));
        if (S.alg == GOSSIP && S.topo != FULL) HIP_TRY(launch_injector_init(S, s->grid, s->stream));
    }
    if ((rc = exchange(s, 0))) return rc;     // halos and random edges of round 0
    if ((rc = finalize(s, 0, 0))) return rc;  // prepare round 0
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        set_err("initialisation failed: %s", hipGetErrorString(e));
        return GP_EHIP;
    }
    if (s->timing) {
        s->ev.resize((size_t)2 * BATCH * round_launches(s));
        for (auto& x : s->ev) HIP_TRY(hipEventCreate(&x));
    }
    return GP_OK;
}

}  // namespace

int create_common(const gp_config* cfg, int mode, int world, int rank, const uint8_t* uid, gp_sim** out) {
    if (!cfg || !out) {
        set_err("gp_create: null argument");
        return GP_EINVAL;
    }
    *out = nullptr;
    if (cfg->algorithm != GP_GOSSIP && cfg->algorithm != GP_PUSHSUM) {
        set_err("option invalid: algorithm id %d", cfg->algorithm);
        return GP_EINVAL;
    }
    int64_t P, T, g;
    int rc = gp_resolve(cfg->num_nodes, cfg->topology, &P, &T, &g);
    if (rc) return rc;
    if ((rc = check_device(cfg->device))) return rc;
    gp_sim* s = new gp_sim();
    s->cfg = *cfg;
    s->device = cfg->device;
    s->P = P;
    s->T = T;
    s->g = g;
    s->mode = mode;
    s->world = world;
    s->rank = rank;
    s->timing = (cfg->flags & GP_FLAG_KERNEL_TIMING) != 0;
    if (hipSetDevice(s->device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        set_err("hipSetDevice/hipStreamCreate failed on device %d", s->device);
        gp_destroy(s);
        return GP_EHIP;
    }
    if (mode == MODE_RCCL) {
        ncclUniqueId id;
        std::memcpy(id.internal, uid, NCCL_UNIQUE_ID_BYTES);
        ncclResult_t r = ncclCommInitRank(&s->comm, world, id, rank);
        if (r != ncclSuccess) {
            set_err("ncclCommInitRank(rank %d of %d) failed: %s", rank, world, ncclGetErrorString(r));
            s->comm = nullptr;
            gp_destroy(s);
            return GP_ENCCL;
        }
    }
    rc = build_sim(s);
    if (rc) {
        const std::string msg = g_err;
        gp_destroy(s);
        g_err = msg;
        return rc;
    }
    *out = s;
    return GP_OK;
}
