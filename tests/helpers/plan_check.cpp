// Host-side evaluation of the multi-rank run plan (gp_plan.hpp is host-only): reads one query
// per line from standard input -- a name and its integer arguments (doubles as decimal text) --
// and prints one line per query, the results as integers; groups of a result are separated
// by " ; ".  Built by tests/test_plan.py with the host compiler; runs on the CPU.
//   K                                      the constants
//   bounds P g W cut(0 line, 1 full, 2 planes)      -> error halo bounds...
//   full_region nloc NH h                  -> t0 t1 s0 s1
//   multi_s1 W bounds...                   -> s1
//   multi_cap n s1 P | pair_cap na nb P | cap m limit
//   coarse_bins p s1 W bounds...           -> bins
//   bins_bytes nb cap                      -> hdr_off pay_off bytes
//   xbuf cap push                          -> vals_off bytes
//   bin_plan P fused                       -> s1 nb1 nb2 cap1 cap2
//   tiles_for lo nloc
//   region_tiles lo nloc g2 NR             -> ok rb[0..NR]
//   list_region_tiles lo nloc g2 NH        -> tb[0..XMAXH]
//   xregion lo nloc lists NH h tb[0..XMAXH]  -> s_lo s_hi
//   exchange_regions push imp3d W bounds...
//   round_regions g2 NH W bounds...        -> on fit
//   halo_cap g imp3d | halo_slots n cap
//   chunk W NH b h a size[hh * W + aa]...  -> offset
//   list_tables nt W NH tb[0..XMAXH] hc... -> ok bad_d bad_words ; gw ; lwt ; nw
//   bits me W n[a * W + b]...              -> ok nbits_out nbits_in ; bo ; bn ; ro ; rn
//   layout kind(0 lists, 1 slots, 2 bins) W NH a rregions push bounds... caps... list_nw...
//       -> ok send recv own hdr_in xr_stride xnv ; cap_out ; cap_in ; soff ; sbytes ; roff ;
//          rbytes ; ooff ; lhdr ; lval ; rhdr ; rval ; vbase
//   xkind topology algorithm world kernel  -> XKind (0 none, 1 lists, 2 bits, 3 slots, 4 bins)
//   walk lo nloc g2 wx NR                  -> ok ; woff[h][0..8]... ; list
//   kernel_plan topo alg P g W mode  cus col_blocks_per_cu res4 res_wide block_resident
//               kernel xsegs walk wx wide rregions xregions fuse stage_cap no_full grid
//       (gp_kernel_plan.hpp; the overrides as parsed, "-" for one not set, grid as its text; the
//       facts are what the device queries would answer, and gather_kernel_facts picks from them)
//       -> bad_grid grid_max ; kernel col_xsegs walk wx wide grid rregions fuse_finalize
//          stage_cap no_full xregions grid_override ; bplan ; queries made (block, col, res4, wide)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../gossipprotocol_amd/csrc/gp_kernel_plan.hpp"

using namespace gp;

template <typename V>
static void put(const V& v, bool sep = true) {
    if (sep) std::printf(" ;");
    for (auto x : v) std::printf(" %llu", (unsigned long long)x);
}

static std::vector<uint32_t> take(std::istringstream& in, size_t n) {
    std::vector<uint32_t> v(n);
    for (auto& x : v) in >> x;
    return v;
}

int main() {
    std::string line, q;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> q)) continue;
        std::printf("%s", q.c_str());
        if (q == "K") {
            std::printf(" %d %d %u %u %d %d %u %u %d %d %zu %d %d %u %u", XMAXW, XMAXH, XTILE, HALO_CHUNK, RREG_MAX, XREGIONS,
                        RREG_MIN_NODES, BITS_ALIGN, FB_TB, FB_CAP2, FB_JUNK, FB_REGIONS, FB_MAXBINS, FBF_MAXB1, FBM_KEYS);
        } else if (q == "bounds") {
            long long P, g;
            int W, cut;
            in >> P >> g >> W >> cut;
            std::vector<uint32_t> b;
            uint32_t halo = 0;
            const BoundsError e = slab_bounds(P, g, W, cut == 0 ? SlabCut::Line : cut == 1 ? SlabCut::Full : SlabCut::Planes, b, halo);
            std::printf(" %d %u", (int)e, halo);
            put(b, false);
        } else if (q == "full_region") {
            uint32_t nloc, t0, t1, s0, s1;
            int NH, h;
            in >> nloc >> NH >> h;
            full_region(nloc, NH, h, t0, t1, s0, s1);
            std::printf(" %u %u %u %u", t0, t1, s0, s1);
        } else if (q == "multi_s1") {
            int W;
            in >> W;
            const std::vector<uint32_t> b = take(in, W + 1);
            std::printf(" %u", full_bin_multi_s1(b.data(), W));
        } else if (q == "multi_cap") {
            uint32_t n, s1, P;
            in >> n >> s1 >> P;
            std::printf(" %u", full_bin_multi_cap(n, s1, P));
        } else if (q == "pair_cap") {
            uint32_t na, nb, P;
            in >> na >> nb >> P;
            std::printf(" %u", full_pair_cap(na, nb, P));
        } else if (q == "cap") {
            double m, limit;
            in >> m >> limit;
            std::printf(" %u", msg_capacity(m, limit));
        } else if (q == "coarse_bins") {
            int p, W;
            uint32_t s1;
            in >> p >> s1 >> W;
            std::printf(" %u", full_coarse_bins(take(in, W + 1), p, s1));
        } else if (q == "bins_bytes") {
            uint32_t nb, cap;
            in >> nb >> cap;
            std::printf(" %zu %zu %zu", fb_bins_hdr_off(nb), fb_bins_pay_off(nb, cap), fb_bins_bytes(nb, cap));
        } else if (q == "xbuf") {
            uint32_t cap;
            int push;
            in >> cap >> push;
            std::printf(" %zu %zu", xbuf_vals_off(cap), xbuf_bytes(cap, push != 0));
        } else if (q == "bin_plan") {
            uint32_t P;
            int fused;
            in >> P >> fused;
            const FullBinPlan p = full_bin_plan(P, fused != 0);
            std::printf(" %u %u %u %u %u", p.s1, p.nb1, p.nb2, p.cap1, p.cap2);
        } else if (q == "tiles_for") {
            uint32_t lo, nloc;
            in >> lo >> nloc;
            std::printf(" %u", tiles_for(lo, nloc));
        } else if (q == "region_tiles") {
            uint32_t lo, nloc;
            uint64_t g2;
            int NR;
            in >> lo >> nloc >> g2 >> NR;
            std::vector<uint32_t> rb(NR + 1, 0);
            std::printf(" %d", region_tiles(lo, nloc, g2, NR, rb.data()) ? 1 : 0);
            put(rb, false);
        } else if (q == "list_region_tiles") {
            uint32_t lo, nloc;
            uint64_t g2;
            int NH;
            in >> lo >> nloc >> g2 >> NH;
            std::vector<uint32_t> tb(XMAXH + 1, 0);
            list_region_tiles(lo, nloc, g2, NH, tb.data());
            put(tb, false);
        } else if (q == "xregion") {
            uint32_t lo, nloc, s_lo, s_hi;
            int lists, NH, h;
            in >> lo >> nloc >> lists >> NH >> h;
            const std::vector<uint32_t> tb = take(in, XMAXH + 1);
            xregion(lo, nloc, lists != 0, tb.data(), NH, h, s_lo, s_hi);
            std::printf(" %u %u", s_lo, s_hi);
        } else if (q == "exchange_regions") {
            int push, imp3d, W;
            in >> push >> imp3d >> W;
            std::printf(" %d", exchange_regions(push != 0, imp3d != 0, W, take(in, W + 1)));
        } else if (q == "round_regions") {
            uint64_t g2;
            int NH, W;
            in >> g2 >> NH >> W;
            const std::vector<uint32_t> b = take(in, W + 1);
            std::printf(" %d %d", round_regions_on(W, b) ? 1 : 0, round_regions_fit(W, b, g2, NH) ? 1 : 0);
        } else if (q == "halo_cap") {
            uint32_t g;
            int imp3d;
            in >> g >> imp3d;
            std::printf(" %u", halo_chunk_cap(g, imp3d != 0));
        } else if (q == "halo_slots") {
            uint32_t n, cap;
            in >> n >> cap;
            std::printf(" %zu", halo_buf_slots(n, cap));
        } else if (q == "chunk") {
            int W, NH, b, h, a;
            in >> W >> NH >> b >> h >> a;
            const std::vector<uint32_t> size = take(in, (size_t)NH * W);
            std::printf(" %llu", (unsigned long long)chunk_offset(W, NH, b, h, a, [&](int hh, int aa) { return size[(size_t)hh * W + aa]; }));
        } else if (q == "list_tables") {
            uint32_t nt;
            int W, NH;
            in >> nt >> W >> NH;
            const std::vector<uint32_t> tb = take(in, XMAXH + 1), hc = take(in, (size_t)nt * W);
            std::vector<uint32_t> gw, nw((size_t)NH * W, 0);
            std::vector<uint8_t> lwt;
            int bad_d = 0;
            uint64_t bad_words = 0;
            const bool ok = list_tables(hc, nt, W, NH, tb.data(), gw, lwt, nw.data(), bad_d, bad_words);
            std::printf(" %d %d %llu", ok ? 1 : 0, bad_d, (unsigned long long)bad_words);
            put(gw);
            put(lwt);
            put(nw);
        } else if (q == "bits") {
            int me, W;
            in >> me >> W;
            std::vector<std::vector<uint32_t>> n(W);
            for (auto& row : n) row = take(in, W);
            BitsLayout L;
            const bool ok = bits_layout(n, me, L);
            std::printf(" %d %u %u", ok ? 1 : 0, L.nbits_out, L.nbits_in);
            put(L.bo);
            put(L.bn);
            put(L.ro);
            put(L.rn);
        } else if (q == "layout") {
            int kind, W, NH, a, push;
            uint32_t rregions;
            in >> kind >> W >> NH >> a >> rregions >> push;
            const std::vector<uint32_t> bounds = take(in, W + 1), caps = take(in, (size_t)NH * W * W);
            const std::vector<uint32_t> nw = take(in, kind == 0 ? (size_t)W * NH * W : 0);
            XLayout L;
            const bool ok = exchange_layout(kind == 0 ? XKind::Lists : kind == 1 ? XKind::Slots : XKind::FullBins, caps, nw, bounds,
                                            W, NH, a, rregions, push != 0, L);
            std::printf(" %d %zu %zu %zu %zu %zu %u", ok ? 1 : 0, L.send_bytes, L.recv_bytes, L.own_bytes, L.hdr_in, L.xr_stride,
                        L.xnv);
            put(L.cap_out);
            put(L.cap_in);
            put(L.soff);
            put(L.sbytes);
            put(L.roff);
            put(L.rbytes);
            put(std::vector<size_t>(L.ooff, L.ooff + FB_REGIONS));
            put(L.lhdr);
            put(L.lval);
            put(L.rhdr);
            put(L.rval);
            put(L.vbase);
        } else if (q == "xkind") {
            RunShape r;
            int kernel;
            in >> r.topology >> r.algorithm >> r.world >> kernel;
            std::printf(" %d", (int)exchange_kind(r, kernel));
        } else if (q == "walk") {
            uint32_t lo, nloc, wx;
            uint64_t g2;
            int NR;
            in >> lo >> nloc >> g2 >> wx >> NR;
            std::vector<uint32_t> list;
            uint32_t woff[RREG_MAX][9] = {};
            const bool ok = NR <= RREG_MAX && build_walk_list(lo, nloc, g2, wx, NR, list, woff);
            std::printf(" %d ;", ok ? 1 : 0);
            for (int h = 0; h < NR && h < RREG_MAX; ++h)
                for (int c = 0; c <= 8; ++c) std::printf(" %u", woff[h][c]);
            put(list);
        } else if (q == "kernel_plan") {
            RunShape r;
            long long P;
            KernelFacts have;
            int block = 0;
            in >> r.topology >> r.algorithm >> P >> r.g >> r.world >> r.mode >> have.cus >> have.col_blocks_per_cu >>
                have.res4 >> have.res_wide >> block;
            have.block_resident = block != 0;
            uint32_t halo = 0;
            slab_bounds(P, r.g, r.world,
                        r.topology == RunShape::Full ? SlabCut::Full : r.topology == RunShape::Line ? SlabCut::Line : SlabCut::Planes,
                        r.bounds, halo);
            auto opt = [&](auto& field) {
                std::string tok;
                in >> tok;
                if (tok != "-") field = (typename std::decay_t<decltype(field)>::value_type)std::stoll(tok);
            };
            KernelOverrides ov;
            opt(ov.kernel), opt(ov.xsegs), opt(ov.walk), opt(ov.wx), opt(ov.wide), opt(ov.rregions), opt(ov.xregions);
            opt(ov.fuse), opt(ov.stage_cap), opt(ov.no_full);
            std::string grid;
            in >> grid;
            if (grid != "-") ov.grid = grid;
            struct Device {  // answers from `have`, counting what is asked
                const KernelFacts& have;
                int asked[4] = {};
                int cus() { return have.cus; }
                bool block_resident(const BlockPlan&, int) { return ++asked[0], have.block_resident; }
                int col_blocks_per_cu() { return ++asked[1], have.col_blocks_per_cu; }
                int res4() { return ++asked[2], have.res4; }
                int res_wide() { return ++asked[3], have.res_wide; }
            } dev{have};
            const KernelFacts f = gather_kernel_facts(r, ov, dev);
            KernelPlanError err;
            const KernelPlan p = kernel_plan(r, f, ov, err);
            std::printf(" %d %d ; %d %u %u %u %u %d %u %u %u %u %d %d ; %u %u %u %u %u %u ; %d %d %d %d", err.bad_grid ? 1 : 0,
                        err.grid_max, p.kernel, p.col_xsegs, p.walk, p.wx, p.wide, p.grid, p.rregions, p.fuse_finalize,
                        p.stage_cap, p.no_full, p.xregions, p.grid_override ? 1 : 0, p.bplan.nbx, p.bplan.nby, p.bplan.nbz,
                        p.bplan.vmax, p.bplan.fmax, p.bplan.lds, dev.asked[0], dev.asked[1], dev.asked[2], dev.asked[3]);
        } else {
            std::printf(" ?");
        }
        std::printf("\n");
    }
    return 0;
}
