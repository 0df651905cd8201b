// gp_topology.hip -- the Imp3D topology build (build_imp3d, before round 0): every node's random
// edge and the receiver-sorted in-lists; across ranks, what the random edges' exchange needs --
// the sender-ordered lists (build_lists), the gossip column kernel's bitmaps (build_bits) or the
// tile kernel's slots.  Launches, copies and allocations; the tables come from gp_plan.hpp.
#include "gp_host.hpp"

namespace {

uint32_t bits_for(uint64_t maxval) {
    uint32_t b = 1;
    while (b < 32 && (maxval >> b) != 0) ++b;
    return b;
}

// Imp3D push-sum over several ranks: the static list plan (gp_xchg.hpp) of every slab
// from the global random edges, the header-word counts of every chunk, and for this
// rank's slabs the tile table gw and every remote in-edge's list key (rk).  kk: a
// P-word scratch array; src: senders in receiver order (global); edge0: first global
// in-edge of every rank.
int build_lists(gp_sim* s, const uint32_t* rnd_all, uint32_t* kk, const uint32_t* src,
                const std::vector<uint32_t>& edge0) {
    const int W = s->world;
    const int NH = s->xhalves = s->kplan.xregions;
    s->list_nw.assign((size_t)W * NH * W, 0);
    std::vector<std::vector<uint32_t>> gw_all(W);
    std::vector<std::vector<uint8_t>> lwt_all(W);
    std::vector<std::array<uint32_t, XMAXH + 1>> tb(W);  // per slab: region tile boundaries
    Scratch tmp_mem;
    for (int a = 0; a < W; ++a) {
        const uint32_t lo = s->bounds[a], nloc = s->bounds[a + 1] - lo;
        const uint32_t nt = tiles_for(lo, nloc);
        list_region_tiles(lo, nloc, (uint64_t)s->g * s->g, NH, tb[a].data());
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
        int bad_d = 0;
        uint64_t bad_words = 0;
        if (!list_tables(hc, nt, W, NH, tb[a].data(), gw_all[a], lwt_all[a], &s->list_nw[(size_t)a * NH * W], bad_d,
                         bad_words)) {
            set_err("internal: random-edge list %d -> %d has %llu header words (limit 2^26)", a, bad_d,
                    (unsigned long long)bad_words);
            return GP_EINVAL;
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
            for (int b = 0; b < W; ++b) ka.hw[h][b] = b == a ? 0u : list_hw(s->list_nw, W, NH, b, h, a);
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
        sl.nt = tiles_for(S.lo, S.nloc);
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
    int rc;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        const int me = sl.rank;
        if (!bits_layout(n, me, sl.bl)) {
            set_err("internal: random-edge bitmaps beyond 2^31 bits");
            return GP_EINVAL;
        }
        const size_t so = sl.bl.nbits_out, ri = sl.bl.nbits_in;
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
            ea.bo[w] = sl.bl.bo[w];
            ea.ro[w] = sl.bl.ro[w];
        }
        HIP_TRY(launch_bits_ends(ea, s->grid, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}

}  // namespace

// Imp3D: draw rnd[] for every node (Program.fs:258-260), then a stable sort of
// (key(rnd[i]), i) by key gives every receiver's senders in ascending id order,
// and the exclusive scan of the per-receiver in-degrees the CSR offsets (in_off,
// in_src in id order).  Every rank builds the global order (it is
// deterministic; ranks own consecutive id ranges) and keeps its
// receivers' slice; with several ranks, what the run's exchange kind needs (kplan.xkind):
// Slots -- each local sender the position of its message in the destination's in-edge array
// (pos) and the destination (xdst); Lists -- build_lists; Bits -- build_bits.

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
    const XKind kind = s->kplan.xkind;
    if (kind == XKind::Slots || kind == XKind::Bits) {  // (the lists are keyed from the senders' side)
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
        const bool pack = !s->exp.no_pack.value_or(false);  // (GP_NO_PACK=1: force the unpacked (P > 2^30) path)
        if (S.alg == PUSHSUM && S.kernel == KERNEL_TILE && s->P <= (1ll << 30) && s->g >= 2 && pack) {
            if ((rc = dev_alloc_t(s, &S.in_srcd, (size_t)ne + 4))) return rc;
            if (ne) HIP_TRY(launch_pack_src_deg(S.in_src, S.in_srcd, ne, S.G, s->grid, s->stream));
        }
        S.ind4 = nullptr;
        if (S.alg == PUSHSUM && S.kernel == KERNEL_TILE) {
            if ((rc = dev_alloc_t(s, &S.ind4, ind4_bytes_for(S.lo, S.nloc)))) return rc;
            const uint32_t wide_at = s->exp.ind4_wide.value_or(15);  // in-degree >= 15: the tile reads in_off (gp_ps_tile.hip; GP_IND4_WIDE)
            HIP_TRY(launch_pack_ind4(S, wide_at, s->grid, s->stream));
        }
        if (kind == XKind::Slots) {
            // gossip tile kernel across ranks: every sender's {slot} entry and its destination
            // (k_pack), the in-edges' round tags (k_unpack)
            if ((rc = dev_alloc_t(s, &sl.xdst, (size_t)S.nloc + 64)) || (rc = dev_alloc_t(s, &sl.pos, S.nloc)) ||
                (rc = dev_alloc_t(s, &S.rtag, ne)))
                return rc;
            HIP_TRY(hipMemsetAsync(S.rtag, 0xFF, sizeof(uint32_t) * (ne ? ne : 1), s->stream));
            PosArgs pa{};
            pa.rnd = S.rnd;
            pa.inv = inv;
            pa.pos = sl.pos;
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
    if (kind == XKind::Lists && (rc = build_lists(s, rnd_all, iota, src_sorted, edge0))) return rc;
    // (counts, off_all -- copied into the slabs' in_off -- and iota are free again: the bitmaps'
    // scratch, in stream order after those copies)
    if (kind == XKind::Bits && (rc = build_bits(s, src_sorted, keys_sorted, inv, edge0, counts, off_all, iota)))
        return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}
