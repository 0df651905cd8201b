// gp_exchange.hip -- one synchronous round (launch_round, for gp_step's batch loop): the round
// kernel(s), the inter-rank exchange and the finalize kernel(s).
//
// Sharding: contiguous node-id slabs, plane-aligned for 3D / Imp3D.  Each slab's
// node arrays carry one halo plane (line: one node) per neighbouring slab.  After every round
// the halos are refreshed from the neighbours and the Imp3D random-edge messages are exchanged
// (gp_xchg.hip); the round's alert / activation / injector counts are summed over ranks.
// Two transports: RCCL between processes (one process per GPU, gp_create_rank), and in-process
// "virtual ranks" on one device (gp_config.flags GP_FLAG_VIRTUAL_RANKS), which run the same
// kernels and exchange plan with device copies -- the single-GPU test bed of the multi-GPU
// path.  Both move what one list per slab and region describes (build_transfers, run_transfers).
#include "gp_host.hpp"

// Every inter-rank transfer of a round, described once per slab from its layout tables
// (alloc_slab, setup_exchange, setup_halo, build_lists, build_bits; gp_plan.hpp): Slab::xhalo[b] the halo
// planes and Slab::xplan[b][h] region h's messages of the round whose state lies in buffers b
// (the pointers depend on the round through its parity only), in the order they are issued:
//   1. the halo node bytes, lower neighbour then upper;
//   2. with them the halo (s, w): compacted (hsend / hrecv, setup_halo) or the full planes;
//   3. per peer the payload of the run's exchange kind (kplan.xkind): its bitmap chunk; or its
//      list's header words, then messages; or its slot / bin buffer.
// The k-th send of rank a to rank d is the k-th receive d posts from a: RCCL matches them
// by that order, and in-process ranks check it (run_transfers).
void build_transfers(gp_sim* s) {
    const int W = s->world, NH = s->xhalves;
    const uint32_t H = s->halo;
    const bool push = s->cfg.algorithm == GP_PUSHSUM;
    const size_t HS = s->halo_slots, sw_bytes = (HS ? HS : H) * 16;
    auto add = [](std::vector<Xfer>& v, bool send, int peer, auto* ptr, size_t bytes) {  // (nothing to move: no entry)
        if (bytes) v.push_back(Xfer{send, peer, reinterpret_cast<uint8_t*>(ptr), bytes});
    };
    for (Slab& sl : s->slab)
        for (int b = 0; b < 2; ++b) {
            DevState& S = sl.S;
            const int r = sl.rank;
            std::vector<Xfer>& halo = sl.xhalo[b];
            for (int k = 0; k < 2 && H; ++k) {  // my first H ids <-> lower neighbour's last H ids; my last <-> upper's first
                const int p = k == 0 ? r - 1 : r + 1;
                if (p < 0 || p >= W) continue;
                // my plane that travels and the halo plane that receives, from the node arrays' base
                const uint32_t out = (k == 0 ? S.lo : sl.hi - H) - S.base, in = (k == 0 ? S.lo - H : sl.hi) - S.base;
                add(halo, true, p, S.nb[b] + out, H);
                add(halo, false, p, S.nb[b] + in, H);
                if (!push) continue;
                add(halo, true, p, HS ? sl.hsend[k] : S.sw[b] + out, sw_bytes);
                add(halo, false, p, HS ? sl.hrecv[k] : S.sw[b] + in, sw_bytes);
            }
            uint8_t* xr = sl.xrecv + (size_t)b * sl.xl.xr_stride;  // lists: this round parity's receive buffer
            sl.xplan[b].assign(NH, {});
            for (int h = 0; h < NH; ++h)
                for (int p = 0; p < W; ++p) {
                    if (p == r) continue;
                    std::vector<Xfer>& v = sl.xplan[b][h];
                    const size_t i = (size_t)h * W + p;
                    switch (s->kplan.xkind) {
                    case XKind::None:  // (line / 3D: the halo planes are all that travels)
                        break;
                    case XKind::Bits:  // the bitmap chunks, each way
                        add(v, true, p, S.sbits + sl.bl.bo[p] / 32, (size_t)(sl.bl.bn[p] + 31) / 32 * 4);
                        add(v, false, p, sl.rbits_in + sl.bl.ro[p] / 32, (size_t)(sl.bl.rn[p] + 31) / 32 * 4);
                        break;
                    case XKind::Lists:  // header words, then messages, each way
                        add(v, true, p, sl.xsend + sl.xl.lhdr[i], (size_t)s->list_nw[((size_t)r * NH + h) * W + p] * 16);
                        add(v, true, p, sl.xsend + sl.xl.lval[i], (size_t)sl.xl.cap_out[i] * 16);
                        add(v, false, p, xr + sl.xl.rhdr[i], (size_t)s->list_nw[((size_t)p * NH + h) * W + r] * 16);
                        add(v, false, p, xr + sl.xl.rval[i], (size_t)sl.xl.cap_in[i] * 16);
                        break;
                    case XKind::Slots:     // slot buffers (gossip)
                    case XKind::FullBins:  // coarse bins (full push-sum)
                        add(v, true, p, sl.xsend + sl.xl.soff[i], sl.xl.sbytes[i]);
                        add(v, false, p, sl.xrecv + sl.xl.roff[i], sl.xl.rbytes[i]);
                        break;
                    }
                }
        }
}

namespace {

XPeer xpeer(uint8_t* buf, size_t off, uint32_t cap) {
    XPeer p{};
    if (!cap) return p;
    uint8_t* b = buf + off;
    p.cnt = reinterpret_cast<uint32_t*>(b);
    p.slots = reinterpret_cast<uint32_t*>(b + XBUF_SLOTS_OFF);
    p.cap = cap;
    return p;
}

// The halo planes' compacted (s, w) of buffers b: pack (the slab's first / last plane, before the
// transfer) or expand (into the halo planes, after it).  Lower side: the first plane's senders
// toward x - 1 (direction 0) go down; the lower halo takes the neighbour's senders toward x + 1
// (direction 1).  The upper side the other way round.
int halo_pack_expand(gp_sim* s, int b, bool pack, hipStream_t st) {
    const uint32_t H = s->halo;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        for (int k = 0; k < 2; ++k) {
            if (!sl.hsend[k]) continue;
            // plane start: pack -- lo (k = 0) / hi - H; expand -- lo - H (k = 0) / hi
            const uint32_t at = pack ? (k == 0 ? S.lo : sl.hi - H) : (k == 0 ? S.lo - H : sl.hi);
            HaloArgs h{};
            h.nb = S.nb[b] + (at - S.base);
            h.sw = S.sw[b] + (at - S.base);
            h.buf = pack ? sl.hsend[k] : sl.hrecv[k];
            h.n = H;
            h.cap = s->halo_cap;
            h.dir = pack ? (k == 0 ? 0u : 1u) : (k == 0 ? 1u : 0u);
            h.overflow = sl.overflow ? sl.overflow : &S.ctl->overflow;
            HIP_TRY(pack ? launch_halo_pack(h, st) : launch_halo_expand(h, st));
        }
    }
    return GP_OK;
}

// Issues the transfers of round parity b on stream st: the halo planes' (Slab::xhalo) and / or
// region h's (Slab::xplan).  RCCL: one group with this rank's sends and receives in list order.
// In-process ranks: for every pair (a, d), a's k-th send to d is copied into d's k-th receive
// from a; the two lists were built independently, as two processes would build them, so a
// difference in count or size is an addressing error the RCCL path would have too.
int run_transfers(gp_sim* s, int b, int h, bool halo, bool payload, hipStream_t st) {
    const int part0 = halo ? 0 : 1, part1 = payload ? 2 : 1;  // parts [part0, part1): 0 halo planes, 1 region h
    auto list = [&](const Slab& sl, int part) -> const std::vector<Xfer>& {
        return part == 0 ? sl.xhalo[b] : sl.xplan[b][h];
    };
    if (s->mode == MODE_RCCL) {
        NCCL_TRY(ncclGroupStart());
        for (int part = part0; part < part1; ++part)
            for (const Xfer& x : list(s->slab[0], part)) {
                if (x.send) NCCL_TRY(ncclSend(x.ptr, x.bytes, ncclUint8, x.peer, s->comm, st));
                else NCCL_TRY(ncclRecv(x.ptr, x.bytes, ncclUint8, x.peer, s->comm, st));
            }
        NCCL_TRY(ncclGroupEnd());
        return GP_OK;
    }
    auto next = [](const std::vector<Xfer>& v, size_t i, bool send, int peer) {  // next such entry from i on
        while (i < v.size() && (v[i].send != send || v[i].peer != peer)) ++i;
        return i;
    };
    for (int part = part0; part < part1; ++part)
        for (const Slab& a : s->slab)
            for (const Slab& d : s->slab) {
                if (&a == &d) continue;
                const std::vector<Xfer>&out = list(a, part), &in = list(d, part);
                size_t i = next(out, 0, true, d.rank), j = next(in, 0, false, a.rank);
                for (int k = 0; i < out.size() || j < in.size(); ++k) {
                    const size_t sent = i < out.size() ? out[i].bytes : 0, expected = j < in.size() ? in[j].bytes : 0;
                    if (sent != expected) {
                        set_err("internal: transfer %d -> %d, %s %d, index %d: %zu bytes sent, %zu expected", a.rank, d.rank,
                                part == 0 ? "halo planes with region" : "region", h, k, sent, expected);
                        return GP_EINVAL;
                    }
                    HIP_TRY(hipMemcpyAsync(in[j].ptr, out[i].ptr, sent, hipMemcpyDeviceToDevice, st));
                    i = next(out, i + 1, true, d.rank);
                    j = next(in, j + 1, false, a.rank);
                }
            }
    return GP_OK;
}

FullArgs make_full_args(gp_sim* s, Slab& sl, uint32_t round) {
    DevState& S = sl.S;
    const int cur = round & 1;
    const bool push = S.alg == PUSHSUM;
    const uint32_t d = S.lo - S.base;  // node arrays start at `base`; index these by id - lo
    FullArgs a{};
    a.nb = push ? S.nb[0] + d : nullptr;
    a.swc = push ? S.sw[cur] + d : nullptr;
    a.swn = push ? S.sw[cur ^ 1] + d : nullptr;
    a.c = S.c;
    a.inc = S.inc;
    a.ctl = S.ctl;
    a.overflow = sl.overflow;
    a.P = S.G.P;
    a.lo = S.lo;
    a.nloc = S.nloc;
    a.k0 = S.k0;
    a.k1 = S.k1;
    a.seed_node = S.seed_node;
    a.W = s->world;
    a.me = sl.rank;
    for (int w = 0; w <= s->world; ++w) a.bounds[w] = s->bounds[w];
    for (int p = 0; p < s->world; ++p) {
        a.peer[p] = xpeer(sl.xsend, sl.xl.soff[p], sl.xl.cap_out[p]);
        a.rpeer[p] = xpeer(sl.xrecv, sl.xl.roff[p], sl.xl.cap_in[p]);
    }
    return a;
}

// Push-sum on the full topology, one rank of several (gp_fullbin.hip): this
// rank's receivers [lo, lo + nloc), node arrays indexed by id - lo; exchange region h:
// the fold's tiles and senders (full_region), the bins it sends to every rank (out;
// its own share into its own receive region) and the bins received from every rank (in).
// This rank's own share of region h's bins, round parity `par` (Slab::xown).
FbBins own_bins(gp_sim* s, Slab& sl, int h, uint32_t par) {
    const size_t i = (size_t)h * s->world + sl.rank;
    uint8_t* base = par & 1u ? sl.xown + sl.xl.ooff[h] : sl.xrecv + sl.xl.roff[i];
    return fb_bins_at(base, sl.S.fb_nb1, sl.xl.cap_in[i]);
}

// send_pass: round 0's send pass fills this round's own bins (the fold fills the next round's).
FullBinArgs make_fullbin_args(gp_sim* s, Slab& sl, uint32_t round, int h, bool send_pass = false) {
    DevState& S = sl.S;
    const int cur = round & 1;
    const uint32_t d = S.lo - S.base;
    const int W = s->world;
    FullBinArgs a{};
    a.swc = S.sw[cur] + d;
    a.swn = S.sw[cur ^ 1] + d;
    a.nb = S.nb[0] + d;
    a.ctl = S.ctl;
    a.overflow = sl.overflow;
    a.P = S.G.P;
    a.k0 = S.k0;
    a.k1 = S.k1;
    a.s1 = S.fb_s1;
    a.nb1 = S.fb_nb1;
    a.nb2 = S.fb_nb2;
    a.cap2 = S.fb_cap2;
    a.cnt2 = S.fb_cnt2;
    a.hdr2 = S.fb_hdr2;
    a.pay2 = S.fb_pay2;
    a.lo = S.lo;
    a.nloc = S.nloc;
    full_region(S.nloc, s->xhalves, h, a.t_lo, a.t_hi, a.s_lo, a.s_hi);
    a.fused = 1;
    a.W = W;
    a.me = sl.rank;
    for (int w = 0; w <= W; ++w) a.bounds[w] = s->bounds[w];
    const uint32_t item = full_bin_item_messages();
    a.in_item0[0] = 0;
    for (int p = 0; p < W; ++p) {
        const size_t i = (size_t)h * W + p;
        a.in[p] = p == sl.rank ? own_bins(s, sl, h, round) : fb_bins_at(sl.xrecv + sl.xl.roff[i], S.fb_nb1, sl.xl.cap_in[i]);
        a.out[p] = p == sl.rank ? own_bins(s, sl, h, send_pass ? round : round + 1)
                                : fb_bins_at(sl.xsend + sl.xl.soff[i], full_coarse_bins(s->bounds, p, S.fb_s1), sl.xl.cap_out[i]);
        a.in_item0[p + 1] = a.in_item0[p] + (sl.xl.cap_in[i] ? S.fb_nb1 * ((sl.xl.cap_in[i] + item - 1) / item) : 0u);
    }
    return a;
}

// Full topology on several ranks: one round (push-sum gp_fullbin.hip, gossip gp_full.hip).
// Push-sum (round 6): the messages of round r reach this rank as the coarse bins of its
// receivers in the exchange buffers of every region and source, where the split reads them;
// the fold then runs region by region, and region h's fold bins its tiles' round-(r+1)
// messages by destination rank and coarse bin straight into region h's buffers, which travel
// (exchange stream, one RCCL group) while the next region's fold runs.  Round 0's messages
// come from the send pass (only the seed sends).  Events order the streams; every RCCL
// operation is issued in one order on every rank (group region 0, 1, then the finalize
// all-reduce, which waits for the last group).
int launch_round_full_multi(gp_sim* s, uint32_t r, hipEvent_t e0, hipEvent_t e1) {
    const bool push = s->cfg.algorithm == GP_PUSHSUM;
    int rc;
    if (e0) HIP_TRY(hipEventRecord(e0, s->stream));
    if (push) {
        const int NH = s->xhalves;
        hipStream_t xs = s->xstream ? s->xstream : s->stream;
        auto send_region = [&](int h) -> int {  // region h's buffers to the exchange stream
            if (xs != s->stream) {
                HIP_TRY(hipEventRecord(s->ev_send[h], s->stream));
                HIP_TRY(hipStreamWaitEvent(xs, s->ev_send[h], 0));
            }
            int rc2;
            if ((rc2 = run_transfers(s, 0, h, false, true, xs))) return rc2;  // (buffers of either parity: list 0)
            if (xs != s->stream) HIP_TRY(hipEventRecord(s->ev_xfer[h], xs));
            return GP_OK;
        };
        // the counters this round fills, in one launch: the fine tiles', every region's send bins'
        // (their last transfer is done: finalize waited for it), the own next-round bins' (the
        // split of round r - 1 read them); round 0 also this round's own bins, for the send pass
        // (zero_send: the send bins alone -- round 0's send pass has used them once already)
        // at most: the fine tiles', and per region (NH = FB_REGIONS, exchange_regions) the bins to
        // each of W <= XMAXW ranks and the own bins of this parity
        static_assert(ZeroList::MAX >= 1 + FB_REGIONS * (XMAXW + 1), "a round's counter arrays fit the ZeroList");
        auto zero_counts = [&](bool zero_send) -> int {
            for (Slab& sl : s->slab) {
                ZeroList z{};
                bool fits = true;
                auto add = [&](uint32_t* p, uint32_t n) {
                    if (!p || !n) return;
                    if (z.k == ZeroList::MAX) {
                        fits = false;
                        return;
                    }
                    z.p[z.k] = p;
                    z.n[z.k++] = n;
                };
                if (!zero_send) add(sl.S.fb_cnt2, sl.S.fb_nb2);
                for (int h = 0; h < NH; ++h) {
                    const FullBinArgs a = make_fullbin_args(s, sl, r, h);
                    for (int p = 0; p < s->world; ++p)
                        if (p != sl.rank || !zero_send) add(a.out[p].cnt, a.out[p].nb);  // (own: next parity)
                    if (r == 0 && !zero_send) add(a.in[sl.rank].cnt, a.in[sl.rank].nb);
                }
                if (!fits) {
                    set_err("internal: more than %d counter arrays to clear per round", ZeroList::MAX);
                    return GP_EINVAL;
                }
                HIP_TRY(launch_zero_list(z, s->stream));
            }
            return GP_OK;
        };
        if ((rc = zero_counts(false))) return rc;
        if (r == 0) {  // round 0's messages: the send pass
            for (int h = 0; h < NH; ++h) {
                for (Slab& sl : s->slab) HIP_TRY(launch_full_bin_send_multi(make_fullbin_args(s, sl, r, h, true), r, s->stream));
                if ((rc = send_region(h))) return rc;
            }
        }
        for (int h = 0; h < NH; ++h) {  // region h's bins into the fine tiles once they are here
            if (xs != s->stream) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_xfer[h], 0));
            for (Slab& sl : s->slab) HIP_TRY(launch_full_bin_split_multi(make_fullbin_args(s, sl, r, h), r, s->stream));
        }
        if (r == 0 && (rc = zero_counts(true))) return rc;  // (the send pass's transfers are done)
        for (int h = 0; h < NH; ++h) {  // the fold, region by region; round r+1's messages travel behind it
            for (Slab& sl : s->slab)
                HIP_TRY(launch_full_bin_fold_multi(make_fullbin_args(s, sl, r, h), r, s->cus, s->stream));
            if ((rc = send_region(h))) return rc;
        }
        if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
        if (xs != s->stream) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_xfer[NH - 1], 0));
        return finalize(s, r, r + 1);
    }
    for (Slab& sl : s->slab) {
        FullArgs a = make_full_args(s, sl, r);
        ZeroArgs z{};
        for (int p = 0; p < s->world; ++p) z.cnt[p] = a.peer[p].cnt;
        z.n = s->world;
        HIP_TRY(launch_zero_counts(z, s->stream));
        HIP_TRY(launch_fullm_gossip_send(a, r, s->grid, s->stream));
    }
    if ((rc = run_transfers(s, 0, 0, false, true, s->stream))) return rc;
    for (Slab& sl : s->slab) {
        FullArgs a = make_full_args(s, sl, r);
        HIP_TRY(launch_fullm_gossip_unpack(a, std::max(1, s->grid / 8), s->stream));
        HIP_TRY(launch_fullm_gossip_recv(a, s->grid, s->stream));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s->stream));
    return finalize(s, r, r + 1);
}

// Halo refresh + Imp3D random-edge exchange for round `rn`, whose state the
// previous round kernel has just written to buffers rn & 1.  What the random edges need is the
// run's exchange kind (kplan.xkind).  Lists (push-sum): k_list_pack writes header words +
// compacted messages, read in place by the next round kernel -- no unpack -- in s->xhalves
// regions: a region is packed and handed to the exchange stream, whose transfer overlaps the
// next region's packing.  Slots (gossip, tile kernel): k_pack writes {slot} entries, k_unpack
// tags the in-edges they name.  Bits (gossip, column kernel): the round kernel has set the
// bits; k_apply_bits counts the received ones.  None (line / 3D): halo planes only.  Events
// order the streams, so every rank issues its RCCL groups in one order (region 0, 1, ...),
// before the finalize all-reduce on the compute stream.  exchange() = exchange_open,
// exchange_region for every region (halo planes in region 0's group), exchange_close;
// launch_round_regions runs the same pieces region by region behind the round kernel's
// launches (halo planes in the last group).
struct XchgCtx {
    XKind kind;
    int W, b, NH;
    bool push;
    hipStream_t xs;
    size_t HS;
    XchgCtx(const gp_sim* s, uint32_t rn) {
        kind = s->kplan.xkind;
        W = s->world;
        b = rn & 1;
        push = s->cfg.algorithm == GP_PUSHSUM;
        // Lists: the slab's regions; else 1 -- gossip has one region, line / 3D never set xhalves, and
        // the full topology (xhalves 2 for push-sum) never comes here: exchange() returns before
        NH = s->xhalves;
        xs = NH > 1 && s->xstream ? s->xstream : s->stream;
        HS = s->halo_slots;  // push-sum: the halo planes' (s, w) compacted (setup_halo)
    }
};

// The halo planes of round rn: compacted (s, w) packed; in-process ranks copy them here.
// cs: the stream of the packs.
int exchange_open(gp_sim* s, uint32_t rn, hipStream_t cs) {
    const XchgCtx x(s, rn);
    int rc;
    if (x.push && x.HS && (rc = halo_pack_expand(s, x.b, true, cs))) return rc;
    // in-process ranks: the halo planes by device copies (round kernel -> next round kernel)
    return s->mode == MODE_VIRTUAL ? run_transfers(s, x.b, 0, true, false, cs) : GP_OK;
}

// Lists: header words + compacted messages of a slab's region h (k_list_pack).
int pack_lists(Slab& sl, const XchgCtx& x, int h, hipStream_t cs) {
    const DevState& S = sl.S;
    const int W = x.W;
    HIP_TRY(hipMemsetAsync(sl.xcnt + (size_t)h * W, 0, sizeof(uint32_t) * W, cs));
    ListPackArgs la{};
    la.nbn = S.nb[x.b];
    la.swn = S.sw[x.b];
    la.xdr = sl.xdr;
    la.lwt = sl.lwt;
    la.gw = sl.gw;
    la.lo = S.lo;
    la.nloc = S.nloc;
    la.base = S.base;
    la.t0 = sl.tb[h];
    la.t1 = h + 1 == x.NH ? sl.nt : sl.tb[h + 1];
    la.W = W;
    la.me = sl.rank;
    for (int d = 0; d < W; ++d) {
        if (d == sl.rank) continue;
        const size_t i = (size_t)h * W + d;
        la.peer[d].hdr = reinterpret_cast<XHdr*>(sl.xsend + sl.xl.lhdr[i]);
        la.peer[d].vals = reinterpret_cast<double2*>(sl.xsend + sl.xl.lval[i]);
        la.peer[d].cnt = sl.xcnt + i;
        la.peer[d].cap = sl.xl.cap_out[i];
        la.peer[d].vbase = sl.xl.vbase[i];
    }
    la.overflow = sl.overflow;
    HIP_TRY(launch_list_pack(la, cs));
    return GP_OK;
}

// Slots: the {slot} entries of a slab's region h, per destination (k_pack).
int pack_slots(Slab& sl, const XchgCtx& x, int h, hipStream_t cs) {
    const DevState& S = sl.S;
    const int W = x.W;
    ZeroArgs z{};
    PackArgs pa{};
    pa.nbn = S.nb[x.b];
    pa.pos = sl.pos;
    pa.xdst = sl.xdst;
    pa.lo = S.lo;
    pa.nloc = S.nloc;
    xregion(S.lo, S.nloc, /* lists */ false, sl.tb, x.NH, h, pa.s_lo, pa.s_hi);
    pa.base = S.base;
    pa.W = W;
    pa.me = sl.rank;
    for (int p = 0; p < W; ++p) {
        const size_t i = (size_t)h * W + p;
        pa.peer[p] = xpeer(sl.xsend, sl.xl.soff[i], sl.xl.cap_out[i]);
        z.cnt[p] = pa.peer[p].cnt;
    }
    z.n = W;
    pa.overflow = sl.overflow;
    HIP_TRY(launch_zero_counts(z, cs));
    HIP_TRY(launch_pack(pa, cs));
    return GP_OK;
}

// Slots: region h's received entries tag the in-edges they name with round rn (k_unpack).
int unpack_slots(Slab& sl, const XchgCtx& x, int h, uint32_t rn, hipStream_t st) {
    UnpackArgs ua{};
    ua.rtag = sl.S.rtag;
    ua.nedges = sl.nedges;
    ua.W = x.W;
    ua.me = sl.rank;
    for (int p = 0; p < x.W; ++p) {
        const size_t i = (size_t)h * x.W + p;
        ua.peer[p] = xpeer(sl.xrecv, sl.xl.roff[i], sl.xl.cap_in[i]);
    }
    ua.overflow = sl.overflow;
    HIP_TRY(launch_unpack(ua, rn, st));
    return GP_OK;
}

// Region h of round rn's random-edge exchange: packed on the compute stream, then handed to the
// exchange stream (one RCCL group per region; the halo planes travel in region hg's group).
int exchange_region(gp_sim* s, uint32_t rn, int h, int hg, hipStream_t cs) {
    const XchgCtx x(s, rn);
    int rc;
    for (Slab& sl : s->slab) {
        if (x.kind == XKind::Lists && (rc = pack_lists(sl, x, h, cs))) return rc;
        if (x.kind == XKind::Slots && (rc = pack_slots(sl, x, h, cs))) return rc;
        // (Bits: set by the round kernel itself)
    }
    if (x.xs != s->stream) {
        HIP_TRY(hipEventRecord(s->ev_send[h], cs));
        HIP_TRY(hipStreamWaitEvent(x.xs, s->ev_send[h], 0));
    }
    // (in-process ranks have copied the halo planes on the packs' stream: exchange_open)
    if ((rc = run_transfers(s, x.b, h, s->mode == MODE_RCCL && h == hg, true, x.xs))) return rc;
    if (x.xs != s->stream) HIP_TRY(hipEventRecord(s->ev_xfer[h], x.xs));
    return GP_OK;
}

// After the last region: received bitmaps applied / entries unpacked, halo planes expanded.
int exchange_close(gp_sim* s, uint32_t rn) {
    const XchgCtx x(s, rn);
    int rc;
    // (the exchange stream runs the regions' transfers in order: after the last, all are here)
    if (x.xs != s->stream) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_xfer[x.NH - 1], 0));
    switch (x.kind) {
    case XKind::Bits:
        for (Slab& sl : s->slab) {
            // one rumour per received bit at its target, counted for round rn; then the send
            // bitmap is cleared for the next round kernel
            HIP_TRY(launch_apply_bits(sl.rbits_in, sl.bl.nbits_in / 32, sl.tgt, sl.S.rq[rn & 1], sl.S.rq8, s->stream));
            if (sl.bl.nbits_out) HIP_TRY(hipMemsetAsync(sl.S.sbits, 0, (size_t)sl.bl.nbits_out / 8, s->stream));
        }
        break;
    case XKind::Slots:
        for (int h = 0; h < x.NH; ++h)
            for (Slab& sl : s->slab)
                if ((rc = unpack_slots(sl, x, h, rn, s->stream))) return rc;
        break;
    default:  // Lists: read in place by the round kernel; None: nothing travelled but the halo planes
        break;
    }
    if (x.push && x.HS && (rc = halo_pack_expand(s, x.b, false, s->stream))) return rc;
    return GP_OK;
}

}  // namespace

int exchange(gp_sim* s, uint32_t rn) {
    if (s->world == 1 || s->cfg.topology == GP_FULL) return GP_OK;  // full: the exchange is inside the round
    const XchgCtx x(s, rn);
    int rc;
    if ((rc = exchange_open(s, rn, s->stream))) return rc;
    for (int h = 0; h < x.NH; ++h)
        if ((rc = exchange_region(s, rn, h, 0, s->stream))) return rc;
    return exchange_close(s, rn);
}

// Close round `round_done` (if round_next > 0) and prepare round `round_next`.
int finalize(gp_sim* s, uint32_t round_done, uint32_t round_next) {
    if (s->mode == MODE_SINGLE) {
        HIP_TRY(launch_finalize(s->slab[0].S, round_done, round_next, s->stream));
        return GP_OK;
    }
    for (Slab& sl : s->slab) HIP_TRY(launch_finalize_pre(sl.S, round_next, s->stream));
    if (s->mode == MODE_VIRTUAL) {
        SumArgs sa{};
        sa.W = (int)s->slab.size();
        for (int w = 0; w < sa.W; ++w) sa.ctl[w] = s->slab[w].S.ctl;
        HIP_TRY(launch_sum_xchg(sa, s->stream));
    } else {
        Ctl* c = s->slab[0].S.ctl;
        NCCL_TRY(ncclAllReduce(c->xchg, c->xchg, 4, ncclUint64, ncclSum, s->comm, s->stream));
    }
    for (Slab& sl : s->slab) HIP_TRY(launch_finalize_post(sl.S, round_done, round_next, s->stream));
    return GP_OK;
}

namespace {

// One round of Imp3D push-sum across ranks, region by region (DevState::rregions): the round
// kernel over region h's tiles, then region h's lists packed and handed to the exchange stream,
// whose transfer overlaps the next regions' round kernel launches; the halo planes (first and
// last region) travel in the last group.  The lists arrive in the other parity's receive buffer
// (Slab::xr_stride): this round's kernels still read theirs.  ev (kernel timing, else null):
// 2 NR events, ev[2h] / ev[2h + 1] around launch h (the round kernel time excludes the packs).
int launch_round_regions(gp_sim* s, uint32_t r, hipEvent_t* ev) {
    const uint32_t NR = s->slab[0].S.rregions;
    const uint32_t rn = r + 1;
    int rc;
    for (uint32_t h = 0; h < NR; ++h) {
        if (ev) HIP_TRY(hipEventRecord(ev[2 * h], s->stream));
        for (Slab& sl : s->slab) HIP_TRY(launch_round_tile_region(sl.S, r, h, s->grid, s->stream));
        if (ev) HIP_TRY(hipEventRecord(ev[2 * h + 1], s->stream));
        // (region h's pack on a stream of its own, beside launch h + 1: 2-5 % slower,
        // profiles/r05/rejected/pack_stream.txt)
        const hipStream_t cs = s->stream;
        if (h + 1 == NR && (rc = exchange_open(s, rn, cs))) return rc;
        if ((rc = exchange_region(s, rn, (int)h, (int)NR - 1, cs))) return rc;
    }
    if ((rc = exchange_close(s, rn))) return rc;
    return finalize(s, r, rn);
}

}  // namespace

// Round kernel launches per round the kernel timing brackets (DevState::rregions, else 1).
uint32_t round_launches(const gp_sim* s) { return std::max<uint32_t>(1u, s->slab[0].S.rregions); }

// One synchronous round r: round kernel(s), exchange, finalize.
// ev (kernel timing, else null): 2 * round_launches(s) events.
int launch_round(gp_sim* s, uint32_t r, hipEvent_t* ev) {
    if (s->slab[0].S.rregions > 1) return launch_round_regions(s, r, ev);
    const hipEvent_t e0 = ev ? ev[0] : nullptr, e1 = ev ? ev[1] : nullptr;
    if (s->cfg.topology == GP_FULL && s->world > 1) return launch_round_full_multi(s, r, e0, e1);
    for (size_t q = 0; q < s->slab.size(); ++q) {
        DevState& S = s->slab[q].S;
        if (q == 0 && e0) HIP_TRY(hipEventRecord(e0, s->stream));
        HIP_TRY(launch_bulk(S, r, s->grid, s->stream));
        if (q == 0 && e1) HIP_TRY(hipEventRecord(e1, s->stream));
    }
    int rc;
    if ((rc = exchange(s, r + 1))) return rc;
    if (s->slab[0].S.fuse_finalize) return GP_OK;  // the round kernel closed its own round
    return finalize(s, r, r + 1);
}
