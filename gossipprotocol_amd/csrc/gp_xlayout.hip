// gp_xlayout.hip -- the exchange buffers of a run over several ranks (setup_exchange, before
// round 0): every buffer's message capacity from the expected messages per round, then the
// layout gp_plan.hpp derives from them, allocated and cleared.
#include "gp_host.hpp"

// Fixed-capacity exchange buffers per rank pair: capacity = expected messages
// per round + 12 sigma + 64 (never more than the pair's random edges).  Push-sum
// exchanges cut each slab's senders into regions (kplan.xregions -> s->xhalves: the lists'
// tiles in XREGIONS or eight regions, the full topology's fine tiles in two), one buffer per
// pair and region, moved separately on the exchange stream so that one region's transfer
// overlaps the others' packing (full topology: launch_round_full_multi; Imp3D: exchange,
// launch_round_regions).  Gossip has one region.
int setup_exchange(gp_sim* s) {
    const int W = s->world;
    const XKind kind = s->kplan.xkind;
    const bool push = s->cfg.algorithm == GP_PUSHSUM;
    const bool full = s->cfg.topology == GP_FULL;
    for (Slab& sl : s->slab) sl.overflow = &sl.S.ctl->overflow;
    if (kind == XKind::Bits) {  // gossip column kernel: fixed-size bitmaps (build_bits)
        s->xhalves = 1;
        return GP_OK;
    }
    const int NH = s->kplan.xregions;
    s->xhalves = NH;
    std::vector<uint32_t> caps((size_t)NH * W * W, 0);  // caps[(h * W + a) * W + b]: a -> b, region h
    Scratch tmp_mem;
    double* mu = nullptr;
    unsigned long long* n = nullptr;
    HIP_TRY(tmp_mem.alloc(&mu, XMAXW));
    HIP_TRY(tmp_mem.alloc(&n, XMAXW));
    // full push-sum: the coarse bins of every destination travel as the exchange buffers
    // (FbBins, gp_fullbin.hpp); the coarse-bin size every rank uses
    const uint32_t fs1 = full && push ? full_bin_multi_s1(s->bounds.data(), W) : 0;
    if (full) {
        // every active sender picks a uniform target among P-1: a function of the slab bounds
        // only, so every rank computes the whole table
        for (int a = 0; a < W; ++a) {
            const uint32_t na = s->bounds[a + 1] - s->bounds[a];
            for (int h = 0; h < NH; ++h) {
                uint32_t t0, t1, s0, s1;
                full_region(na, NH, h, t0, t1, s0, s1);
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
                    caps[((size_t)h * W + a) * W + b] = full_pair_cap(s1 - s0, s->bounds[b + 1] - s->bounds[b], (uint32_t)s->P);
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
            xregion(S.lo, S.nloc, kind == XKind::Lists, sl.tb, NH, h, ea.s_lo, ea.s_hi);
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
                caps[((size_t)h * W + sl.rank) * W + b] = msg_capacity(hmu[b], (double)hn[b]);
            }
        }
    }
    if (s->exp.xcap)  // (GP_XCAP) tests: force tiny buffers (overflow handling)
        for (auto& c : caps) c = std::min(c, *s->exp.xcap);
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
    // the layout of every rank's buffers from the capacities (exchange_layout, gp_plan.hpp):
    // Imp3D push-sum sender-ordered lists (gp_xchg.hpp), gossip slot buffers (entries only: no
    // vals part), or full push-sum's coarse bins (own messages: straight to xrecv; the own
    // share's second parity: Slab::xown)
    int rc;
    for (Slab& sl : s->slab) {
        XLayout& L = sl.xl;
        if (!exchange_layout(kind, caps, s->list_nw, s->bounds, W, NH, sl.rank, sl.S.rregions, /* slot buffers' vals part */ false, L)) {
            set_err("internal: exchange vals region beyond 2^32 slots");
            return GP_EINVAL;
        }
        if ((rc = dev_alloc_t(s, &sl.xsend, L.send_bytes)) || (rc = dev_alloc_t(s, &sl.xrecv, L.recv_bytes))) return rc;
        if (kind == XKind::Lists && (rc = dev_alloc_t(s, &sl.xcnt, (size_t)NH * W))) return rc;
        HIP_TRY(hipMemsetAsync(sl.xsend, 0, L.send_bytes ? L.send_bytes : 16, s->stream));
        HIP_TRY(hipMemsetAsync(sl.xrecv, 0, L.recv_bytes ? L.recv_bytes : 16, s->stream));
        if (kind == XKind::Lists) {
            for (int k = 0; k < 2; ++k) {
                sl.S.xhdr[k] = reinterpret_cast<const XHdr*>(sl.xrecv + k * L.xr_stride);
                sl.S.xvals[k] = reinterpret_cast<const double2*>(sl.xrecv + k * L.xr_stride + L.hdr_in);
            }
            sl.S.xnv = L.xnv;
        }
        if (kind == XKind::FullBins) {
            if ((rc = dev_alloc_t(s, &sl.xown, L.own_bytes))) return rc;
            HIP_TRY(hipMemsetAsync(sl.xown, 0, L.own_bytes ? L.own_bytes : 16, s->stream));
        }
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
