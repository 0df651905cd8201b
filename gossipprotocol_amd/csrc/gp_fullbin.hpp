// gp_fullbin.hpp -- full-topology push-sum rounds by two-level LDS binning
// (gp_fullbin.hip).  Not part of the C-ABI.  The bins' plan -- FB_* constants, FullBinPlan,
// full_bin_plan, full_bin_multi_s1 / _cap, fb_bins_bytes -- is host arithmetic: gp_plan.hpp.
#pragma once

#include "gp_xchg.hpp"

namespace gp {

// A set of `nb` coarse bins of `cap` messages each -- one rank's own coarse bins (cnt1 / hdr1 /
// pay1), or, across ranks, the coarse bins of one destination rank's receivers that one exchange
// region carries: [counts: nb u32 | pad to 16 B][sender ids: nb * cap u32 | pad][payloads:
// nb * cap (s / 2, w / 2)], one contiguous buffer (fb_bins_bytes / fb_bins_at), so it travels
// as one RCCL send with its counts in band.
struct FbBins {
    uint32_t* cnt;
    uint32_t* hdr;
    double2* pay;
    uint32_t cap;
    uint32_t nb;
};
FbBins fb_bins_at(uint8_t* base, uint32_t nb, uint32_t cap);

struct FullBinArgs {
    const double2* swc;  // (s, w) at round start
    double2* swn;        // (s, w) after the round
    uint8_t* nb;         // node byte (active / converged / count), single buffer
    Ctl* ctl;
    unsigned int* overflow;
    uint32_t P, k0, k1;
    uint32_t s1, nb1, nb2, cap1, cap2;
    uint32_t* cnt1;      // [nb1] messages per coarse bin (one rank; zeroed every round)
    uint32_t* cnt2;      // [nb2] messages per fine tile
    uint32_t* hdr1;      // [nb1 * cap1] sender id (the target is recomputed from its Philox draw)
    double2* pay1;       // [nb1 * cap1] {s / 2, w / 2}
    uint32_t* hdr2;      // [nb2 * cap2] sender id
    double2* pay2;
    // receivers of this rank: global ids [lo, lo + nloc) (one rank: 0, P); node
    // arrays (swc, swn, nb) are indexed by id - lo, coarse bins and fine tiles count
    // from lo
    uint32_t lo, nloc;
    uint32_t s_lo, s_hi;  // send pass: the senders lo + [s_lo, s_hi) (several ranks: one exchange region)
    uint32_t t_lo, t_hi;  // fold: the fine tiles [t_lo, t_hi) (several ranks: one exchange region's)
    uint32_t fused;       // one rank: the fold bins the next round's messages into hdr1 / pay1
    // several ranks: every rank's coarse bins have the size 2^s1, so a message to target t
    // has the key kb(b) + ((t - bounds[b]) >> s1), b = owner of t, kb(b) = the bins of the
    // ranks below b -- the LDS bins of the send pass and of the fold's send phase
    int W, me;
    uint32_t bounds[XMAXW + 1];
    FbBins out[XMAXW];   // this region's bins for rank b's receivers (b == me: its own receive region)
    FbBins in[XMAXW];    // the region's bins from rank p for this rank's receivers (after the exchange)
    uint32_t in_item0[XMAXW + 1];  // first split work item of each source rank
};

hipError_t launch_full_bin_round(const FullBinArgs& a, uint32_t round, int grid, hipStream_t st);
// several ranks: round 0's messages (senders [s_lo, s_hi)) into the exchange buffers ...
hipError_t launch_full_bin_send_multi(const FullBinArgs& a, uint32_t round, hipStream_t st);
// ... per round: the counters the round fills cleared in one launch (the fine tiles', every
// region's send bins', this rank's own next-round bins': ZeroList), each region's received bins
// split into this rank's fine tiles, and the fold of each region's tiles, which bins their
// next-round messages into the region's exchange buffers
struct ZeroList {
    // per slab and round: the fine tiles'; per region every rank's send bins' (the own share's
    // next parity among them) and, in round 0, the own share's this parity (zero_counts, gp_exchange.hip)
    static constexpr int MAX = 1 + FB_REGIONS * XMAXW + FB_REGIONS;
    uint32_t* p[MAX];
    uint32_t n[MAX];
    int k;
};
hipError_t launch_zero_list(const ZeroList& z, hipStream_t st);
hipError_t launch_full_bin_split_multi(const FullBinArgs& a, uint32_t round, hipStream_t st);
hipError_t launch_full_bin_fold_multi(const FullBinArgs& a, uint32_t round, int cus, hipStream_t st);
uint32_t full_bin_item_messages();
uint32_t full_bin_fused_max_bins();  // coarse bins the fused fold can bin into

}  // namespace gp
