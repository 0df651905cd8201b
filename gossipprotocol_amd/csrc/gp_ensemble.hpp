// gp_ensemble.hpp -- ensemble runs (gp_ensemble.hip): one workgroup simulates one
// whole small network in LDS, a grid of workgroups runs many seeds at once.
// This header is the variant descriptor, the LDS layout (and with it the population cap
// per pair and variant), the kernel arguments and the host launch interface; DESIGN.md §9.
#pragma once

#include <stdint.h>

#include "../../include/gossip_hip.h"
#include "gp_device.hpp"

namespace gp {

constexpr int ENS_THREADS = 1024;            // largest workgroup
constexpr int ENS_NPT_MAX = 8;               // push-sum: node slots a thread keeps in registers
constexpr uint32_t ENS_LDS_MAX = 150 * 1024; // dynamic LDS a member may ask for (a CU has 160 KiB)
constexpr uint32_t ENS_LDS_HDR = 16;         // [0] cumulative alerts, [1] injector live count;
                                             // failure kernels: [2] |D|, [3] messages lost in this launch
constexpr uint32_t ENS_NONE = 0xFFFFu;       // end of a receiver's message list (node ids are < 0xFFFF)

constexpr uint32_t ens_up8(uint32_t b) { return (b + 7u) & ~7u; }

// Which kernels run an ensemble: with the failure model, recording a trace.
struct EnsVariant {
    bool faults, trace;
};

// LDS image of one member, arrays in this order, each padded to 8 bytes:
//   gossip   : c int32[P], inc int32[P], rnd u16[P] (Imp3D), live bitmap u32[ceil(T/32)] (not full)
//   push-sum : hs f64[P], hw f64[P] (the halves a sender offers this round), head u32[P] + next u16[P]
//              (full, Imp3D: per-receiver list of this round's random-edge senders), rnd u16[P] (Imp3D),
//              dir u8[P] (not full)
// The per-node (s, w, flags) of push-sum live in registers (ENS_NPT_MAX slots per thread).
// The failure kernels (SRS v1-F, gp_ensemble_faults.hip) append
//   doomed bitmap u32[ceil(P/32)]: bit i set iff node i is in D
// to either image, redrawn from the seed at the start of every launch.
// The traced kernels (SRS v1-T, gp_ensemble_trace.hip) append after that
//   trace block, ENS_LDS_TRACE bytes (EnsTraceLds): the words a row is made of
constexpr uint32_t ENS_LDS_TRACE = 32;
constexpr uint32_t ens_lds_bytes(int topo, int alg, uint32_t P, EnsVariant v) {
    uint32_t b = ENS_LDS_HDR;
    if (alg == GOSSIP) {
        b += ens_up8(4 * P) * 2;
        if (topo == IMP3D) b += ens_up8(2 * P);
        if (topo != FULL) b += ens_up8(4 * ((P + 31) / 32));
    } else {
        b += 8 * P * 2;
        if (topo == FULL || topo == IMP3D) b += ens_up8(4 * P) + ens_up8(2 * P);
        if (topo == IMP3D) b += ens_up8(2 * P);
        if (topo != FULL) b += ens_up8(P);
    }
    if (v.faults) b += ens_up8(4 * ((P + 31) / 32));
    if (v.trace) b += ENS_LDS_TRACE;
    return b;
}

// Largest population a member may have: the LDS image fits and every node has a
// thread slot.  A compile-time function of the layout above.
constexpr uint32_t ens_max_population(int topo, int alg, EnsVariant v) {
    uint32_t P = (uint32_t)ENS_THREADS * ENS_NPT_MAX;
    while (P > 2 && ens_lds_bytes(topo, alg, P, v) > ENS_LDS_MAX) --P;
    return P;
}
// Every variant of every pair covers the report's range.
constexpr bool ens_covers_report_range() {
    for (int faults = 0; faults < 2; ++faults)
        for (int trace = 0; trace < 2; ++trace)
            for (int topo = LINE; topo <= IMP3D; ++topo)
                for (int alg = GOSSIP; alg <= PUSHSUM; ++alg)
                    if (ens_max_population(topo, alg, EnsVariant{faults != 0, trace != 0}) < 1001) return false;
    return true;
}
static_assert(ens_covers_report_range(), "report range");
static_assert((uint32_t)ENS_THREADS * ENS_NPT_MAX < ENS_NONE, "node ids must fit the 16-bit list links");

// Largest num_nodes: line / full P = n + 1; 3D / Imp3D the largest whole cube.
constexpr int64_t ens_max_nodes(int topo, int alg, EnsVariant v) {
    const uint32_t P = ens_max_population(topo, alg, v);
    if (topo == LINE || topo == FULL) return (int64_t)P - 1;
    uint32_t g = 1;
    while ((g + 1) * (g + 1) * (g + 1) <= P) ++g;
    return (int64_t)g * g * g;
}

// Failure model (SRS v1-F): Philox streams and the per-member record
// that persists between launches beside gp_member (whose `converged` carries the
// counted alerts).  D itself is never stored: a pure function of the seed.
constexpr uint32_t S_FAULT_NODE = 5, S_FAULT_DROP = 6;
struct EnsFaultRec {
    int64_t lost;    // messages sent that nobody received, all launches so far
    int64_t doomed;  // |D|
};
// The failure parameters.  An event with threshold q happens iff (uint64) x < q, x the
// first Philox output word.
struct EnsFaults {
    EnsFaultRec* frec;
    uint64_t q_node, q_drop;  // floor(p * 2^32); 2^32 = always
    int64_t fail_round;
};

// Node i in D?  (host: gp_ensemble_read_state; device: the bitmap redraw)
GP_HD bool ens_doomed(uint32_t k0, uint32_t k1, uint32_t i, uint32_t seed_node, uint64_t q_node) {
    uint32_t x, y;
    philox2(i, 0, S_FAULT_NODE, k0, k1, x, y);
    return i != seed_node && (uint64_t)x < q_node;
}

// Traces (SRS v1-T): a member that has just completed round R records row
// k = R / stride - 1 iff R % stride == 0 and k < capacity, at rows[m * capacity + k].
// The LDS trace block holds what a row is made of; `sent` alone has to outlive a launch
// and persists in the member's trace record, the way EnsFaultRec.lost does.
struct EnsTraceLds {
    unsigned long long sent;  // messages sent, all launches so far (threads flush into it before a row is taken)
    unsigned long long err;   // push-sum: largest |e| bit pattern of the recording round
    uint32_t reached;         // recounted at launch start, then kept incrementally
    uint32_t pad[3];
};
static_assert(sizeof(EnsTraceLds) == ENS_LDS_TRACE, "trace block");
struct EnsTraceRec {
    uint64_t sent;  // cumulative node-to-node messages sent, all launches so far
};
struct EnsTrace {
    gp_trace_row* rows;  // nseeds x capacity
    EnsTraceRec* trec;   // nseeds
    int64_t stride, capacity;
};

// Kernel arguments, the same block for every variant.  rec[m] is member m's record
// (gp_member; `reserved` carries the injector's live count between launches); idx[b] is
// the member workgroup b runs.  A kernel without the failure model never reads f, an
// untraced one never reads t.
struct EnsArgs {
    gp_member* rec;
    const uint32_t* idx;
    int32_t* c;      // gossip: nseeds x P rumour counters
    uint32_t* bits;  // gossip, not full: nseeds x nwords live bitmap of the injector
    double* s;       // push-sum: nseeds x P
    double* w;
    uint8_t* fl;     // push-sum: nseeds x P, bit0 active, bit1 converged, bits2-3 count
    Geom G;
    uint32_t nwords;
    int32_t init;        // 1: set the member up from its seed instead of loading it
    int64_t nrounds;     // rounds this launch may run
    int64_t max_rounds;  // cap on a member's total rounds
    EnsFaults f;
    EnsTrace t;
};

// The launch interface of one variant, defined in gp_ensemble_kernels.hpp and instantiated by
// gp_ensemble.hip (plain), gp_ensemble_faults.hip (failure) and gp_ensemble_trace.hip (both traced).
// Setup raises the kernel's dynamic-LDS limit for population P, once per handle; launch runs
// one workgroup per listed member.
template <bool FAULTS, bool TRACE>
hipError_t ens_setup_t(int topo, int alg, uint32_t P);
template <bool FAULTS, bool TRACE>
hipError_t ens_launch_t(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st);
// (extern: the dispatchers below must not instantiate every variant in every unit)
extern template hipError_t ens_setup_t<false, false>(int, int, uint32_t);
extern template hipError_t ens_setup_t<true, false>(int, int, uint32_t);
extern template hipError_t ens_setup_t<false, true>(int, int, uint32_t);
extern template hipError_t ens_setup_t<true, true>(int, int, uint32_t);
extern template hipError_t ens_launch_t<false, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<true, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<false, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<true, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);

inline hipError_t ens_setup(EnsVariant v, int topo, int alg, uint32_t P) {
    if (v.trace) return v.faults ? ens_setup_t<true, true>(topo, alg, P) : ens_setup_t<false, true>(topo, alg, P);
    return v.faults ? ens_setup_t<true, false>(topo, alg, P) : ens_setup_t<false, false>(topo, alg, P);
}
inline hipError_t ens_launch(EnsVariant v, int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st) {
    if (v.trace)
        return v.faults ? ens_launch_t<true, true>(topo, alg, a, nblocks, st)
                        : ens_launch_t<false, true>(topo, alg, a, nblocks, st);
    return v.faults ? ens_launch_t<true, false>(topo, alg, a, nblocks, st)
                    : ens_launch_t<false, false>(topo, alg, a, nblocks, st);
}

}  // namespace gp
