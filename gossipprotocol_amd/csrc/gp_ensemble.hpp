// gp_ensemble.hpp -- ensemble runs (gp_ensemble.hip): one workgroup simulates one
// whole small network in LDS, a grid of workgroups runs many seeds at once.
// This header is the LDS layout (and with it the population cap per pair) plus
// the host launch interface; DESIGN.md §9.
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
constexpr uint32_t ens_lds_bytes(int topo, int alg, uint32_t P, bool faults = false, bool trace = false) {
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
    if (faults) b += ens_up8(4 * ((P + 31) / 32));
    if (trace) b += ENS_LDS_TRACE;
    return b;
}

// Largest population a member may have: the LDS image fits and every node has a
// thread slot.  A compile-time function of the layout above.
constexpr uint32_t ens_max_population(int topo, int alg, bool faults = false, bool trace = false) {
    uint32_t P = (uint32_t)ENS_THREADS * ENS_NPT_MAX;
    while (P > 2 && ens_lds_bytes(topo, alg, P, faults, trace) > ENS_LDS_MAX) --P;
    return P;
}
static_assert(ens_max_population(IMP3D, PUSHSUM) >= 1001 && ens_max_population(FULL, PUSHSUM) >= 1001, "report range");
static_assert(ens_max_population(IMP3D, PUSHSUM, true) >= 1001 && ens_max_population(FULL, PUSHSUM, true) >= 1001,
              "report range, failure layout");
static_assert(ens_max_population(LINE, GOSSIP, false, true) >= 1001 && ens_max_population(LINE, PUSHSUM, false, true) >= 1001 &&
                  ens_max_population(FULL, GOSSIP, false, true) >= 1001 && ens_max_population(FULL, PUSHSUM, false, true) >= 1001 &&
                  ens_max_population(GRID3D, GOSSIP, false, true) >= 1001 && ens_max_population(GRID3D, PUSHSUM, false, true) >= 1001 &&
                  ens_max_population(IMP3D, GOSSIP, false, true) >= 1001 && ens_max_population(IMP3D, PUSHSUM, false, true) >= 1001,
              "report range, trace layout");
static_assert(ens_max_population(LINE, GOSSIP, true, true) >= 1001 && ens_max_population(LINE, PUSHSUM, true, true) >= 1001 &&
                  ens_max_population(FULL, GOSSIP, true, true) >= 1001 && ens_max_population(FULL, PUSHSUM, true, true) >= 1001 &&
                  ens_max_population(GRID3D, GOSSIP, true, true) >= 1001 && ens_max_population(GRID3D, PUSHSUM, true, true) >= 1001 &&
                  ens_max_population(IMP3D, GOSSIP, true, true) >= 1001 && ens_max_population(IMP3D, PUSHSUM, true, true) >= 1001,
              "report range, trace + failure layout");
static_assert((uint32_t)ENS_THREADS * ENS_NPT_MAX < ENS_NONE, "node ids must fit the 16-bit list links");

// Largest num_nodes: line / full P = n + 1; 3D / Imp3D the largest whole cube.
constexpr int64_t ens_max_nodes(int topo, int alg, bool faults = false, bool trace = false) {
    const uint32_t P = ens_max_population(topo, alg, faults, trace);
    if (topo == LINE || topo == FULL) return (int64_t)P - 1;
    uint32_t g = 1;
    while ((g + 1) * (g + 1) * (g + 1) <= P) ++g;
    return (int64_t)g * g * g;
}

// Kernel arguments.  rec[m] is member m's record (gp_member; `reserved` carries the
// injector's live count between launches); idx[b] is the member workgroup b runs.
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
};

// Failure model (SRS v1-F): Philox streams and the per-member record
// that persists between launches beside gp_member (whose `converged` carries the
// counted alerts).  D itself is never stored: a pure function of the seed.
constexpr uint32_t S_FAULT_NODE = 5, S_FAULT_DROP = 6;
struct EnsFaultRec {
    int64_t lost;    // messages sent that nobody received, all launches so far
    int64_t doomed;  // |D|
};
// Arguments of the failure kernels: the plain ones plus the failure parameters.  An
// event with threshold q happens iff (uint64) x < q, x the first Philox output word.
struct EnsFaultArgs {
    EnsArgs a;
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
// Arguments of the traced kernels: the plain / failure ones plus the trace.
struct EnsTraceArgs {
    EnsArgs a;
    EnsTrace t;
};
struct EnsTraceFaultArgs {
    EnsFaultArgs a;
    EnsTrace t;
};

// Raises the kernel's dynamic-LDS limit for population P; once per handle.
hipError_t ens_setup(int topo, int alg, uint32_t P);
// Plain launch, one workgroup per listed member.
hipError_t ens_launch(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st);
// The same two for the failure kernels (gp_ensemble_faults.hip).
hipError_t ens_faults_setup(int topo, int alg, uint32_t P);
hipError_t ens_faults_launch(int topo, int alg, const EnsFaultArgs& a, uint32_t nblocks, hipStream_t st);
// The same for the traced kernels (gp_ensemble_trace.hip), without and with the failure model.
hipError_t ens_trace_setup(int topo, int alg, uint32_t P, bool faults);
hipError_t ens_trace_launch(int topo, int alg, const EnsTraceArgs& a, uint32_t nblocks, hipStream_t st);
hipError_t ens_trace_launch(int topo, int alg, const EnsTraceFaultArgs& a, uint32_t nblocks, hipStream_t st);

}  // namespace gp
