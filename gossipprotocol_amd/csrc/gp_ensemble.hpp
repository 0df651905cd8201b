// gp_ensemble.hpp -- ensemble runs (gp_ensemble.hip): one workgroup simulates one
// whole small network in LDS, a grid of workgroups runs many seeds at once.
// This header is the kernel arguments and the host launch interface; the variant descriptor
// and the launch shape (LDS layout, population caps, slots, threads) are gp_ensemble_shape.hpp;
// DESIGN.md §9.
#pragma once

#include <stdint.h>

#include "../../include/gossip_hip.h"
#include "gp_device.hpp"
#include "gp_ensemble_shape.hpp"

namespace gp {

// The launch shape -- LDS layout, population caps, node slots and workgroup size -- is host-clean
// and lives in gp_ensemble_shape.hpp, written over the public enums:
static_assert(LINE == GP_LINE && FULL == GP_FULL && GRID3D == GP_3D && IMP3D == GP_IMP3D, "topology enums");
static_assert(GOSSIP == GP_GOSSIP && PUSHSUM == GP_PUSHSUM, "algorithm enums");
// A caller-supplied graph (SRS v1-G): a topology of the ensemble kernels alone.
constexpr int GRAPH = ENS_GRAPH;
static_assert(GRAPH == IMP3D + 1, "the graph follows the reference's four topologies");

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
    uint32_t pad;
    double mu;                // push-sum: what err is measured against (EnsArgs::mu), read where a row's errors are taken
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
    // push-sum, SRS v1-V (gp_ensemble_create_values): the initial (s, w) of every member, P doubles
    // each on the device; x0 null: s = id, w = 1; w0 null: every weight 1.  Read by the set-up launch only.
    const double* x0;
    const double* w0;
    double mu;  // TRACE: what err_max is measured against; (P - 1) / 2 unless values were given
    // GRAPH, SRS v1-G (gp_ensemble_create_graph): the out-CSR in the caller's order and, for push-sum, the
    // transposed, deduplicated in-CSR (gp_graph.hpp), on the device; every array padded to a multiple of
    // 8 bytes, which is how a launch stages them into LDS.  Null / 0 for the built-in topologies.
    const uint32_t* g_out_off;  // P + 1
    const uint16_t* g_out_nbr;  // g_eout
    const uint32_t* g_in_off;   // P + 1
    const uint16_t* g_in_nbr;   // g_ein
    uint32_t g_eout, g_ein;
};

// The launch interface of one variant, defined in gp_ensemble_kernels.hpp and instantiated by
// gp_ensemble.hip (plain), gp_ensemble_faults.hip (failure) and gp_ensemble_trace.hip (both traced).
// Setup raises the kernel's dynamic-LDS limit for population P, once per handle; launch runs
// one workgroup per listed member.
template <bool FAULTS, bool TRACE>
hipError_t ens_setup_t(int topo, int alg, uint32_t P, uint32_t graph_lds);
template <bool FAULTS, bool TRACE>
hipError_t ens_launch_t(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st);
// (extern: the dispatchers below must not instantiate every variant in every unit)
extern template hipError_t ens_setup_t<false, false>(int, int, uint32_t, uint32_t);
extern template hipError_t ens_setup_t<true, false>(int, int, uint32_t, uint32_t);
extern template hipError_t ens_setup_t<false, true>(int, int, uint32_t, uint32_t);
extern template hipError_t ens_setup_t<true, true>(int, int, uint32_t, uint32_t);
extern template hipError_t ens_launch_t<false, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<true, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<false, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);
extern template hipError_t ens_launch_t<true, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);

// graph_lds: GRAPH only, the image of the handle's graph (ens_graph_lds_bytes); else 0.
inline hipError_t ens_setup(EnsVariant v, int topo, int alg, uint32_t P, uint32_t graph_lds) {
    if (v.trace)
        return v.faults ? ens_setup_t<true, true>(topo, alg, P, graph_lds) : ens_setup_t<false, true>(topo, alg, P, graph_lds);
    return v.faults ? ens_setup_t<true, false>(topo, alg, P, graph_lds) : ens_setup_t<false, false>(topo, alg, P, graph_lds);
}
inline hipError_t ens_launch(EnsVariant v, int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st) {
    if (v.trace)
        return v.faults ? ens_launch_t<true, true>(topo, alg, a, nblocks, st)
                        : ens_launch_t<false, true>(topo, alg, a, nblocks, st);
    return v.faults ? ens_launch_t<true, false>(topo, alg, a, nblocks, st)
                    : ens_launch_t<false, false>(topo, alg, a, nblocks, st);
}

}  // namespace gp
