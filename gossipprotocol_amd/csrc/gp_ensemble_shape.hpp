// gp_ensemble_shape.hpp -- the shape of an ensemble launch as a function of (topology, algorithm,
// population, variant): the LDS image of a member (and with it the population cap per pair and
// variant), the node slots a push-sum thread keeps and the workgroup size.  Host-clean: integer
// arithmetic over the public enums of gossip_hip.h, nothing of HIP, so a host compiler can include it
// (tests/helpers/ensemble_shape_check.cpp).  Included through gp_ensemble.hpp; DESIGN.md §9.
// A caller-supplied graph (SRS v1-G) has an image of its own, ens_graph_lds_bytes,
// with the entry counts in it; ens_lds_bytes and the caps below are the built-in topologies'.
#pragma once

#include <stdint.h>

#include "../../include/gossip_hip.h"

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
    if (alg == GP_GOSSIP) {
        b += ens_up8(4 * P) * 2;
        if (topo == GP_IMP3D) b += ens_up8(2 * P);
        if (topo != GP_FULL) b += ens_up8(4 * ((P + 31) / 32));
    } else {
        b += 8 * P * 2;
        if (topo == GP_FULL || topo == GP_IMP3D) b += ens_up8(4 * P) + ens_up8(2 * P);
        if (topo == GP_IMP3D) b += ens_up8(2 * P);
        if (topo != GP_FULL) b += ens_up8(P);
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
            for (int topo = GP_LINE; topo <= GP_IMP3D; ++topo)
                for (int alg = GP_GOSSIP; alg <= GP_PUSHSUM; ++alg)
                    if (ens_max_population(topo, alg, EnsVariant{faults != 0, trace != 0}) < 1001) return false;
    return true;
}
static_assert(ens_covers_report_range(), "report range");
static_assert((uint32_t)ENS_THREADS * ENS_NPT_MAX < ENS_NONE, "node ids must fit the 16-bit list links");

// ---- a caller-supplied graph (SRS v1-G) ----
// The fifth topology of the ensemble kernels; no other part of the library knows it.
constexpr int ENS_GRAPH = GP_GRAPH;
// Largest population of a graph: every node has a thread slot (ids then fit the 16-bit entries).
constexpr uint32_t ENS_GRAPH_POP_MAX = (uint32_t)ENS_THREADS * ENS_NPT_MAX;
// LDS image of one member on a graph of P nodes with e_out out-entries and e_in entries of the
// transposed, deduplicated in-CSR (gp_graph.hpp), arrays in this order, each padded to 8 bytes:
//   gossip   : c int32[P], inc int32[P], live bitmap u32[ceil(P/32)]
//   push-sum : hs f64[P], hw f64[P], tgt u16[P] (this round's target of a sender whose message
//              arrives, else ENS_NONE)
//   then the doomed bitmap and the trace block as above, then the adjacency, staged from HBM at
//   the start of every launch:
//   out_off u32[P + 1], out_nbr u16[e_out]; push-sum also in_off u32[P + 1], in_nbr u16[e_in]
// The offsets live in LDS, not in the node slots' registers: the 8-slot push-sum kernel is at its
// register ceiling already, and the offsets cost 8 of the 26 + 4 d bytes a node of average degree d takes.
// 64-bit: the entry counts are the caller's.
constexpr uint64_t ens_graph_lds_bytes(int alg, uint64_t P, uint64_t e_out, uint64_t e_in, EnsVariant v) {
    const uint64_t m8 = ~(uint64_t)7;
    uint64_t b = ENS_LDS_HDR;
    if (alg == GP_GOSSIP) {
        b += ((4 * P + 7) & m8) * 2 + ((4 * ((P + 31) / 32) + 7) & m8);
    } else {
        b += 8 * P * 2 + ((2 * P + 7) & m8);
    }
    if (v.faults) b += (4 * ((P + 31) / 32) + 7) & m8;
    if (v.trace) b += ENS_LDS_TRACE;
    b += ((4 * (P + 1) + 7) & m8) + ((2 * e_out + 7) & m8);
    if (alg != GP_GOSSIP) b += ((4 * (P + 1) + 7) & m8) + ((2 * e_in + 7) & m8);
    return b;
}
// A symmetric graph of 1000 nodes and average degree 16 fits in every variant of both algorithms.
constexpr bool ens_graph_covers_degree_16() {
    for (int faults = 0; faults < 2; ++faults)
        for (int trace = 0; trace < 2; ++trace)
            for (int alg = GP_GOSSIP; alg <= GP_PUSHSUM; ++alg)
                if (ens_graph_lds_bytes(alg, 1000, 16000, 16000, EnsVariant{faults != 0, trace != 0}) > ENS_LDS_MAX)
                    return false;
    return true;
}
static_assert(ens_graph_covers_degree_16(), "graph range");

// Largest num_nodes: line / full P = n + 1; 3D / Imp3D the largest whole cube.
constexpr int64_t ens_max_nodes(int topo, int alg, EnsVariant v) {
    const uint32_t P = ens_max_population(topo, alg, v);
    if (topo == GP_LINE || topo == GP_FULL) return (int64_t)P - 1;
    uint32_t g = 1;
    while ((g + 1) * (g + 1) * (g + 1) <= P) ++g;
    return (int64_t)g * g * g;
}

// Push-sum: the node slots per thread, the smallest power of two that gives every node a slot in a
// workgroup of at most ENS_THREADS (1, 2, 4 or 8 up to the cap: the instantiations of k_ens_pushsum).
constexpr int ens_npt(uint32_t P) {
    int npt = 1;
    while ((uint32_t)npt * ENS_THREADS < P) npt *= 2;
    return npt;
}

// The workgroup: whole waves, enough for one node a thread per slot (push-sum: thread t keeps nodes
// t + q * threads, q < npt, so the last slot may be partly filled) or per pass of the strided loops
// (gossip), at most ENS_THREADS.
constexpr uint32_t ens_threads(int alg, uint32_t P) {
    const uint32_t per = alg == GP_PUSHSUM ? (P + ens_npt(P) - 1) / ens_npt(P) : P;
    const uint32_t t = (per + 63u) & ~63u;
    return t > (uint32_t)ENS_THREADS ? (uint32_t)ENS_THREADS : t;
}

}  // namespace gp
