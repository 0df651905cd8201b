// gp_ensemble_kernels.hpp -- ensemble kernels: workgroup b simulates one whole network
// (member idx[b], seed rec[m].seed) with its node state in LDS and registers, a
// workgroup barrier between the phases of a round, no launch per round and no HBM
// traffic in the round loop.  Workgroups never talk to each other; a grid larger
// than what is resident simply queues.  DESIGN.md §9; layout and launch shape: gp_ensemble_shape.hpp.
//
// Included by exactly three translation units, each of which explicitly instantiates
// ens_setup_t / ens_launch_t (declared in gp_ensemble.hpp, defined at the end of this
// file) and with them the kernels of its variants: gp_ensemble.hip <false, false> (the
// plain kernels), gp_ensemble_faults.hip <true, false> (crashed nodes and lost messages,
// SRS v1-F) and gp_ensemble_trace.hip <false, true> and <true, true> (a
// row per stride rounds, SRS v1-T).  The kernels themselves stay in the
// anonymous namespace.  Every variant takes the same EnsArgs; every line a fault adds
// sits under `if (FAULTS)`, every line tracing adds under `if constexpr (TRACE)`,
// compile-time branches, so a kernel never reads the part of the arguments it has no use for.
//
// The rounds are SRS v1 exactly as the per-round kernels
// and the oracle run them: same Philox draws (gp_device.hpp), push-sum folded own
// half first, then lattice messages in the receiver's slot order, then random-edge
// / full messages by ascending sender id.  Built with -ffp-contract=off.
//
// TOPO == GRAPH (SRS v1-G) is a fifth topology of these kernels alone:
// the neighbour lists come from the caller's CSR, staged from HBM into LDS at the start of every
// launch.  Gossip pushes as before; push-sum pulls: a sender publishes its target, a receiver walks
// its in-list (transposed, ascending, deduplicated: gp_graph.hpp) and folds the senders that target
// it, which is the canonical order.  Every line it adds sits under `if constexpr (TOPO == GRAPH)`.
//
// Reference mapping (Program.fs = the reference's Project2/Program.fs): the actor
// loops Program.fs:84-131, the injector Program.fs:141-163 and the scheduler
// Program.fs:41-61 of one run; the setup Program.fs:169-176,193,221,258-263.
#pragma once

#include "gp_ensemble.hpp"

namespace gp {
namespace {

// Sum / maximum over the 64 lanes of a wave; every lane gets the result.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

struct Member {
    uint32_t k0, k1;  // Philox key, wave-uniform
    uint32_t seed_node;
    uint32_t alerts;
    uint32_t live;
    int64_t rounds;
    int64_t left;  // rounds this launch may still run
};

// Reads member m's record (or sets it up from the seed); every thread gets the same values.
__device__ __forceinline__ Member member_begin(const EnsArgs& a, uint32_t m) {
    const gp_member* rec = a.rec + m;
    Member M;
    const uint64_t seed = rec->seed;
    M.k0 = __builtin_amdgcn_readfirstlane((uint32_t)seed);
    M.k1 = __builtin_amdgcn_readfirstlane((uint32_t)(seed >> 32));
    if (a.init) {
        // seed choice = Random().Next(0, nodes) (Program.fs:193,221,263)
        M.seed_node = uniform(M.k0, M.k1, S_START, 0, 0, a.G.T);
        M.alerts = 0;
        M.live = a.G.T;
        M.rounds = 0;
    } else {
        M.seed_node = (uint32_t)rec->seed_node;
        M.alerts = (uint32_t)rec->converged;
        M.live = (uint32_t)rec->reserved;
        M.rounds = rec->rounds;
    }
    const int64_t cap = a.max_rounds - M.rounds;
    M.left = a.nrounds < cap ? a.nrounds : cap;
    return M;
}

// thr: the alerts that end the run (T; T_f under the failure model).
__device__ __forceinline__ void member_end(const EnsArgs& a, uint32_t m, const Member& M, uint32_t thr) {
    if (threadIdx.x != 0) return;
    gp_member* rec = a.rec + m;
    rec->rounds = M.rounds;
    rec->converged = M.alerts;
    rec->seed_node = M.seed_node;
    rec->status = M.alerts >= thr ? GP_STATUS_CONVERGED
                  : M.rounds >= a.max_rounds ? GP_STATUS_MAX_ROUNDS : GP_STATUS_RUNNING;
    rec->reserved = (int32_t)M.live;
}

// Present-direction mask of node j (Imp3D: its lattice part).
template <int TOPO>
__device__ __forceinline__ uint32_t ens_mask(uint32_t j, const Geom& G) {
    return present_mask<(TOPO == LINE ? LINE : GRID3D)>(j, G);
}

// ------------------------------------------------------------------ failure model
// hdr[2] = |D| and hdr[3] = this launch's lost messages must be zero before the redraw.
__device__ __forceinline__ void faults_clear(uint32_t* hdr) {
    if (threadIdx.x == 0) {
        hdr[2] = 0;
        hdr[3] = 0;
    }
    __syncthreads();
}

// One node of the redraw of D (one Philox draw per node per launch, nothing of D in
// HBM).  Call with i = tid + k * nthr in ascending k: a wave then holds the 64
// consecutive ids from a multiple of 64 on, i.e. two whole bitmap words, which its
// first lane stores -- no atomics, and every word of the bitmap gets written.  Lanes
// past P have left the caller's loop and read as 0 in the ballot.  Returns i in D.
// This needs a workgroup of whole waves (nthr a multiple of 64, so that the first
// lane's i is one too); ens_launch_t refuses any other launch of the failure kernels.
__device__ __forceinline__ bool faults_draw(const EnsFaults& f, const Geom& G, const Member& M, uint32_t i,
                                            uint32_t* dm, uint32_t* hdr) {
    const bool in = ens_doomed(M.k0, M.k1, i, M.seed_node, f.q_node);
    const uint64_t b = __ballot(in);
    if ((threadIdx.x & 63u) == 0) {
        const uint32_t wd = i >> 5, nw = (G.P + 31u) >> 5;
        dm[wd] = (uint32_t)b;
        if (wd + 1 < nw) dm[wd + 1] = (uint32_t)(b >> 32);
        if (b) atomicAdd(&hdr[2], (uint32_t)__popcll(b));
    }
    return in;
}

__device__ __forceinline__ bool faults_bit(const uint32_t* dm, uint32_t i) { return (dm[i >> 5] >> (i & 31u)) & 1u; }

// T_f = max(1, T - |D|) (after the barrier that follows the redraw).
__device__ __forceinline__ uint32_t faults_threshold(const Geom& G, const uint32_t* hdr) {
    const int32_t t = (int32_t)G.T - (int32_t)hdr[2];
    return t < 1 ? 1u : (uint32_t)t;
}

// Does sender i's message of round r disappear on the way (stream S_FAULT_DROP)?
__device__ __forceinline__ bool faults_dropped(const EnsFaults& f, const Member& M, uint32_t i, uint32_t r) {
    uint32_t x, y;
    philox2(i, r, S_FAULT_DROP, M.k0, M.k1, x, y);
    return (uint64_t)x < f.q_drop;
}

// End of a launch: the threads' lost counts, one wave reduction and one LDS add per
// wave, then a single store to the member's record.
__device__ __forceinline__ void faults_end(const EnsFaults& f, uint32_t m, bool init, uint32_t lost,
                                           uint32_t* hdr) {
    lost = wave_sum(lost);
    if ((threadIdx.x & 63u) == 0 && lost) atomicAdd(&hdr[3], lost);
    __syncthreads();
    if (threadIdx.x == 0) {
        EnsFaultRec* fr = f.frec + m;
        fr->lost = (init ? 0 : fr->lost) + (int64_t)hdr[3];
        fr->doomed = (int64_t)hdr[2];
    }
}

// ------------------------------------------------------------------ trace (SRS v1-T)
// Which round records the next row: workgroup-uniform scalars, no division in the round loop.
struct TraceClock {
    int64_t next_round;  // the next multiple of stride above the member's rounds
    int64_t row;         // its row index, next_round / stride - 1
};
__device__ __forceinline__ TraceClock trace_begin(const EnsTrace& t, const Member& M) {
    const int64_t k = M.rounds / t.stride;
    return TraceClock{(k + 1) * t.stride, k};
}
// Does the round that starts with M.rounds completed record a row?
__device__ __forceinline__ bool trace_records(const EnsTrace& t, const TraceClock& K, const Member& M) {
    return M.rounds + 1 == K.next_round && K.row < t.capacity;
}
// Thread 0, before the barrier that ends the set-up: sent continues from the member's record.
__device__ __forceinline__ void trace_clear(const EnsTrace& t, uint32_t m, bool init, double mu, EnsTraceLds* tr) {
    tr->sent = init ? 0ull : (unsigned long long)t.trec[m].sent;
    tr->err = 0;
    tr->reached = 0;
    tr->mu = mu;
}
// The threads' counts into an LDS word: one wave reduction, one LDS atomic per wave.
__device__ __forceinline__ void trace_add32(uint32_t* word, uint32_t v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(word, v);
}
__device__ __forceinline__ void trace_add64(unsigned long long* word, uint32_t v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(word, (unsigned long long)v);
}
__device__ __forceinline__ void trace_max64(unsigned long long* word, unsigned long long v) {
    v = wave_max(v);
    if ((threadIdx.x & 63u) == 0 && v) atomicMax(word, v);
}
// |e| of one push-sum node as its bit pattern, e = fl(fl(s / w) - mu): no floating-point
// comparison decides anything (a weight that underflowed to 0 gives inf or NaN).
__device__ __forceinline__ unsigned long long trace_err_bits(double s, double w, double mu) {
    const double e = s / w - mu;
    return (unsigned long long)__double_as_longlong(e) & 0x7FFFFFFFFFFFFFFFull;
}
// One lane, after the round's closing barrier: the row of the round just completed.
__device__ __forceinline__ void trace_row(const EnsTrace& t, uint32_t m, const TraceClock& K, const Member& M,
                                          const EnsTraceLds* tr) {
    gp_trace_row* row = t.rows + ((size_t)m * (size_t)t.capacity + (size_t)K.row);
    unsigned long long e = tr->err;
    if (e > 0x7FF0000000000000ull) e = 0x7FF8000000000000ull;  // any NaN: the canonical quiet one
    row->round = M.rounds;
    row->reached = tr->reached;
    row->alerts = M.alerts;
    row->sent = tr->sent;
    row->err_max = __longlong_as_double((long long)e);
}
// End of a launch: what the threads still hold goes into the total, which the record keeps.
// (If the last round recorded a row, every thread flushed there and adds nothing here, so
// thread 0's read of the total for that row is not disturbed.)
__device__ __forceinline__ void trace_end(const EnsTrace& t, uint32_t m, uint32_t nsent, EnsTraceLds* tr) {
    trace_add64(&tr->sent, nsent);
    __syncthreads();
    if (threadIdx.x == 0) t.trec[m].sent = tr->sent;
}

// ------------------------------------------------------------------ graph (SRS v1-G)
// Stages `bytes` (a multiple of 8: the device arrays and their LDS copies are padded alike) from
// HBM into LDS, 8 bytes a thread and pass; the caller's next barrier publishes them.
__device__ __forceinline__ void graph_stage(void* dst, const void* src, uint32_t bytes) {
    uint2* d = reinterpret_cast<uint2*>(dst);
    const uint2* s = reinterpret_cast<const uint2*>(src);
    for (uint32_t q = threadIdx.x; q < bytes / 8u; q += blockDim.x) d[q] = s[q];
}

// ------------------------------------------------------------------ gossip
// Per round (SRS v1 B.3): phase 1 every sending node draws a neighbour and bumps
// inc[target] iff the target is unconverged in c, which nobody writes in this phase
// (the round-start snapshot); wave 0 also runs the injector.  Phase 2 applies inc.
// FAULTS (B.5): a down node neither sends nor receives (the injector drops it from
// its list like a converged one), so its c stays frozen; a sender's message may be
// dropped; alerts of doomed nodes are not counted.
// TRACE (SRS v1-T): reached = nodes with c >= 1 or the seed node, bumped in phase 2; sent
// counted per thread in phase 1 and flushed before the closing barrier of a recording round.
template <int TOPO, bool FAULTS, bool TRACE>
__global__ __launch_bounds__(ENS_THREADS) void k_ens_gossip(const EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t P = a.G.P, tid = threadIdx.x, nthr = blockDim.x;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(lds);
    unsigned char* at = lds + ENS_LDS_HDR;
    int32_t* c = reinterpret_cast<int32_t*>(at);
    at += ens_up8(4 * P);
    int32_t* inc = reinterpret_cast<int32_t*>(at);
    at += ens_up8(4 * P);
    uint16_t* rnd = reinterpret_cast<uint16_t*>(at);
    if (TOPO == IMP3D) at += ens_up8(2 * P);
    uint32_t* bits = reinterpret_cast<uint32_t*>(at);
    if (TOPO != FULL) at += ens_up8(4 * ((P + 31) / 32));
    uint32_t* dm = reinterpret_cast<uint32_t*>(at);  // FAULTS: doomed bitmap
    if (FAULTS) at += ens_up8(4 * ((P + 31) / 32));
    EnsTraceLds* tr = reinterpret_cast<EnsTraceLds*>(at);  // TRACE: trace block
    uint32_t* goff = nullptr;  // GRAPH: out-CSR offsets, P + 1
    uint16_t* gnbr = nullptr;  // GRAPH: out-neighbours in the caller's order
    if constexpr (TOPO == GRAPH) {
        if (TRACE) at += ENS_LDS_TRACE;
        goff = reinterpret_cast<uint32_t*>(at);
        gnbr = reinterpret_cast<uint16_t*>(at + ens_up8(4 * (P + 1)));
        // the adjacency, redone at every launch like rnd; published by the set-up's barrier
        graph_stage(goff, a.g_out_off, ens_up8(4 * (P + 1)));
        graph_stage(gnbr, a.g_out_nbr, ens_up8(2 * a.g_eout));
    }

    const uint32_t m = a.idx[blockIdx.x];
    Member M = member_begin(a, m);
    int32_t* gc = a.c + (size_t)m * P;
    uint32_t* gbits = TOPO == FULL ? nullptr : a.bits + (size_t)m * a.nwords;
    uint32_t thr = a.G.T, lost = 0;
    if constexpr (FAULTS) faults_clear(hdr);
    uint32_t nsent = 0, nreached = 0;  // TRACE: this thread's messages not yet in tr->sent; its nodes that know the rumour

    for (uint32_t i = tid; i < P; i += nthr) {
        c[i] = a.init ? 0 : gc[i];  // rumours = 0 (Program.fs:68)
        inc[i] = 0;
        if constexpr (TRACE) nreached += (i == M.seed_node || c[i] >= 1) ? 1u : 0u;
        // Imp3D random neighbour: Random().Next(0, nodes-1) -> [0, P-2] (Program.fs:259)
        if (TOPO == IMP3D) rnd[i] = (uint16_t)uniform(M.k0, M.k1, S_TOPO, i, 0, P - 1);
        if constexpr (FAULTS) faults_draw(a.f, a.G, M, i, dm, hdr);
    }
    if (TOPO != FULL)
        for (uint32_t q = tid; q < a.nwords; q += nthr) {
            // injector list = ids 0..nodes-1 (Program.fs:147-148)
            const uint32_t rest = a.G.T - q * 32;
            bits[q] = a.init ? (rest >= 32 ? 0xFFFFFFFFu : (1u << rest) - 1u) : gbits[q];
        }
    if (tid == 0) hdr[0] = M.alerts;
    if constexpr (TRACE)
        if (tid == 0) trace_clear(a.t, m, a.init, a.mu, tr);
    __syncthreads();
    if constexpr (FAULTS) thr = faults_threshold(a.G, hdr);
    TraceClock K{};
    if constexpr (TRACE) {
        // the recount of the loaded state; phase 2 adds to it only after a later barrier
        trace_add32(&tr->reached, nreached);
        K = trace_begin(a.t, M);
    }

    for (int64_t it = 0; it < M.left && M.alerts < thr; ++it) {
        const uint32_t r = (uint32_t)M.rounds;
        bool down_now = false;  // are the doomed nodes down in this round?  (workgroup-uniform)
        if constexpr (FAULTS) down_now = M.rounds >= a.f.fail_round;
        bool rec_now = false;  // does this round record a row?  (workgroup-uniform)
        if constexpr (TRACE) rec_now = trace_records(a.t, K, M);
        for (uint32_t i = tid; i < P; i += nthr) {
            const int32_t ci = c[i];
            if (!((i == M.seed_node || ci >= 1) && ci <= 10)) continue;  // Program.fs:85
            if constexpr (FAULTS)
                if (down_now && faults_bit(dm, i)) continue;  // (c <= 10 alone would let it send)
            if constexpr (TRACE) nsent += 1;  // it draws a target: sent, whatever becomes of the message
            uint32_t t;
            if constexpr (TOPO == GRAPH) {
                const uint32_t o = goff[i];  // nb(i)[U_GOSSIP(deg i)]
                t = gnbr[o + uniform(M.k0, M.k1, S_GOSSIP, i, r, goff[i + 1] - o)];
            } else if (TOPO == FULL) {
                t = full_target(i, uniform(M.k0, M.k1, S_GOSSIP, i, r, P - 1));
            } else {
                const uint32_t mask = ens_mask<TOPO>(i, a.G);
                const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                const uint32_t d = slot_to_dir(mask, uniform(M.k0, M.k1, S_GOSSIP, i, r, deg));
                t = (TOPO == IMP3D && d == DIR_RANDOM) ? (uint32_t)rnd[i] : nbr<(TOPO == LINE ? LINE : GRID3D)>(i, d, a.G);
            }
            if constexpr (FAULTS) {
                // dropped, else addressed to a down node: lost; a converged target only suppresses
                if ((a.f.q_drop != 0 && faults_dropped(a.f, M, i, r)) || (down_now && faults_bit(dm, t))) {
                    lost += 1;
                    continue;
                }
            }
            if (c[t] < (int32_t)GOSSIP_DONE) atomicAdd(&inc[t], 1);
        }
        if (TOPO != FULL && tid < 64) {
            // Injector (Program.fs:150-159): the k-th smallest live id, k = U_INJECT(live);
            // deliver if unconverged, else remove.  Rank-select over the bitmap by wave 0:
            // each lane counts a run of words, a wave scan finds the lane holding rank k.
            if (M.live > 0) {
                const uint32_t k = uniform(M.k0, M.k1, S_INJECT, 0, r, M.live);
                const uint32_t W = (a.nwords + 63) / 64, base = tid * W;
                uint32_t cnt = 0;
                for (uint32_t q = 0; q < W; ++q)
                    if (base + q < a.nwords) cnt += (uint32_t)__popc(bits[base + q]);
                uint32_t incl = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t v = __shfl_up(incl, off, 64);
                    if ((int)tid >= off) incl += v;
                }
                uint32_t rem = k - (incl - cnt);  // rank inside this lane's run, if it holds k
                int removed = 0;
                if (k >= incl - cnt && k < incl) {
                    for (uint32_t q = 0; q < W; ++q) {
                        uint32_t wd = bits[base + q];
                        const uint32_t pc = (uint32_t)__popc(wd);
                        if (rem >= pc) {
                            rem -= pc;
                            continue;
                        }
                        for (; rem; --rem) wd &= wd - 1;  // (rem < 32)
                        const uint32_t b = (uint32_t)__ffs(wd) - 1u;
                        const uint32_t t = (base + q) * 32 + b;
                        bool gone = c[t] >= (int32_t)GOSSIP_DONE;
                        if constexpr (FAULTS) gone = gone || (down_now && faults_bit(dm, t));  // never dropped
                        if (gone) {
                            bits[base + q] &= ~(1u << b);
                            removed = 1;
                        } else {
                            atomicAdd(&inc[t], 1);
                        }
                        break;
                    }
                }
                if (__any(removed)) M.live -= 1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < P; j += nthr) {
            const int32_t d = inc[j];
            if (!d) continue;
            const int32_t c0 = c[j], c1 = c0 + d;
            if (c0 <= 10 && c1 > 10) {  // Program.fs:91-98
                bool counted = true;
                if constexpr (FAULTS) counted = !faults_bit(dm, j);
                if (counted) atomicAdd(&hdr[0], 1u);
            }
            if constexpr (TRACE)
                if (c0 == 0 && j != M.seed_node) atomicAdd(&tr->reached, 1u);  // (d > 0: it knows the rumour now)
            c[j] = c1;
            inc[j] = 0;
        }
        if constexpr (TRACE) {
            // in this phase, not phase 1: thread 0 may still be reading the last row's total there
            if (rec_now) {
                trace_add64(&tr->sent, nsent);
                nsent = 0;
            }
        }
        __syncthreads();
        M.alerts = hdr[0];
        M.rounds += 1;
        if constexpr (TRACE) {
            if (rec_now && tid == 0) trace_row(a.t, m, K, M, tr);
            if (M.rounds == K.next_round) {
                K.next_round += a.t.stride;
                K.row += 1;
            }
        }
    }

    for (uint32_t i = tid; i < P; i += nthr) gc[i] = c[i];
    if (TOPO != FULL)
        for (uint32_t q = tid; q < a.nwords; q += nthr) gbits[q] = bits[q];
    if constexpr (TRACE) trace_end(a.t, m, nsent, tr);
    if constexpr (FAULTS) faults_end(a.f, m, a.init, lost, hdr);
    member_end(a, m, M, thr);  // (thread 0 is in wave 0, which counted the injector's removals)
}

// ------------------------------------------------------------------ push-sum
// Thread t keeps nodes t, t + nthr, ... (NPT slots) in registers.  Per round (SRS
// v1 B.4): phase A every active node draws its direction, publishes it and its
// halves (s/2, w/2 -- the half it keeps and the half it sends are the same
// number) in LDS, and hooks itself into the target's list if the edge is a random
// one; phase B every node folds own half, then lattice senders in its own slot
// order (neighbour n sends to j iff dir[n] is the opposite of j's slot), then the
// list by ascending sender id, and runs the ratio test (Program.fs:114-123).
// FAULTS (B.5): a down node is skipped in both phases (its registers stay as they
// are); a sender whose message is dropped or addressed to a down node halves itself
// but publishes DIR_NONE and hooks into no list, so no receiver ever sees it.
// GRAPH (B.7): phase A publishes tgt[i] (ENS_NONE: no message arrives from i) beside the halves;
// phase B folds own half, then hs[n], hw[n] of every n in j's in-list with tgt[n] == j, ascending.
// TRACE (SRS v1-T): reached = nodes with the active bit, bumped in phase B; sent counted
// per thread in phase A; in a recording round thread 0 zeroes the err word in phase A and
// every wave folds its nodes' |e| and its sent count in after phase B, before the closing barrier.
template <int TOPO, int NPT, bool FAULTS, bool TRACE>
__global__ __launch_bounds__(ENS_THREADS) void k_ens_pushsum(const EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool LISTS = TOPO == FULL || TOPO == IMP3D;
    constexpr int LT = TOPO == LINE ? LINE : GRID3D;
    constexpr bool LATTICE = TOPO != FULL && TOPO != GRAPH;  // implicit lattice slots: mask in fl, dir[] in LDS
    constexpr uint32_t F_DOOMED = 1u << 14;  // FAULTS: fl bit, node in D
    const uint32_t P = a.G.P, tid = threadIdx.x, nthr = blockDim.x;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(lds);
    unsigned char* at = lds + ENS_LDS_HDR;
    double* hs = reinterpret_cast<double*>(at);
    at += 8 * P;
    double* hw = reinterpret_cast<double*>(at);
    at += 8 * P;
    uint32_t* head = reinterpret_cast<uint32_t*>(at);
    if (LISTS) at += ens_up8(4 * P);
    uint16_t* next = reinterpret_cast<uint16_t*>(at);
    if (LISTS) at += ens_up8(2 * P);
    uint16_t* rnd = reinterpret_cast<uint16_t*>(at);
    if (TOPO == IMP3D) at += ens_up8(2 * P);
    uint8_t* dir = at;
    if (LATTICE) at += ens_up8(P);
    uint16_t* tgt = reinterpret_cast<uint16_t*>(at);  // GRAPH: this round's target of a sender whose message arrives
    if (TOPO == GRAPH) at += ens_up8(2 * P);
    uint32_t* dm = reinterpret_cast<uint32_t*>(at);  // FAULTS: doomed bitmap
    if (FAULTS) at += ens_up8(4 * ((P + 31) / 32));
    EnsTraceLds* tr = reinterpret_cast<EnsTraceLds*>(at);  // TRACE: trace block
    // GRAPH: out-CSR (offsets P + 1, neighbours), then the transposed, deduplicated in-CSR
    uint32_t *goff = nullptr, *gioff = nullptr;
    uint16_t *gnbr = nullptr, *ginbr = nullptr;
    if constexpr (TOPO == GRAPH) {
        if (TRACE) at += ENS_LDS_TRACE;
        const uint32_t offb = ens_up8(4 * (P + 1)), outb = ens_up8(2 * a.g_eout);
        goff = reinterpret_cast<uint32_t*>(at);
        gnbr = reinterpret_cast<uint16_t*>(at + offb);
        gioff = reinterpret_cast<uint32_t*>(at + offb + outb);
        ginbr = reinterpret_cast<uint16_t*>(at + 2 * offb + outb);
        // the adjacency, redone at every launch like rnd; published by the set-up's barrier
        graph_stage(goff, a.g_out_off, ens_up8(4 * (P + 1)));
        graph_stage(gnbr, a.g_out_nbr, ens_up8(2 * a.g_eout));
        graph_stage(gioff, a.g_in_off, ens_up8(4 * (P + 1)));
        graph_stage(ginbr, a.g_in_nbr, ens_up8(2 * a.g_ein));
    }

    const uint32_t m = a.idx[blockIdx.x];
    Member M = member_begin(a, m);
    double* gs = a.s + (size_t)m * P;
    double* gw = a.w + (size_t)m * P;
    uint8_t* gf = a.fl + (size_t)m * P;
    uint32_t thr = a.G.T, lost = 0;
    if constexpr (FAULTS) faults_clear(hdr);
    uint32_t nsent = 0, nreached = 0;  // TRACE: this thread's messages not yet in tr->sent; its active nodes

    // fl: bit0 active, bit1 converged, bits2-3 count (the gp_read_state byte), bits 8-13 lattice mask
    double s[NPT], w[NPT];
    uint32_t fl[NPT];
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const uint32_t i = tid + q * nthr;
        s[q] = 0.0;
        w[q] = 1.0;
        fl[q] = 0;
        if (i >= P) continue;
        if (a.init) {
            // sum = id, weight = 1, count = 1; only the seed is active (Program.fs:67,71,78,174)
            s[q] = (double)i;
            fl[q] = (1u << 2) | (i == M.seed_node ? 1u : 0u);
        } else {
            s[q] = gs[i];
            w[q] = gw[i];
            fl[q] = gf[i];
        }
        if constexpr (TRACE) nreached += fl[q] & 1u;
        if (LATTICE) fl[q] |= ens_mask<TOPO>(i, a.G) << 8;
        if (LISTS) head[i] = ENS_NONE;
        if (TOPO == IMP3D) rnd[i] = (uint16_t)uniform(M.k0, M.k1, S_TOPO, i, 0, P - 1);
        if constexpr (FAULTS)
            if (faults_draw(a.f, a.G, M, i, dm, hdr)) fl[q] |= F_DOOMED;
    }
    if (a.init && a.x0) {  // SRS v1-V: sum = x_i, weight = omega_i where the caller gave them (set-up launch only)
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t i = tid + q * nthr;
            if (i >= P) continue;
            s[q] = a.x0[i];
            if (a.w0) w[q] = a.w0[i];
        }
    }
    if (tid == 0) hdr[0] = M.alerts;
    if constexpr (TRACE)
        if (tid == 0) trace_clear(a.t, m, a.init, a.mu, tr);
    __syncthreads();
    if constexpr (FAULTS) thr = faults_threshold(a.G, hdr);
    TraceClock K{};
    if constexpr (TRACE) {
        // the recount of the loaded state; phase B adds to it only after a later barrier
        trace_add32(&tr->reached, nreached);
        K = trace_begin(a.t, M);
    }

    for (int64_t it = 0; it < M.left && M.alerts < thr; ++it) {
        const uint32_t r = (uint32_t)M.rounds;
        bool down_now = false;  // are the doomed nodes down in this round?  (workgroup-uniform)
        if constexpr (FAULTS) down_now = M.rounds >= a.f.fail_round;
        bool rec_now = false;  // does this round record a row?  (workgroup-uniform)
        if constexpr (TRACE) {
            rec_now = trace_records(a.t, K, M);
            if (rec_now && tid == 0) tr->err = 0;  // (the last row's read of it was this thread's own)
        }
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t i = tid + q * nthr;
            if (i >= P) continue;
            uint32_t d = DIR_NONE;
            bool sends = fl[q] & 1u;
            if constexpr (FAULTS) sends = sends && !(down_now && (fl[q] & F_DOOMED));
            if constexpr (TOPO == GRAPH) tgt[i] = (uint16_t)ENS_NONE;  // no sender, or its message is lost
            if (sends) {
                if constexpr (TRACE) nsent += 1;  // sent, whatever becomes of the message
                uint32_t t = 0;
                if constexpr (TOPO == GRAPH) {
                    d = DIR_RANDOM;  // (here: the message has a target; DIR_NONE below: it is lost)
                    const uint32_t o = goff[i];  // nb(i)[U_PUSHSUM(deg i)]
                    t = gnbr[o + uniform(M.k0, M.k1, S_PUSHSUM, i, r, goff[i + 1] - o)];
                } else if (TOPO == FULL) {
                    d = DIR_RANDOM;
                    t = full_target(i, uniform(M.k0, M.k1, S_PUSHSUM, i, r, P - 1));
                } else {
                    const uint32_t mask = (fl[q] >> 8) & 63u;
                    const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                    d = slot_to_dir(mask, uniform(M.k0, M.k1, S_PUSHSUM, i, r, deg));
                    if (TOPO == IMP3D) t = rnd[i];
                }
                bool gone = false;
                if constexpr (FAULTS) {
                    if (a.f.q_drop != 0) gone = faults_dropped(a.f, M, i, r);
                    if (down_now && !gone) {
                        if (LATTICE && d != DIR_RANDOM) t = nbr<LT>(i, d, a.G);
                        gone = faults_bit(dm, t);
                    }
                }
                if (gone) {
                    lost += 1;
                    d = DIR_NONE;  // the sent half leaves the network
                } else {
                    hs[i] = s[q] * 0.5;
                    hw[i] = w[q] * 0.5;
                    if (LISTS && d == DIR_RANDOM) next[i] = (uint16_t)atomicExch(&head[t], i);
                    if constexpr (TOPO == GRAPH) tgt[i] = (uint16_t)t;
                }
            }
            if (LATTICE) dir[i] = (uint8_t)d;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t j = tid + q * nthr;
            if (j >= P) continue;
            if constexpr (FAULTS) {
                if (down_now && (fl[q] & F_DOOMED)) {  // ignores its mail; s, w, count, active bit frozen
                    if (LISTS) head[j] = ENS_NONE;
                    continue;
                }
            }
            const double s0 = s[q], w0 = w[q];
            double as = (fl[q] & 1u) ? s0 * 0.5 : s0;
            double aw = (fl[q] & 1u) ? w0 * 0.5 : w0;
            bool recv = false;
            if constexpr (TOPO == GRAPH) {
                // pull: the in-list holds the nodes that list j, ascending and each once, so the walk is
                // the canonical fold order (B.7: every message by ascending sender id) and needs no search
                const uint32_t e1 = gioff[j + 1];
                for (uint32_t e = gioff[j]; e < e1; ++e) {
                    const uint32_t n = ginbr[e];
                    if (tgt[n] != j) continue;
                    as = as + hs[n];
                    aw = aw + hw[n];
                    recv = true;
                }
            }
            if (LATTICE) {
                const uint32_t mask = (fl[q] >> 8) & 63u;
#pragma unroll
                for (uint32_t d = 0; d < (TOPO == LINE ? 2u : 6u); ++d) {
                    if (!(mask & (1u << d))) continue;
                    const uint32_t n = nbr<LT>(j, d, a.G);
                    if (dir[n] != (d ^ 1u)) continue;
                    as = as + hs[n];
                    aw = aw + hw[n];
                    recv = true;
                }
            }
            if (LISTS) {
                const uint32_t h = head[j];
                if (h != ENS_NONE) {
                    head[j] = ENS_NONE;
                    // the list holds this round's senders in arrival order: take them by
                    // ascending id (a list is one or two long; at most P)
                    int last = -1;
                    for (uint32_t taken = 0; taken < P; ++taken) {
                        uint32_t best = ENS_NONE, p = h;
                        for (uint32_t hop = 0; hop < P && p != ENS_NONE; ++hop) {
                            if ((int)p > last && p < best) best = p;
                            p = next[p];
                        }
                        if (best == ENS_NONE) break;
                        as = as + hs[best];
                        aw = aw + hw[best];
                        last = (int)best;
                    }
                    recv = true;
                }
            }
            if (recv) {
                if (!(fl[q] & 2u)) {
                    uint32_t cnt = (fl[q] >> 2) & 3u;
                    cnt = ratio_moved(s0, w0, as, aw) ? 0u : cnt + 1u;
                    if (cnt == 3u) {
                        fl[q] |= 2u;
                        if (!FAULTS || !(fl[q] & F_DOOMED)) atomicAdd(&hdr[0], 1u);  // a doomed node's alert is not counted
                    }
                    fl[q] = (fl[q] & ~12u) | (cnt << 2);
                }
                if constexpr (TRACE)
                    if (!(fl[q] & 1u)) atomicAdd(&tr->reached, 1u);  // active for the first time
                fl[q] |= 1u;
            }
            s[q] = as;
            w[q] = aw;
        }
        if constexpr (TRACE) {
            if (rec_now) {
                // all P nodes, down ones included (their s, w are frozen); the division is paid here only
                unsigned long long e = 0;
                const double mu = tr->mu;  // the handle's mean
#pragma unroll
                for (int q = 0; q < NPT; ++q) {
                    if (tid + q * nthr >= P) continue;
                    const unsigned long long eq = trace_err_bits(s[q], w[q], mu);
                    e = eq > e ? eq : e;
                }
                trace_max64(&tr->err, e);
                // in this phase, not phase A: thread 0 may still be reading the last row's total there
                trace_add64(&tr->sent, nsent);
                nsent = 0;
            }
        }
        __syncthreads();
        M.alerts = hdr[0];
        M.rounds += 1;
        if constexpr (TRACE) {
            if (rec_now && tid == 0) trace_row(a.t, m, K, M, tr);
            if (M.rounds == K.next_round) {
                K.next_round += a.t.stride;
                K.row += 1;
            }
        }
    }

#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const uint32_t i = tid + q * nthr;
        if (i >= P) continue;
        gs[i] = s[q];
        gw[i] = w[q];
        gf[i] = (uint8_t)(fl[q] & 15u);
    }
    if constexpr (TRACE) trace_end(a.t, m, nsent, tr);
    if constexpr (FAULTS) faults_end(a.f, m, a.init, lost, hdr);
    member_end(a, m, M, thr);
}

template <int TOPO, bool FAULTS, bool TRACE>
const void* ps_kernel(int npt) {
    switch (npt) {
        case 1: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 1, FAULTS, TRACE>);
        case 2: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 2, FAULTS, TRACE>);
        case 4: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 4, FAULTS, TRACE>);
        case 8: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 8, FAULTS, TRACE>);
        default: return nullptr;
    }
}
static_assert(ENS_NPT_MAX == 8, "ps_kernel lists the slot counts");

template <bool FAULTS, bool TRACE>
const void* ens_kernel(int topo, int alg, uint32_t P) {
    if (alg == GOSSIP) {
        switch (topo) {
            case LINE: return reinterpret_cast<const void*>(&k_ens_gossip<LINE, FAULTS, TRACE>);
            case FULL: return reinterpret_cast<const void*>(&k_ens_gossip<FULL, FAULTS, TRACE>);
            case GRID3D: return reinterpret_cast<const void*>(&k_ens_gossip<GRID3D, FAULTS, TRACE>);
            case IMP3D: return reinterpret_cast<const void*>(&k_ens_gossip<IMP3D, FAULTS, TRACE>);
            case GRAPH: return reinterpret_cast<const void*>(&k_ens_gossip<GRAPH, FAULTS, TRACE>);
            default: return nullptr;
        }
    }
    const int npt = ens_npt(P);
    switch (topo) {
        case LINE: return ps_kernel<LINE, FAULTS, TRACE>(npt);
        case FULL: return ps_kernel<FULL, FAULTS, TRACE>(npt);
        case GRID3D: return ps_kernel<GRID3D, FAULTS, TRACE>(npt);
        case IMP3D: return ps_kernel<IMP3D, FAULTS, TRACE>(npt);
        case GRAPH: return ps_kernel<GRAPH, FAULTS, TRACE>(npt);
        default: return nullptr;
    }
}

}  // namespace

// graph_lds: the image of the handle's graph (GRAPH only: its LDS size has an edge count in it).
template <bool FAULTS, bool TRACE>
hipError_t ens_setup_t(int topo, int alg, uint32_t P, uint32_t graph_lds) {
    constexpr EnsVariant v{FAULTS, TRACE};
    const void* k = ens_kernel<FAULTS, TRACE>(topo, alg, P);
    if (!k) return hipErrorInvalidValue;  // a missing kernel is an error
    if (topo == GRAPH) {
        if (P > ENS_GRAPH_POP_MAX || graph_lds > ENS_LDS_MAX) return hipErrorInvalidValue;
        return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)graph_lds);
    }
    if (P > ens_max_population(topo, alg, v)) return hipErrorInvalidValue;
    return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ens_lds_bytes(topo, alg, P, v));
}

template <bool FAULTS, bool TRACE>
hipError_t ens_launch_t(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st) {
    constexpr EnsVariant v{FAULTS, TRACE};
    const uint32_t P = a.G.P;
    const void* k = ens_kernel<FAULTS, TRACE>(topo, alg, P);
    if (!k) return hipErrorInvalidValue;
    uint64_t lds;
    if (topo == GRAPH) {
        lds = ens_graph_lds_bytes(alg, P, a.g_eout, a.g_ein, v);
        if (P > ENS_GRAPH_POP_MAX || lds > ENS_LDS_MAX) return hipErrorInvalidValue;
    } else {
        if (P > ens_max_population(topo, alg, v)) return hipErrorInvalidValue;
        lds = ens_lds_bytes(topo, alg, P, v);
    }
    const uint32_t threads = ens_threads(alg, P);
    // faults_draw stores whole waves' bitmap words; the trace reduces over whole waves
    if ((FAULTS || TRACE) && threads % 64u != 0) return hipErrorInvalidValue;
    EnsArgs copy = a;
    void* args[] = {&copy};
    return hipLaunchKernel(k, dim3(nblocks), dim3(threads), args, (size_t)lds, st);
}

}  // namespace gp
