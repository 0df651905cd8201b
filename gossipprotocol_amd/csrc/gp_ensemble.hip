// gp_ensemble.hip -- ensemble kernels: workgroup b simulates one whole network
// (member idx[b], seed rec[m].seed) with its node state in LDS and registers, a
// workgroup barrier between the phases of a round, no launch per round and no HBM
// traffic in the round loop.  Workgroups never talk to each other; a grid larger
// than what is resident simply queues.  DESIGN.md §9; layout: gp_ensemble.hpp.
//
// The rounds are SRS v1 exactly as the per-round kernels
// and the oracle run them: same Philox draws (gp_device.hpp), push-sum folded own
// half first, then lattice messages in the receiver's slot order, then random-edge
// / full messages by ascending sender id.  Built with -ffp-contract=off.
//
// Reference mapping (Program.fs = the reference's Project2/Program.fs): the actor
// loops Program.fs:84-131, the injector Program.fs:141-163 and the scheduler
// Program.fs:41-61 of one run; the setup Program.fs:169-176,193,221,258-263.
#include "gp_ensemble.hpp"

namespace gp {
namespace {

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

__device__ __forceinline__ void member_end(const EnsArgs& a, uint32_t m, const Member& M) {
    if (threadIdx.x != 0) return;
    gp_member* rec = a.rec + m;
    rec->rounds = M.rounds;
    rec->converged = M.alerts;
    rec->seed_node = M.seed_node;
    rec->status = M.alerts >= a.G.T ? GP_STATUS_CONVERGED
                  : M.rounds >= a.max_rounds ? GP_STATUS_MAX_ROUNDS : GP_STATUS_RUNNING;
    rec->reserved = (int32_t)M.live;
}

// Present-direction mask of node j (Imp3D: its lattice part).
template <int TOPO>
__device__ __forceinline__ uint32_t ens_mask(uint32_t j, const Geom& G) {
    return present_mask<(TOPO == LINE ? LINE : GRID3D)>(j, G);
}

// ------------------------------------------------------------------ gossip
// Per round (SRS v1 B.3): phase 1 every sending node draws a neighbour and bumps
// inc[target] iff the target is unconverged in c, which nobody writes in this phase
// (the round-start snapshot); wave 0 also runs the injector.  Phase 2 applies inc.
template <int TOPO>
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

    const uint32_t m = a.idx[blockIdx.x];
    Member M = member_begin(a, m);
    int32_t* gc = a.c + (size_t)m * P;
    uint32_t* gbits = TOPO == FULL ? nullptr : a.bits + (size_t)m * a.nwords;

    for (uint32_t i = tid; i < P; i += nthr) {
        c[i] = a.init ? 0 : gc[i];  // rumours = 0 (Program.fs:68)
        inc[i] = 0;
        // Imp3D random neighbour: Random().Next(0, nodes-1) -> [0, P-2] (Program.fs:259)
        if (TOPO == IMP3D) rnd[i] = (uint16_t)uniform(M.k0, M.k1, S_TOPO, i, 0, P - 1);
    }
    if (TOPO != FULL)
        for (uint32_t q = tid; q < a.nwords; q += nthr) {
            // injector list = ids 0..nodes-1 (Program.fs:147-148)
            const uint32_t rest = a.G.T - q * 32;
            bits[q] = a.init ? (rest >= 32 ? 0xFFFFFFFFu : (1u << rest) - 1u) : gbits[q];
        }
    if (tid == 0) hdr[0] = M.alerts;
    __syncthreads();

    for (int64_t it = 0; it < M.left && M.alerts < a.G.T; ++it) {
        const uint32_t r = (uint32_t)M.rounds;
        for (uint32_t i = tid; i < P; i += nthr) {
            const int32_t ci = c[i];
            if (!((i == M.seed_node || ci >= 1) && ci <= 10)) continue;  // Program.fs:85
            uint32_t t;
            if (TOPO == FULL) {
                t = full_target(i, uniform(M.k0, M.k1, S_GOSSIP, i, r, P - 1));
            } else {
                const uint32_t mask = ens_mask<TOPO>(i, a.G);
                const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                const uint32_t d = slot_to_dir(mask, uniform(M.k0, M.k1, S_GOSSIP, i, r, deg));
                t = (TOPO == IMP3D && d == DIR_RANDOM) ? (uint32_t)rnd[i] : nbr<(TOPO == LINE ? LINE : GRID3D)>(i, d, a.G);
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
                        if (c[t] >= (int32_t)GOSSIP_DONE) {
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
            if (c0 <= 10 && c1 > 10) atomicAdd(&hdr[0], 1u);  // Program.fs:91-98
            c[j] = c1;
            inc[j] = 0;
        }
        __syncthreads();
        M.alerts = hdr[0];
        M.rounds += 1;
    }

    for (uint32_t i = tid; i < P; i += nthr) gc[i] = c[i];
    if (TOPO != FULL)
        for (uint32_t q = tid; q < a.nwords; q += nthr) gbits[q] = bits[q];
    member_end(a, m, M);  // (thread 0 is in wave 0, which counted the injector's removals)
}

// ------------------------------------------------------------------ push-sum
// Thread t keeps nodes t, t + nthr, ... (NPT slots) in registers.  Per round (SRS
// v1 B.4): phase A every active node draws its direction, publishes it and its
// halves (s/2, w/2 -- the half it keeps and the half it sends are the same
// number) in LDS, and hooks itself into the target's list if the edge is a random
// one; phase B every node folds own half, then lattice senders in its own slot
// order (neighbour n sends to j iff dir[n] is the opposite of j's slot), then the
// list by ascending sender id, and runs the ratio test (Program.fs:114-123).
template <int TOPO, int NPT>
__global__ __launch_bounds__(ENS_THREADS) void k_ens_pushsum(const EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool LISTS = TOPO == FULL || TOPO == IMP3D;
    constexpr int LT = TOPO == LINE ? LINE : GRID3D;
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

    const uint32_t m = a.idx[blockIdx.x];
    Member M = member_begin(a, m);
    double* gs = a.s + (size_t)m * P;
    double* gw = a.w + (size_t)m * P;
    uint8_t* gf = a.fl + (size_t)m * P;

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
        if (TOPO != FULL) fl[q] |= ens_mask<TOPO>(i, a.G) << 8;
        if (LISTS) head[i] = ENS_NONE;
        if (TOPO == IMP3D) rnd[i] = (uint16_t)uniform(M.k0, M.k1, S_TOPO, i, 0, P - 1);
    }
    if (tid == 0) hdr[0] = M.alerts;
    __syncthreads();

    for (int64_t it = 0; it < M.left && M.alerts < a.G.T; ++it) {
        const uint32_t r = (uint32_t)M.rounds;
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t i = tid + q * nthr;
            if (i >= P) continue;
            uint32_t d = DIR_NONE;
            if (fl[q] & 1u) {
                uint32_t t = 0;
                if (TOPO == FULL) {
                    d = DIR_RANDOM;
                    t = full_target(i, uniform(M.k0, M.k1, S_PUSHSUM, i, r, P - 1));
                } else {
                    const uint32_t mask = (fl[q] >> 8) & 63u;
                    const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                    d = slot_to_dir(mask, uniform(M.k0, M.k1, S_PUSHSUM, i, r, deg));
                    if (TOPO == IMP3D) t = rnd[i];
                }
                hs[i] = s[q] * 0.5;
                hw[i] = w[q] * 0.5;
                if (LISTS && d == DIR_RANDOM) next[i] = (uint16_t)atomicExch(&head[t], i);
            }
            if (TOPO != FULL) dir[i] = (uint8_t)d;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t j = tid + q * nthr;
            if (j >= P) continue;
            const double s0 = s[q], w0 = w[q];
            double as = (fl[q] & 1u) ? s0 * 0.5 : s0;
            double aw = (fl[q] & 1u) ? w0 * 0.5 : w0;
            bool recv = false;
            if (TOPO != FULL) {
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
                        atomicAdd(&hdr[0], 1u);
                    }
                    fl[q] = (fl[q] & ~12u) | (cnt << 2);
                }
                fl[q] |= 1u;
            }
            s[q] = as;
            w[q] = aw;
        }
        __syncthreads();
        M.alerts = hdr[0];
        M.rounds += 1;
    }

#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const uint32_t i = tid + q * nthr;
        if (i >= P) continue;
        gs[i] = s[q];
        gw[i] = w[q];
        gf[i] = (uint8_t)(fl[q] & 15u);
    }
    member_end(a, m, M);
}

int ens_npt(uint32_t P) {
    int npt = 1;
    while ((uint32_t)npt * ENS_THREADS < P) npt *= 2;
    return npt;
}

uint32_t ens_threads(int alg, uint32_t P) {
    const uint32_t per = alg == PUSHSUM ? (P + ens_npt(P) - 1) / ens_npt(P) : P;
    const uint32_t t = (per + 63u) & ~63u;
    return t > (uint32_t)ENS_THREADS ? (uint32_t)ENS_THREADS : t;
}

template <int TOPO>
const void* ps_kernel(int npt) {
    switch (npt) {
        case 1: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 1>);
        case 2: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 2>);
        case 4: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 4>);
        case 8: return reinterpret_cast<const void*>(&k_ens_pushsum<TOPO, 8>);
        default: return nullptr;
    }
}
static_assert(ENS_NPT_MAX == 8, "ps_kernel lists the slot counts");

const void* ens_kernel(int topo, int alg, uint32_t P) {
    if (alg == GOSSIP) {
        switch (topo) {
            case LINE: return reinterpret_cast<const void*>(&k_ens_gossip<LINE>);
            case FULL: return reinterpret_cast<const void*>(&k_ens_gossip<FULL>);
            case GRID3D: return reinterpret_cast<const void*>(&k_ens_gossip<GRID3D>);
            case IMP3D: return reinterpret_cast<const void*>(&k_ens_gossip<IMP3D>);
            default: return nullptr;
        }
    }
    const int npt = ens_npt(P);
    switch (topo) {
        case LINE: return ps_kernel<LINE>(npt);
        case FULL: return ps_kernel<FULL>(npt);
        case GRID3D: return ps_kernel<GRID3D>(npt);
        case IMP3D: return ps_kernel<IMP3D>(npt);
        default: return nullptr;
    }
}

}  // namespace

hipError_t ens_setup(int topo, int alg, uint32_t P) {
    const void* k = ens_kernel(topo, alg, P);
    if (!k || P > ens_max_population(topo, alg)) return hipErrorInvalidValue;  // a missing kernel is an error
    return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ens_lds_bytes(topo, alg, P));
}

hipError_t ens_launch(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st) {
    const void* k = ens_kernel(topo, alg, a.G.P);
    if (!k || a.G.P > ens_max_population(topo, alg)) return hipErrorInvalidValue;
    EnsArgs copy = a;
    void* args[] = {&copy};
    return hipLaunchKernel(k, dim3(nblocks), dim3(ens_threads(alg, a.G.P)), args, ens_lds_bytes(topo, alg, a.G.P), st);
}

}  // namespace gp
