// gp_summary.hip -- state summaries (include/gossip_hip.h, gp_summary): what a run
// computed, reduced where the state lives.  One bandwidth-bound pass over a slab's state -- 17 B
// per push-sum node ((s, w) as one 16-byte load, the node byte as a quarter of a word load), 4 B per
// gossip node (four counters per 16-byte load) -- by a persistent grid:
//
//   lane   accumulates its nodes in ascending id order: counts, min / max, the largest |e| with
//          its node id, and the three sums as double-doubles (TwoSum: gp_summary.hpp);
//   wave   folds its 64 lanes with shuffles (no LDS);
//   group  wave leaders leave their records in LDS (one record each, written by separate
//          instructions: no bank conflict), thread 0 joins them in wave order and writes the
//          workgroup's partial record to HBM;
//   grid   a second, single-workgroup launch joins the partial records in ascending order.
//
// No floating-point atomics, and no step depends on the order in which workgroups run: the same
// state gives the same bytes.  The join is associative and commutative in every field but the
// double-double sums, whose order is fixed by the grid (a function of the slab size and the
// device's CU count).  The estimate is the compiler's IEEE fp64 divide; nothing here may be
// contracted (-ffp-contract=off, csrc/Makefile).
//
// Also here: gp_summary_take (the slabs of a handle, and the gather over the ranks' communicator
// for GP_SCOPE_GLOBAL) and gp_summary_merge.
#include "gp_host.hpp"
#pragma GCC visibility push(hidden)
#include "gp_summary_dev.hpp"
#pragma GCC visibility pop

namespace gp {

namespace {

constexpr int SUM_WAVES = SUM_THREADS / 64;
constexpr uint32_t PS_SEG = 256;    // push-sum: nodes a wave takes per step (64 flag words, 4 (s, w) loads a lane)
constexpr uint32_t GO_SEG = 1024;   // gossip: nodes a wave takes per step (4 16-byte loads a lane)

__device__ __forceinline__ void acc_init(SumAcc& a) {
    a.active = a.conv = a.within = 0;
    a.err_node = ~0ull;
    for (int k = 0; k < 12; ++k) a.hist[k] = 0;
    a.est_min = a.w_min = __builtin_huge_val();
    a.est_max = a.w_max = -__builtin_huge_val();
    a.err_max = -1.0;  // below every |e|
    a.ss[0] = a.ss[1] = a.sw[0] = a.sw[1] = a.sq[0] = a.sq[1] = 0.0;
    a.c_max = 0;
    a.pad = 0;
}

// a = a joined with b (the fields of the algorithm only).
template <int ALG>
__device__ __forceinline__ void acc_join(SumAcc& a, const SumAcc& b) {
    a.active += b.active;
    a.conv += b.conv;
    if (ALG == GOSSIP) {
#pragma unroll
        for (int k = 0; k < 12; ++k) a.hist[k] += b.hist[k];
        a.c_max = b.c_max > a.c_max ? b.c_max : a.c_max;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.hist[k] += b.hist[k];
        a.within += b.within;
        if (b.est_min < a.est_min) a.est_min = b.est_min;
        if (b.est_max > a.est_max) a.est_max = b.est_max;
        if (b.w_min < a.w_min) a.w_min = b.w_min;
        if (b.w_max > a.w_max) a.w_max = b.w_max;
        if (err_beats(b.err_max, b.err_node, a.err_max, a.err_node)) {
            a.err_max = b.err_max;
            a.err_node = b.err_node;
        }
        dd_add(a.ss[0], a.ss[1], b.ss[0], b.ss[1]);
        dd_add(a.sw[0], a.sw[1], b.sw[0], b.sw[1]);
        dd_add(a.sq[0], a.sq[1], b.sq[0], b.sq[1]);
    }
}

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, int off) {
    const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_down_f64(double v, int off) {
    return __longlong_as_double((long long)shfl_down_u64((unsigned long long)__double_as_longlong(v), off));
}

// Lane l joins lane l + off's record (lanes without a partner join their own: only lane 0's
// result is used, and its tree never takes from such a lane).
template <int ALG>
__device__ __forceinline__ void acc_join_down(SumAcc& a, int off) {
    SumAcc b;
    acc_init(b);
    b.active = shfl_down_u64(a.active, off);
    b.conv = shfl_down_u64(a.conv, off);
    if (ALG == GOSSIP) {
#pragma unroll
        for (int k = 0; k < 12; ++k) b.hist[k] = shfl_down_u64(a.hist[k], off);
        b.c_max = __shfl_down(a.c_max, off, 64);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) b.hist[k] = shfl_down_u64(a.hist[k], off);
        b.within = shfl_down_u64(a.within, off);
        b.err_node = shfl_down_u64(a.err_node, off);
        b.est_min = shfl_down_f64(a.est_min, off);
        b.est_max = shfl_down_f64(a.est_max, off);
        b.w_min = shfl_down_f64(a.w_min, off);
        b.w_max = shfl_down_f64(a.w_max, off);
        b.err_max = shfl_down_f64(a.err_max, off);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            b.ss[k] = shfl_down_f64(a.ss[k], off);
            b.sw[k] = shfl_down_f64(a.sw[k], off);
            b.sq[k] = shfl_down_f64(a.sq[k], off);
        }
    }
    acc_join<ALG>(a, b);
}

// The workgroup's lanes into one record at *out (written by thread 0).  Every thread calls it.
template <int ALG>
__device__ __forceinline__ void block_fold(SumAcc& a, SumAcc* out) {
    __shared__ SumAcc sh[SUM_WAVES];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc_join_down<ALG>(a, off);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        SumAcc r = sh[0];
        for (int w = 1; w < SUM_WAVES; ++w) acc_join<ALG>(r, sh[w]);
        *out = r;
    }
}

// One push-sum node: s, w, and its flags as gp_read_state reports them.
__device__ __forceinline__ void node_ps(SumAcc& a, double s, double w, uint32_t act, uint32_t conv, uint32_t cnt,
                                        uint64_t id, double mu, double tol) {
    const double est = s / w;
    const double e = est - mu;
    const double ae = __builtin_fabs(e);
    a.active += act;
    a.conv += conv;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) a.hist[k] += cnt == k ? 1u : 0u;
    if (est < a.est_min) a.est_min = est;
    if (est > a.est_max) a.est_max = est;
    if (w < a.w_min) a.w_min = w;
    if (w > a.w_max) a.w_max = w;
    if (err_beats(ae, id, a.err_max, a.err_node)) {
        a.err_max = ae;
        a.err_node = id;
    }
    a.within += ae <= tol ? 1u : 0u;
    dd_add_d(a.ss[0], a.ss[1], s);
    dd_add_d(a.sw[0], a.sw[1], w);
    dd_add_d(a.sq[0], a.sq[1], e * e);
}

// One gossip node: its rumour counter; the flags derive from it and the seed node (gp_read_state).
__device__ __forceinline__ void node_gossip(SumAcc& a, int32_t c, uint64_t id, uint32_t seed_node) {
    const bool act = (id == seed_node || c >= 1) && c <= 10;
    a.active += act ? 1u : 0u;
    a.conv += c >= (int32_t)GOSSIP_DONE ? 1u : 0u;
    const int32_t cc = c > 11 ? 11 : c;
#pragma unroll
    for (int k = 0; k < 12; ++k) a.hist[k] += cc == k ? 1u : 0u;
    a.c_max = c > a.c_max ? c : a.c_max;
}

// Push-sum.  The arrays are walked in segments of PS_SEG array indices, aligned in index space (so
// every flag word is an aligned word of the node-byte array and every (s, w) load instruction of a
// wave covers one KiB-aligned KiB), whichever index the slab's first owned node has; indices
// outside [a0, a0 + n) are masked.  Wave v of the grid takes segments v, v + waves, ...: a lane
// sees ascending ids.  Per step a lane has its flag word and four 16-byte (s, w) loads in flight;
// node k * 64 + lane's byte is byte lane % 4 of the word lane k * 16 + lane / 4 loaded.
__global__ __launch_bounds__(SUM_THREADS) void k_summary_ps(SummaryArgs A) {
    SumAcc acc;
    acc_init(acc);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lo = A.a0, hi = (uint64_t)A.a0 + A.n;
    const uint64_t seg1 = (hi + PS_SEG - 1) / PS_SEG;
    const uint64_t nw = (uint64_t)gridDim.x * SUM_WAVES;
    for (uint64_t seg = lo / PS_SEG + (uint64_t)blockIdx.x * SUM_WAVES + wave; seg < seg1; seg += nw) {
        const uint64_t b = seg * PS_SEG;
        const uint64_t wa = b + 4u * lane;
        uint32_t word = 0;
        if (wa >= lo && wa + 4 <= hi) {
            word = *reinterpret_cast<const uint32_t*>(A.nb + wa);
        } else {  // a word the range covers in part: its bytes one by one
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (wa + j >= lo && wa + j < hi) word |= (uint32_t)A.nb[wa + j] << (8u * j);
        }
        double2 v[4];
        bool ok[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t idx = b + k * 64u + lane;
            ok[k] = idx >= lo && idx < hi;
            v[k] = make_double2(0.0, 1.0);
            if (ok[k]) v[k] = ld_global(A.sw + idx);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t wv = __shfl(word, (int)(k * 16u + (lane >> 2)), 64);
            const uint32_t bb = (wv >> (8u * (lane & 3u))) & 0xFFu;
            if (ok[k])
                node_ps(acc, v[k].x, v[k].y, (bb & B_ACTIVE) ? 1u : 0u, (bb & B_CONV) ? 1u : 0u,
                        (bb >> CNT_SHIFT) & 3u, (uint64_t)A.id0 + b + k * 64u + lane, A.mu, A.tol);
        }
    }
    block_fold<PUSHSUM>(acc, &A.part[blockIdx.x]);
}

// Gossip.  A lane takes four consecutive counters per 16-byte load, four loads per step.
__global__ __launch_bounds__(SUM_THREADS) void k_summary_gossip(SummaryArgs A) {
    SumAcc acc;
    acc_init(acc);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n = A.n;
    const uint64_t seg1 = (n + GO_SEG - 1) / GO_SEG;
    const uint64_t nw = (uint64_t)gridDim.x * SUM_WAVES;
    for (uint64_t seg = (uint64_t)blockIdx.x * SUM_WAVES + wave; seg < seg1; seg += nw) {
        const uint64_t b = seg * GO_SEG;
        int4 v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t idx = b + j * 256u + 4u * lane;
            v[j] = make_int4(0, 0, 0, 0);
            if (idx + 4 <= n) {
                v[j] = *reinterpret_cast<const int4*>(A.c + idx);
            } else {  // the slab's last, partial quad
                if (idx < n) v[j].x = A.c[idx];
                if (idx + 1 < n) v[j].y = A.c[idx + 1];
                if (idx + 2 < n) v[j].z = A.c[idx + 2];
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t idx = b + j * 256u + 4u * lane;
            const uint64_t id = (uint64_t)A.id0 + idx;
            if (idx < n) node_gossip(acc, v[j].x, id, A.seed_node);
            if (idx + 1 < n) node_gossip(acc, v[j].y, id + 1, A.seed_node);
            if (idx + 2 < n) node_gossip(acc, v[j].z, id + 2, A.seed_node);
            if (idx + 3 < n) node_gossip(acc, v[j].w, id + 3, A.seed_node);
        }
    }
    block_fold<GOSSIP>(acc, &A.part[blockIdx.x]);
}

// The grid's partial records into one: thread t joins a contiguous run of records in ascending
// order, the workgroup folds its threads (lower runs first).
template <int ALG>
__global__ __launch_bounds__(SUM_THREADS) void k_summary_fold(const SumAcc* part, uint32_t nparts, SumAcc* out) {
    SumAcc acc;
    acc_init(acc);
    const uint32_t per = (nparts + SUM_THREADS - 1) / SUM_THREADS;
    const uint32_t p0 = threadIdx.x * per, p1 = p0 + per < nparts ? p0 + per : nparts;
    for (uint32_t p = p0; p < p1; ++p) acc_join<ALG>(acc, part[p]);
    block_fold<ALG>(acc, out);
}

// Ensemble members: workgroup m reduces member m (P <= 8191: one workgroup is enough).
template <int ALG>
__global__ __launch_bounds__(SUM_THREADS) void k_summary_ens(SumEnsArgs A) {
    SumAcc acc;
    acc_init(acc);
    const uint32_t m = blockIdx.x;
    const size_t at = (size_t)m * A.P;
    if (ALG == GOSSIP) {
        const uint32_t seed_node = (uint32_t)A.rec[m].seed_node;
        for (uint32_t i = threadIdx.x; i < A.P; i += SUM_THREADS) node_gossip(acc, A.c[at + i], i, seed_node);
    } else {
        for (uint32_t i = threadIdx.x; i < A.P; i += SUM_THREADS) {
            const uint32_t f = A.fl[at + i];
            node_ps(acc, A.s[at + i], A.w[at + i], f & 1u, (f >> 1) & 1u, (f >> 2) & 3u, i, A.mu, A.tol);
        }
    }
    block_fold<ALG>(acc, &A.out[m]);
}

}  // namespace

uint32_t summary_blocks(int alg, uint32_t a0, uint32_t n, int cus) {
    uint64_t segs;
    if (alg == PUSHSUM) segs = ((uint64_t)a0 + n + PS_SEG - 1) / PS_SEG - a0 / PS_SEG;
    else segs = ((uint64_t)n + GO_SEG - 1) / GO_SEG;
    const uint64_t need = std::max<uint64_t>(1, (segs + SUM_WAVES - 1) / SUM_WAVES);
    return (uint32_t)std::min<uint64_t>(need, (uint64_t)std::max(1, cus) * SUM_BLOCKS_PER_CU);
}

hipError_t summary_launch(int alg, const SummaryArgs& a, uint32_t blocks, hipStream_t st) {
    if (alg == PUSHSUM) hipLaunchKernelGGL(k_summary_ps, dim3(blocks), dim3(SUM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_summary_gossip, dim3(blocks), dim3(SUM_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t summary_fold(int alg, const SumAcc* part, uint32_t nparts, SumAcc* out, hipStream_t st) {
    if (alg == PUSHSUM) hipLaunchKernelGGL(k_summary_fold<PUSHSUM>, dim3(1), dim3(SUM_THREADS), 0, st, part, nparts, out);
    else hipLaunchKernelGGL(k_summary_fold<GOSSIP>, dim3(1), dim3(SUM_THREADS), 0, st, part, nparts, out);
    return hipGetLastError();
}

hipError_t summary_ens_launch(int alg, const SumEnsArgs& a, uint32_t nseeds, hipStream_t st) {
    if (alg == PUSHSUM) hipLaunchKernelGGL(k_summary_ens<PUSHSUM>, dim3(nseeds), dim3(SUM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_summary_ens<GOSSIP>, dim3(nseeds), dim3(SUM_THREADS), 0, st, a);
    return hipGetLastError();
}

void summary_from_acc(const SumAcc& a, int alg, int64_t first, int64_t count, int64_t P, int64_t rounds, double tol,
                      gp_summary* out) {
    gp_summary r;
    std::memset(&r, 0, sizeof r);
    r.first = first;
    r.count = count;
    r.population = P;
    r.rounds = rounds;
    r.algorithm = alg == PUSHSUM ? GP_PUSHSUM : GP_GOSSIP;
    r.active = (int64_t)a.active;
    r.converged = (int64_t)a.conv;
    r.tol = tol;
    if (alg == GOSSIP) {
        for (int k = 0; k < 12; ++k) r.c_hist[k] = (int64_t)a.hist[k];
        r.c_max = a.c_max;
    } else {
        for (int k = 0; k < 4; ++k) r.cnt_hist[k] = (int64_t)a.hist[k];
        r.est_min = a.est_min;
        r.est_max = a.est_max;
        r.w_min = a.w_min;
        r.w_max = a.w_max;
        r.err_max = a.err_max;
        r.err_max_node = (int64_t)a.err_node;
        r.within_tol = (int64_t)a.within;
        for (int k = 0; k < 2; ++k) {
            r.sum_s[k] = a.ss[k];
            r.sum_w[k] = a.sw[k];
            r.sum_sqerr[k] = a.sq[k];
        }
    }
    *out = r;
}

}  // namespace gp

namespace {

// The handle's summary scratch: the workgroups' partial records, the folded record, and (RCCL)
// the ranks' gathered gp_summary bytes.  Allocated at the first summary, freed with the handle.
int summary_scratch(gp_sim* s, size_t nparts, SumAcc** part, SumAcc** res, uint8_t** gather) {
    const size_t recs = nparts + 1;
    const size_t gbytes = s->mode == MODE_RCCL ? sizeof(gp_summary) * (size_t)s->world : 0;
    const size_t bytes = recs * sizeof(SumAcc) + gbytes;
    if (!s->sum_scratch || s->sum_scratch_bytes < bytes) {
        void* p = nullptr;
        const int rc = dev_alloc(s, &p, bytes);
        if (rc) return rc;
        s->sum_scratch = p;
        s->sum_scratch_bytes = bytes;
    }
    *part = static_cast<SumAcc*>(s->sum_scratch);
    *res = *part + nparts;
    *gather = reinterpret_cast<uint8_t*>(*part + recs);
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_summary_take(gp_sim* s, double tol, int32_t scope, gp_summary* out) {
    if (!s || !out) {
        set_err("gp_summary_take: null argument");
        return GP_EINVAL;
    }
    if (!(tol >= 0.0) || !std::isfinite(tol)) {
        set_err("gp_summary_take: tol must be finite and >= 0 (got %g)", tol);
        return GP_EINVAL;
    }
    if (scope != GP_SCOPE_LOCAL && scope != GP_SCOPE_GLOBAL) {
        set_err("gp_summary_take: unknown scope %d (GP_SCOPE_LOCAL | GP_SCOPE_GLOBAL)", scope);
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int alg = s->slab[0].S.alg;
    const int cur = (int)(s->rounds_done & 1);
    // the persistent grid's workgroups are shared among the slabs of a virtual-rank handle
    std::vector<uint32_t> blocks(s->slab.size());
    size_t nparts = 0;
    for (size_t q = 0; q < s->slab.size(); ++q) {
        const DevState& S = s->slab[q].S;
        blocks[q] = summary_blocks(alg, alg == PUSHSUM ? S.lo - S.base : 0u, S.nloc, s->cus);
        nparts += blocks[q];
    }
    SumAcc *part = nullptr, *res = nullptr;
    uint8_t* gather = nullptr;
    int rc = summary_scratch(s, nparts, &part, &res, &gather);
    if (rc) return rc;
    size_t at = 0;
    for (size_t q = 0; q < s->slab.size(); ++q) {
        const DevState& S = s->slab[q].S;
        SummaryArgs a{};
        if (alg == PUSHSUM) {
            a.sw = S.sw[cur];
            a.nb = S.topo == FULL ? S.nb[0] : S.nb[cur];
            a.a0 = S.lo - S.base;
            a.id0 = S.base;
        } else {
            a.c = S.c;
            a.a0 = 0;
            a.id0 = S.lo;
        }
        a.n = S.nloc;
        a.seed_node = S.seed_node;
        a.mu = s->mean;
        a.tol = tol;
        a.part = part + at;
        HIP_TRY(summary_launch(alg, a, blocks[q], s->stream));
        at += blocks[q];
    }
    HIP_TRY(summary_fold(alg, part, (uint32_t)nparts, res, s->stream));
    SumAcc h;
    HIP_TRY(hipMemcpyAsync(&h, res, sizeof h, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    gp_summary loc;
    const bool rccl = s->mode == MODE_RCCL;
    summary_from_acc(h, alg, rccl ? (int64_t)s->slab[0].S.lo : 0, rccl ? (int64_t)s->slab[0].S.nloc : s->P, s->P,
                     s->rounds_done, tol, &loc);
    if (!rccl || scope == GP_SCOPE_LOCAL) {
        *out = loc;
        return GP_OK;
    }
    // every rank's record, in rank order, over the run's communicator; joined on the host
    const size_t B = sizeof(gp_summary);
    uint8_t* mine = gather + B * (size_t)s->rank;
    HIP_TRY(hipMemcpyAsync(mine, &loc, B, hipMemcpyHostToDevice, s->stream));
    NCCL_TRY(ncclAllGather(mine, gather, B, ncclUint8, s->comm, s->stream));
    std::vector<gp_summary> all((size_t)s->world);
    HIP_TRY(hipMemcpyAsync(all.data(), gather, B * all.size(), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    gp_summary acc = all[0];
    for (int r = 1; r < s->world; ++r) {
        if (summary_merge(&acc, &all[(size_t)r], &acc) != GP_OK) {
            set_err("gp_summary_take: rank %d's summary does not join rank %d's (ids [%lld, +%lld) after [%lld, +%lld), "
                    "rounds %lld / %lld): every rank must call with the same tol at the same round",
                    r, r - 1, (long long)all[(size_t)r].first, (long long)all[(size_t)r].count, (long long)acc.first,
                    (long long)acc.count, (long long)all[(size_t)r].rounds, (long long)acc.rounds);
            return GP_ESTATE;
        }
    }
    *out = acc;
    return GP_OK;
}

int gp_summary_merge(const gp_summary* a, const gp_summary* b, gp_summary* out) {
    if (!a || !b || !out) {
        set_err("gp_summary_merge: null argument");
        return GP_EINVAL;
    }
    if (summary_merge(a, b, out) != GP_OK) {
        set_err("gp_summary_merge: the summaries do not join: ids [%lld, +%lld) and [%lld, +%lld) must be adjacent, and "
                "population, rounds, algorithm and tol equal",
                (long long)a->first, (long long)a->count, (long long)b->first, (long long)b->count);
        return GP_EINVAL;
    }
    return GP_OK;
}

}  // extern "C"
