// gp_values.hip -- push-sum over caller-supplied values and weights (include/gossip_hip.h,
// gp_set_values / gp_set_mean; SRS v1-V): the admissibility check
// and the write of the initial (s, w), both plain grid-stride kernels over a staged chunk, and
// the host loop that streams the caller's arrays through a bounded pinned buffer.
//
//   k_values_check  one 16-byte load per node where weights are given (the chunk is staged as
//                   (x, w) pairs), else one 8-byte load; a lane keeps the first entry it finds
//                   inadmissible (it visits ascending ids), a wave folds its lanes' verdict words
//                   with shuffles, the wave leaders meet in LDS, and thread 0 issues the
//                   workgroup's one atomic minimum on the packed (id, rule) word -- and none at
//                   all when the workgroup found nothing, the usual case.
//   k_values_write  sw[0][id - base] = (x, w): one 16-byte store per node, consecutive lanes on
//                   consecutive nodes.
//   k_values_split  the same chunk as two arrays of doubles, what the ensemble kernels read
//                   (gp_ensemble_create_values).
//
// All or nothing: every chunk of a call is checked before any is written.  A call that fits the
// staging buffer is uploaded once; a longer one twice, so a caller loading a large network does
// best with calls of at most VAL_STAGE_BYTES / 16 nodes (/ 8 without weights).
#include "gp_host.hpp"

namespace gp {

namespace {

constexpr int VAL_THREADS = 256;
constexpr int VAL_WAVES = VAL_THREADS / 64;
constexpr int VAL_BLOCKS_PER_CU = 8;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// xw: the chunk as (x, w) pairs, or null: x alone, every weight 1.  id0: node id of entry 0.
__global__ __launch_bounds__(VAL_THREADS) void k_values_check(const double2* xw, const double* x, uint32_t n,
                                                              uint64_t id0, unsigned long long* bad) {
    __shared__ unsigned long long sh[VAL_WAVES];
    unsigned long long worst = VAL_NONE;
    for (uint32_t i = blockIdx.x * VAL_THREADS + threadIdx.x; i < n; i += gridDim.x * VAL_THREADS) {
        double xv, wv = 1.0;
        if (xw) {
            const double2 v = ld_global(xw + i);
            xv = v.x;
            wv = v.y;
        } else {
            xv = x[i];
        }
        const uint32_t rule = values_rule(xv, wv);
        if (rule != VAL_OK && worst == VAL_NONE) worst = val_pack(id0 + i, rule);  // (ascending i: the lane's lowest)
    }
    worst = wave_min_u64(worst);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = worst;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < VAL_WAVES; ++k) worst = sh[k] < worst ? sh[k] : worst;
        if (worst != VAL_NONE) atomicMin(bad, worst);
    }
}

__global__ __launch_bounds__(VAL_THREADS) void k_values_write(const double2* xw, const double* x, uint32_t n,
                                                              double2* dst) {
    for (uint32_t i = blockIdx.x * VAL_THREADS + threadIdx.x; i < n; i += gridDim.x * VAL_THREADS)
        st_global(dst + i, xw ? ld_global(xw + i) : make_double2(x[i], 1.0));
}

// The chunk as two arrays (EnsArgs::x0 / w0): a 16-byte load and two 8-byte stores per node, or a copy.
__global__ __launch_bounds__(VAL_THREADS) void k_values_split(const double2* xw, const double* x, uint32_t n,
                                                              double* xo, double* wo) {
    for (uint32_t i = blockIdx.x * VAL_THREADS + threadIdx.x; i < n; i += gridDim.x * VAL_THREADS) {
        if (xw) {
            const double2 v = ld_global(xw + i);
            xo[i] = v.x;
            wo[i] = v.y;
        } else {
            xo[i] = x[i];
        }
    }
}

int val_grid(uint32_t n, int cus) {
    const int need = (int)((n + VAL_THREADS - 1) / VAL_THREADS);
    return std::max(1, std::min(need, std::max(1, cus) * VAL_BLOCKS_PER_CU));
}

int stage_reserve(ValStage& st, size_t need) {
    if (st.bytes >= need) return GP_OK;
    values_stage_free(st);
    if (hipHostMalloc(&st.pin, need, hipHostMallocDefault) != hipSuccess || hipMalloc(&st.dev, need) != hipSuccess ||
        hipMalloc((void**)&st.bad, sizeof(unsigned long long)) != hipSuccess) {
        values_stage_free(st);
        set_err("the values staging buffer (%zu bytes, pinned and on the device) could not be allocated", need);
        return GP_ENOMEM;
    }
    st.bytes = need;
    return GP_OK;
}

const char* rule_text(uint32_t rule) {
    switch (rule) {
        case VAL_X_SIGN: return "the value must be finite with the sign bit clear (no -0.0, inf or NaN)";
        case VAL_W_SIGN: return "the weight must be finite with the sign bit clear (no -0.0, inf or NaN)";
        case VAL_W_RANGE: return "the weight must lie in [2^-32, 2^32]";
        case VAL_X_TINY: return "the value must be 0 or at least 2^-64";
        case VAL_RATIO: return "value * 2^-32 must be below the weight (every ratio stays under 2^32)";
        default: return "unknown rule";
    }
}

}  // namespace

void values_stage_free(ValStage& st) {
    if (st.pin) (void)hipHostFree(st.pin);
    if (st.dev) (void)hipFree(st.dev);
    if (st.bad) (void)hipFree(st.bad);
    st = ValStage{};
}

hipError_t launch_values_write(const void* staged, bool weighted, uint32_t n, double2* dst, int cus, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_values_write, dim3(val_grid(n, cus)), dim3(VAL_THREADS), 0, st,
                       weighted ? static_cast<const double2*>(staged) : nullptr,
                       weighted ? nullptr : static_cast<const double*>(staged), n, dst);
    return hipGetLastError();
}

hipError_t launch_values_split(const void* staged, bool weighted, uint32_t n, double* x, double* w, int cus,
                               hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_values_split, dim3(val_grid(n, cus)), dim3(VAL_THREADS), 0, st,
                       weighted ? static_cast<const double2*>(staged) : nullptr,
                       weighted ? nullptr : static_cast<const double*>(staged), n, x, w);
    return hipGetLastError();
}

int values_stream(ValStage& st, hipStream_t stream, int cus, const char* who, const double* x, const double* w,
                  int64_t count, int64_t id0, ValSink* sink) {
    if (count <= 0) return GP_OK;
    const bool weighted = w != nullptr;
    const size_t per = weighted ? 16 : 8;
    // two halves: the host fills one while the other's upload and kernels run
    const size_t want = std::min<size_t>(VAL_STAGE_BYTES, std::max<size_t>(2 * per * (size_t)count, 8192));
    int rc = stage_reserve(st, want);
    if (rc) return rc;
    const int64_t half = (int64_t)(st.bytes / 2 / per);  // entries per chunk
    const int64_t nchunks = (count + half - 1) / half;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int k = 0; k < 2; ++k)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } guard{ev};
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    bool used[2] = {false, false};
    // chunk q of the input into half q % 2 of the pinned buffer and on to the device's
    auto upload = [&](int64_t q, const void** staged, int64_t* c0, int64_t* c1) -> int {
        const int h = (int)(q & 1);
        if (used[h]) HIP_TRY(hipEventSynchronize(ev[h]));  // its last user is done with it
        *c0 = q * half;
        *c1 = std::min(count, *c0 + half);
        const size_t n = (size_t)(*c1 - *c0), off = (size_t)h * (st.bytes / 2);
        uint8_t* pin = static_cast<uint8_t*>(st.pin) + off;
        if (weighted) {
            double* p = reinterpret_cast<double*>(pin);
            for (size_t i = 0; i < n; ++i) {
                p[2 * i] = x[*c0 + (int64_t)i];
                p[2 * i + 1] = w[*c0 + (int64_t)i];
            }
        } else {
            std::memcpy(pin, x + *c0, n * 8);
        }
        uint8_t* dev = static_cast<uint8_t*>(st.dev) + off;
        HIP_TRY(hipMemcpyAsync(dev, pin, n * per, hipMemcpyHostToDevice, stream));
        *staged = dev;
        return GP_OK;
    };
    auto release = [&](int64_t q) -> int {
        HIP_TRY(hipEventRecord(ev[q & 1], stream));
        used[q & 1] = true;
        return GP_OK;
    };
    HIP_TRY(hipMemsetAsync(st.bad, 0xFF, sizeof(unsigned long long), stream));
    const void* staged = nullptr;
    int64_t c0 = 0, c1 = 0;
    for (int64_t q = 0; q < nchunks; ++q) {
        if ((rc = upload(q, &staged, &c0, &c1))) return rc;
        const uint32_t n = (uint32_t)(c1 - c0);
        hipLaunchKernelGGL(k_values_check, dim3(val_grid(n, cus)), dim3(VAL_THREADS), 0, stream,
                           weighted ? static_cast<const double2*>(staged) : nullptr,
                           weighted ? nullptr : static_cast<const double*>(staged), n, (uint64_t)(id0 + c0), st.bad);
        HIP_TRY(hipGetLastError());
        if ((rc = release(q))) return rc;
    }
    unsigned long long bad = VAL_NONE;
    HIP_TRY(hipMemcpyAsync(&bad, st.bad, sizeof bad, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad != VAL_NONE) {
        const int64_t id = (int64_t)(bad >> 3), i = id - id0;
        set_err("%s: node %lld (x = %g, w = %g): %s", who, (long long)id, x[i], w ? w[i] : 1.0,
                rule_text((uint32_t)(bad & 7u)));
        return GP_EINVAL;
    }
    if (!sink) return GP_OK;
    for (int64_t q = 0; q < nchunks; ++q) {
        if (nchunks > 1) {
            if ((rc = upload(q, &staged, &c0, &c1))) return rc;
        }  // (else: the one chunk is still staged)
        if ((rc = sink->write(staged, weighted, c0, c1, stream))) return rc;
        if ((rc = release(q))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return GP_OK;
}

}  // namespace gp

extern "C" {

int gp_set_values(gp_sim* s, int64_t first, int64_t count, const double* x, const double* w) {
    if (!s) {
        set_err("gp_set_values: null handle");
        return GP_EINVAL;
    }
    if (s->cfg.algorithm != GP_PUSHSUM) {
        set_err("gp_set_values: gossip has no values (the handle runs gossip)");
        return GP_EINVAL;
    }
    if (s->rounds_done > 0) {
        set_err("gp_set_values: the handle has run %lld rounds; values are the initial state", (long long)s->rounds_done);
        return GP_ESTATE;
    }
    const bool rccl = s->mode == MODE_RCCL;
    const int64_t lo = rccl ? (int64_t)s->slab[0].S.lo : 0, hi = rccl ? (int64_t)s->slab[0].hi : s->P;
    if (first < lo || count < 0 || first > hi || count > hi - first) {
        set_err("gp_set_values: range [%lld, +%lld) outside the ids [%lld, %lld) this handle owns", (long long)first,
                (long long)count, (long long)lo, (long long)hi);
        return GP_EINVAL;
    }
    if (count > 0 && !x) {
        set_err("gp_set_values: x is null");
        return GP_EINVAL;
    }
    // several slabs on a lattice: round 0's halo planes and random-edge lists were packed at create
    // from the state as it was; gp_step sends them again before the first round -- after a call
    // that wrote, or an empty one (the ranks of an RCCL run agree through those); a refused call
    // leaves the handle as it was
    const bool resend = s->world > 1 && s->cfg.topology != GP_FULL;
    if (count == 0) {
        if (resend) s->values_dirty = true;
        return GP_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    struct Sink : ValSink {
        gp_sim* s;
        int64_t first;
        int write(const void* staged, bool weighted, int64_t c0, int64_t c1, hipStream_t st) override {
            const size_t per = weighted ? 16 : 8;
            for (const Slab& sl : s->slab) {  // each id to its slab's array (base != lo)
                const DevState& S = sl.S;
                const int64_t a = std::max<int64_t>(first + c0, S.lo), b = std::min<int64_t>(first + c1, sl.hi);
                if (a >= b) continue;
                const uint8_t* src = static_cast<const uint8_t*>(staged) + (size_t)(a - (first + c0)) * per;
                HIP_TRY(launch_values_write(src, weighted, (uint32_t)(b - a), S.sw[0] + (a - S.base), s->cus, st));
            }
            return GP_OK;
        }
    } sink;
    sink.s = s;
    sink.first = first;
    const int rc = values_stream(s->vstage, s->stream, s->cus, "gp_set_values", x, w, count, first, &sink);
    if (rc == GP_OK && resend) s->values_dirty = true;
    return rc;
}

int gp_set_mean(gp_sim* s, double mean) {
    if (!s) {
        set_err("gp_set_mean: null handle");
        return GP_EINVAL;
    }
    if (s->cfg.algorithm != GP_PUSHSUM) {
        set_err("gp_set_mean: gossip has no values (the handle runs gossip)");
        return GP_EINVAL;
    }
    if (!mean_ok(mean)) {
        set_err("gp_set_mean: mean must be finite, >= 0 and < 2^32 (got %g)", mean);
        return GP_EINVAL;
    }
    s->mean = mean;
    return GP_OK;
}

}  // extern "C"
