// gp_values.hpp -- caller-supplied push-sum values and weights (SRS v1-V, SURVEY.md B.6,
// DESIGN.md §13): the admissibility rules, shared by the check kernel and the host that words
// its verdict, and the host interface of gp_values.hip for gp_ensemble_api.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gp_device.hpp"

namespace gp {

// The rule an entry (x, w) breaks, lowest first; VAL_OK: admissible.
//   VAL_X_SIGN   x is finite with the sign bit clear (k_ps_block tags its steps in the sign bits,
//   VAL_W_SIGN   the tile kernel reads a negative s as an underflow); the same for w
//   VAL_W_RANGE  2^-32 <= w <= 2^32
//   VAL_X_TINY   x = 0 or x >= 2^-64
//   VAL_RATIO    x * 2^-32 < w (the scaling is exact: x is 0 or a normal number >= 2^-64), so every
//                ratio s / w a run forms, a weighted mean of the x / w, stays below 2^32: the
//                premise of ratio_moved's division-free branch (gp_device.hpp)
enum : uint32_t { VAL_OK = 0, VAL_X_SIGN = 1, VAL_W_SIGN = 2, VAL_W_RANGE = 3, VAL_X_TINY = 4, VAL_RATIO = 5 };

GP_HD bool val_plain(double v) {  // finite, sign bit clear
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b < 0x7FF0000000000000ull;
}

GP_HD uint32_t values_rule(double x, double w) {
    if (!val_plain(x)) return VAL_X_SIGN;
    if (!val_plain(w)) return VAL_W_SIGN;
    if (!(w >= 0x1p-32 && w <= 0x1p32)) return VAL_W_RANGE;
    if (!(x == 0.0 || x >= 0x1p-64)) return VAL_X_TINY;
    if (!(x * 0x1p-32 < w)) return VAL_RATIO;
    return VAL_OK;
}

// The verdict word the check kernel reduces with an atomic minimum: the lowest offending node id
// wins, and among one id's rules (it breaks the first it fails) the rule travels along.
constexpr unsigned long long VAL_NONE = ~0ull;
GP_HD unsigned long long val_pack(uint64_t id, uint32_t rule) { return (unsigned long long)(id << 3) | rule; }

// mu of a handle with values: finite, >= 0, < 2^32 (the range of the ratios it is compared with).
inline bool mean_ok(double mu) { return mu >= 0.0 && mu < 0x1p32; }  // (NaN fails both)

// The bounded staging of a caller's arrays: a pinned host buffer and a device buffer of the same
// size, grown on demand up to VAL_STAGE_BYTES and kept by the handle.  A chunk holds the entries
// interleaved as (x, w) pairs when weights are given -- the host has to copy the caller's pageable
// arrays into pinned memory anyway, and the kernels then move one 16-byte word per node -- or
// the values alone.
constexpr size_t VAL_STAGE_BYTES = 32u << 20;
struct ValStage {
    void* pin = nullptr;
    void* dev = nullptr;
    unsigned long long* bad = nullptr;  // device: the verdict word
    size_t bytes = 0;
};
void values_stage_free(ValStage& st);

// Where chunk entries [c0, c1) of a call go: called once per staged chunk, after the whole input
// has passed the check; `staged` is the device copy of the chunk (double2 if weighted, else double).
struct ValSink {
    virtual int write(const void* staged, bool weighted, int64_t c0, int64_t c1, hipStream_t st) = 0;
    virtual ~ValSink() = default;
};

// Streams x (and w, or null: all 1) of `count` nodes, ids from id0, through the staging buffer:
// first the check of every chunk (k_values_check), then, only if every entry is admissible, the
// sink's write of every chunk -- all or nothing.  An input of one chunk is uploaded once.
// GP_EINVAL: set_err names the lowest offending id and its rule.  sink may be null (check only).
int values_stream(ValStage& st, hipStream_t stream, int cus, const char* who, const double* x, const double* w,
                  int64_t count, int64_t id0, ValSink* sink);

// sw[i] = (x, w) of the staged chunk's entry i, i < n (k_values_write).
hipError_t launch_values_write(const void* staged, bool weighted, uint32_t n, double2* dst, int cus, hipStream_t st);
// The same entries as two arrays, x[i] and (weighted only) w[i]: the ensembles' layout (k_values_split).
hipError_t launch_values_split(const void* staged, bool weighted, uint32_t n, double* x, double* w, int cus,
                               hipStream_t st);

}  // namespace gp
