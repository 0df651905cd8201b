// gp_summary_dev.hpp -- launch interface of the state-summary kernels (gp_summary.hip) for the
// host units: gp_summary_take (gp_summary.hip) and gp_ensemble_summary (gp_ensemble_api.hip).
// DESIGN.md §10.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gp_summary.hpp"

namespace gp {

constexpr int SUM_THREADS = 256;       // four waves per workgroup
constexpr int SUM_BLOCKS_PER_CU = 8;   // persistent grid: at most this many workgroups per CU

// What a lane, a wave, a workgroup and the whole grid accumulate: the partial record the
// workgroups leave in HBM and the result the fold kernel writes.  hist: gossip c = 0..10 and
// >= 11; push-sum stability count 0..3 in [0..3].
struct SumAcc {
    unsigned long long active, conv, within, err_node;
    unsigned long long hist[12];
    double est_min, est_max, w_min, w_max, err_max;
    double ss[2], sw[2], sq[2];  // double-double sums of s, w and e * e
    int32_t c_max, pad;
};

// One slab's state as gp_read_state addresses it.
struct SummaryArgs {
    const double2* sw;   // push-sum: (s, w) of the round's buffer, from the array's first id
    const uint8_t* nb;   // push-sum: node bytes, same indexing
    const int32_t* c;    // gossip: rumour counters, from the slab's first id
    uint32_t a0;         // array index of the first owned node (push-sum: lo - base; gossip: 0)
    uint32_t n;          // owned nodes
    uint32_t id0;        // node id of array index 0
    uint32_t seed_node;
    double mu, tol;      // the handle's mean ((P - 1) / 2 unless values were set); tolerance on |e|
    SumAcc* part;        // one record per workgroup
};

// Workgroups summary_launch uses for n nodes on a device of `cus` compute units.
uint32_t summary_blocks(int alg, uint32_t a0, uint32_t n, int cus);
// One pass over the slab: workgroup b leaves its partial record in a.part[b].
hipError_t summary_launch(int alg, const SummaryArgs& a, uint32_t blocks, hipStream_t st);
// out[0] = the nparts records of part joined in ascending order.
hipError_t summary_fold(int alg, const SumAcc* part, uint32_t nparts, SumAcc* out, hipStream_t st);

// Ensemble members (gp_ensemble.hpp: c, or s / w / fl, nseeds x P): one workgroup per member,
// out[m] = member m's record.  seed_node: per member (gossip).
struct SumEnsArgs {
    const int32_t* c;
    const double* s;
    const double* w;
    const uint8_t* fl;   // bit0 active, bit1 converged, bits2-3 count
    const gp_member* rec;
    uint32_t P;
    double mu, tol;
    SumAcc* out;
};
hipError_t summary_ens_launch(int alg, const SumEnsArgs& a, uint32_t nseeds, hipStream_t st);

// The C-ABI record of an accumulated range.
void summary_from_acc(const SumAcc& a, int alg, int64_t first, int64_t count, int64_t P, int64_t rounds, double tol,
                      gp_summary* out);

}  // namespace gp
