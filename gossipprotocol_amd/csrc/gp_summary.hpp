// gp_summary.hpp -- the arithmetic of state summaries (include/gossip_hip.h, gp_summary)
// that host and device share: error-free sums into a double-double, and the join of two
// summaries of adjacent id ranges.  Host-only C++ (no HIP type or call), so a stand-alone
// CPU program can include it; under hipcc the same functions also compile for the device,
// so the kernel (gp_summary.hip) and gp_summary_merge round identically.  DESIGN.md §10.
//
// None of this may be contracted or reassociated: build with -ffp-contract=off (the
// library's Makefile does) and without -ffast-math.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/gossip_hip.h"

#if defined(__HIPCC__)
#define GP_SUM_HD __host__ __device__
#else
#define GP_SUM_HD
#endif

namespace gp {

// s + e == a + b exactly, s = fl(a + b) (Knuth's TwoSum; no condition on the operands).
GP_SUM_HD inline void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// The same for |a| >= |b| (Dekker's FastTwoSum).
GP_SUM_HD inline void fast_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    e = b - (s - a);
}

// (hi, lo) += x.  Relative error at most 2 * 2^-106 (Joldes, Muller, Popescu 2017, DWPlusFP).
GP_SUM_HD inline void dd_add_d(double& hi, double& lo, double x) {
    double s, e;
    two_sum(hi, x, s, e);
    e += lo;
    fast_two_sum(s, e, hi, lo);
}

// (hi, lo) += (bh, bl).  Relative error at most 3 * 2^-106 + O(2^-159) (ibid., AccurateDWPlusDW).
GP_SUM_HD inline void dd_add(double& hi, double& lo, double bh, double bl) {
    double sh, sl, th, tl, vh, vl;
    two_sum(hi, bh, sh, sl);
    two_sum(lo, bl, th, tl);
    const double c = sl + th;
    fast_two_sum(sh, c, vh, vl);
    const double w = tl + vl;
    fast_two_sum(vh, w, hi, lo);
}

// Does (value b, id nb) beat (value a, id na) as the largest error?  Larger value, then lower id.
GP_SUM_HD inline bool err_beats(double b, uint64_t nb, double a, uint64_t na) {
    return b > a || (b == a && nb < na);
}

// The join behind gp_summary_merge: 0, or GP_EINVAL when a and b are not adjacent or disagree
// in population, rounds, algorithm or tol.  out may alias a or b.
inline int summary_merge(const gp_summary* a, const gp_summary* b, gp_summary* out) {
    if (!a || !b || !out) return GP_EINVAL;
    if (a->count < 0 || b->count < 0 || a->first + a->count != b->first) return GP_EINVAL;
    if (a->population != b->population || a->rounds != b->rounds || a->algorithm != b->algorithm ||
        memcmp(&a->tol, &b->tol, sizeof(double)) != 0)
        return GP_EINVAL;
    if (a->count == 0 || b->count == 0) {  // an empty range has no minimum: the other side, at a's start
        gp_summary r = a->count == 0 ? *b : *a;
        r.first = a->first;
        *out = r;
        return GP_OK;
    }
    gp_summary r = *a;
    r.count = a->count + b->count;
    r.active += b->active;
    r.converged += b->converged;
    for (int k = 0; k < 12; ++k) r.c_hist[k] += b->c_hist[k];
    if (b->c_max > r.c_max) r.c_max = b->c_max;
    for (int k = 0; k < 4; ++k) r.cnt_hist[k] += b->cnt_hist[k];
    if (b->est_min < r.est_min) r.est_min = b->est_min;
    if (b->est_max > r.est_max) r.est_max = b->est_max;
    if (b->w_min < r.w_min) r.w_min = b->w_min;
    if (b->w_max > r.w_max) r.w_max = b->w_max;
    if (err_beats(b->err_max, (uint64_t)b->err_max_node, r.err_max, (uint64_t)r.err_max_node)) {
        r.err_max = b->err_max;
        r.err_max_node = b->err_max_node;
    }
    r.within_tol += b->within_tol;
    dd_add(r.sum_s[0], r.sum_s[1], b->sum_s[0], b->sum_s[1]);
    dd_add(r.sum_w[0], r.sum_w[1], b->sum_w[0], b->sum_w[1]);
    dd_add(r.sum_sqerr[0], r.sum_sqerr[1], b->sum_sqerr[0], b->sum_sqerr[1]);
    *out = r;
    return GP_OK;
}

}  // namespace gp
