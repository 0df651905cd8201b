// gp_tile_host.hip -- the host side of the tiled round kernels, independent of their size
// class: the kernels' arguments, the three set-up kernels that prepare what the tile kernels
// read, and the entry point that picks the kernel of a round (gp_ps_tile.hip,
// gp_ps_tile_wide.hip, gp_gossip_tile.hip).  The slab's tile and region arithmetic and walk 3's
// tile list: gp_plan.hpp.
#include <algorithm>

#include "gp_internal.hpp"

namespace gp {

constexpr int SETUP_TPB = 256;  // threads per block of the set-up kernels

// Random-edge bits of round 0 (only the seed can be sending).
// nb indexed by global id; bit (j - lo) of rb for the slab's nodes.
// Word w holds ids [64 (w + lo/64), +64) (global 64-alignment, as the round kernels).
__global__ __launch_bounds__(SETUP_TPB) void k_rbits_init(const uint8_t* nb, uint64_t* rb, uint32_t lo, uint32_t nloc,
                                                          uint32_t nwords) {
    const uint32_t j00 = lo & ~63u;
    for (uint32_t jb = blockIdx.x * SETUP_TPB; jb < nwords * 64u; jb += gridDim.x * SETUP_TPB) {
        const uint32_t j = j00 + jb + threadIdx.x;
        const bool bit = j >= lo && j - lo < nloc && (nb[j] & DIR_MASK) == DIR_RANDOM;
        const unsigned long long bits = __ballot(bit);
        if ((threadIdx.x & 63) == 0) rb[(j >> 6) - (lo >> 6)] = bits;
    }
}

// 64-bit words the ballot stores of one round touch (whole tiles) plus slack.
uint32_t rbits_words_for(uint32_t lo, uint32_t nloc) { return tiles_for(lo, nloc) * (TILE / 64) + 16u; }

RoundArgs make_round_args(const DevState& S, uint32_t round) {
    const int cur = round & 1;
    RoundArgs a;
    // node arrays indexed by global id: pointers offset by the slab's first id
    a.swc = S.sw[cur] ? S.sw[cur] - S.base : nullptr;
    a.swn = S.sw[cur ^ 1] ? S.sw[cur ^ 1] - S.base : nullptr;
    a.nbc = S.nb[cur] ? S.nb[cur] - S.base : nullptr;
    a.nbn = S.nb[cur ^ 1] ? S.nb[cur ^ 1] - S.base : nullptr;
    a.rbc = S.rbits[cur];
    a.rbn = S.rbits[cur ^ 1];
    a.in_off = S.in_off ? S.in_off - S.lo : nullptr;
    a.in_src = S.in_src;
    a.in_srcd = S.in_srcd;
    a.ind4 = S.ind4 ? S.ind4 - (S.lo / TILE) * (TILE / 2) : nullptr;
    a.rtag = S.rtag;
    a.rk = S.rk;
    a.xhdr = S.xhdr[round & 1];
    a.xvals = S.xvals[round & 1];
    a.xnv = S.xnv;
    a.c = S.c ? S.c - S.lo : nullptr;
    a.lo = S.lo;
    a.nloc = S.nloc;
    a.ext_lo = S.ext_lo;
    a.ext_hi = S.ext_hi;
    a.ctl = S.ctl;
    a.G = S.G;
    a.k0 = S.k0;
    a.k1 = S.k1;
    a.seed_node = S.seed_node;
    a.ntiles = tiles_for(S.lo, S.nloc);
    a.walk = S.tile_walk;
    a.stage_cap = S.tile_stage_cap;
#ifdef GP_EXPERIMENTS
    a.no_full = S.tile_no_full;
    a.slot_shadow = S.tile_slot_shadow;
#endif
    a.wx = S.tile_wx;
    a.fuse = S.fuse_finalize;
    a.wt = S.wtiles;
    for (int c = 0; c <= 8; ++c) a.wo[c] = S.woff[0][c];
    a.tq = S.tq + (round & 1) * 8 * TQ_STRIDE;
    a.tq_next = S.tq + ((round + 1) & 1) * 8 * TQ_STRIDE;
    return a;
}

// The tile kernel of round `round`: push-sum in the slab's size class (DevState::tile_wide,
// set by choose_kernel for line / 3D push-sum only), gossip in the 256-thread class.
hipError_t launch_round_tile(const DevState& S, uint32_t round, int grid, hipStream_t st) {
    if (S.rregions > 1) return hipErrorInvalidValue;  // launch_round_tile_region per region
    const RoundArgs a = make_round_args(S, round);
    if (S.alg == PUSHSUM)
        return S.tile_wide ? wide::launch_ps_tile(S, a, round, grid, st) : launch_ps_tile(S, a, round, grid, st);
    if (S.tile_wide) return hipErrorInvalidValue;  // not built
    return launch_gossip_tile(S, a, round, grid, st);
}

// Imp3D push-sum senders with their degree packed in the top two bits
// (deg - 4 in [0, 3]; every node has 3..6 lattice slots + the random one when
// g >= 2), so the tile kernel's in-edge pass needs no division to find it.
// Valid when every id fits 30 bits (P <= 2^30).
__global__ __launch_bounds__(SETUP_TPB) void k_pack_src_deg(const uint32_t* src, uint32_t* out, uint32_t n, Geom G) {
    for (uint32_t e = blockIdx.x * SETUP_TPB + threadIdx.x; e < n; e += gridDim.x * SETUP_TPB) {
        const uint32_t i = src[e];
        const uint32_t deg = popc6(present_mask<IMP3D>(i, G)) + 1u;
        out[e] = i | ((deg - 4u) << 30);
    }
}

hipError_t launch_pack_src_deg(const uint32_t* src, uint32_t* out, uint32_t n, const Geom& G, int grid,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_pack_src_deg, dim3(grid), dim3(SETUP_TPB), 0, st, src, out, n, G);
    return hipGetLastError();
}

// Nibble in-degrees of the slab's tiles (DevState::ind4) from in_off.
// wide_at: in-degrees from this value on are stored as 15, the "read in_off"
// mark (15 in the product; tests lower it to exercise that path).
__global__ __launch_bounds__(SETUP_TPB) void k_pack_ind4(const uint32_t* __restrict__ in_off, uint32_t lo, uint32_t nloc,
                                                         uint32_t j00, uint8_t* __restrict__ out, uint32_t nbytes,
                                                         uint32_t wide_at) {
    for (uint32_t b = blockIdx.x * SETUP_TPB + threadIdx.x; b < nbytes; b += gridDim.x * SETUP_TPB) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t j = j00 + 2 * b + h;
            if (j - lo < nloc) {
                const uint32_t d = in_off[j + 1] - in_off[j];
                v |= (d >= wide_at ? 15u : d) << (4 * h);
            }
        }
        out[b] = (uint8_t)v;
    }
}

uint32_t ind4_bytes_for(uint32_t lo, uint32_t nloc) { return tiles_for(lo, nloc) * (TILE / 2) + 16u; }

hipError_t launch_pack_ind4(const DevState& S, uint32_t wide_at, int grid, hipStream_t st) {
    const uint32_t nbytes = tiles_for(S.lo, S.nloc) * (TILE / 2);
    hipLaunchKernelGGL(k_pack_ind4, dim3(grid), dim3(SETUP_TPB), 0, st, S.in_off - S.lo, S.lo, S.nloc,
                       (S.lo / TILE) * TILE, S.ind4, nbytes, std::min(wide_at, 15u));
    return hipGetLastError();
}

hipError_t launch_rbits_init(const DevState& S, int grid, hipStream_t st) {
    hipLaunchKernelGGL(k_rbits_init, dim3(grid), dim3(SETUP_TPB), 0, st, S.nb[0] - S.base, S.rbits[0], S.lo, S.nloc,
                       S.rbits_words);
    return hipGetLastError();
}

}  // namespace gp
