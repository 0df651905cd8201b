// gp_tile.hpp -- what the two tile kernels (gp_ps_tile.hip, gp_gossip_tile.hip) share: the
// size class, the LDS-DMA staging helpers and the tile walk.  Device code only, and with
// internal linkage: a unit is compiled for one size class, and TPB differs between them.
//
// A tile is TILE = 1024 consecutive nodes, lane-contiguous, on a global multiple of TILE.
// Tiles are walked XCD-contiguously (blocks b and b+8 share an XCD on MI355X), so the +-g
// rows a tile gathers from were just read by its XCD.
#pragma once

#include "gp_internal.hpp"

// Size class: 256 threads x 4 nodes unless the including unit (gp_ps_tile_wide.hip) says otherwise.
#ifndef GP_TPB
#define GP_TPB 256
#define GP_NPT 4
// __launch_bounds__ minimum waves per SIMD (= resident 256-thread blocks per CU): the LDS
// tile allows 5, so keep VGPRs <= 96 to not lose the fifth
#define GP_MINB 5
#endif

namespace gp {
namespace {

constexpr int TPB = GP_TPB;                // 256 (wide size class: 1024)
constexpr int NPT = GP_NPT;                // nodes per thread per tile
static_assert(TPB * NPT == TILE, "a block covers one tile");
constexpr int HMAX = 1625;                 // largest lattice edge with g^3 < 2^32
constexpr int W_ROWS = (TILE + 2 * HMAX) / 4 + 4;
constexpr int W_PLANE = TILE / 4 + 4;

// Staged ranges are moved by 16-byte LDS-DMA (global_load_lds_dwordx4) from a
// 16-byte aligned start: every array has 8 words of slack for the alignment.
constexpr int DMA_SLACK = 8;

// set bits of m below this lane
__device__ __forceinline__ uint32_t mbcnt64(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t lds_byte(const uint32_t* w, uint32_t idx) {
    return reinterpret_cast<const uint8_t*>(w)[idx];
}

typedef __attribute__((address_space(1))) void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

// Copy nbytes (rounded up to 16) from a 16-byte aligned global address into LDS
// with LDS-DMA: no VGPR round trip and no wait inside the loop, so every
// staging copy of a tile is in flight at once (retired by the next
// __syncthreads, which waits vmcnt(0)).  One wave-instruction moves 1 KiB.
template <int AUX = 0>
__device__ __forceinline__ void dma_copy(void* lds, const char* g16, uint32_t nbytes) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t c = (threadIdx.x >> 6) * 1024u; c < nbytes; c += TPB * 16u) {
        const uint32_t o = c + lane * 16u;
        if (o < nbytes)
            __builtin_amdgcn_global_load_lds((gvoid_t*)(g16 + o), (lvoid_t*)(reinterpret_cast<char*>(lds) + c), 16, 0,
                                             AUX);
    }
}
// cache-policy bits of a single-use (streamed once per round) staging copy: nt
constexpr int DMA_ONCE = 2;

// Node bytes nb[lo, hi) clamped to [ext_lo,
// ext_hi); returns the node id of LDS byte 0 (up to 15 bytes below lo).  Reads
// at most 15 bytes past hi (node arrays are padded).
__device__ __forceinline__ uint32_t dma_stage_bytes(uint32_t* lds, const uint8_t* nb, int64_t lo, int64_t hi,
                                                    uint32_t ext_lo, uint32_t ext_hi) {
    if (lo < (int64_t)ext_lo) lo = ext_lo;
    if (hi > (int64_t)ext_hi) hi = ext_hi;
    const char* p = reinterpret_cast<const char*>(nb + lo);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    if (hi > lo) dma_copy(lds, p - mis, (uint32_t)(hi - lo) + mis);
    return (uint32_t)lo - mis;
}

// LDS-DMA of the words w[lo, hi); returns how many words below lo were staged
// (w[lo + i] lands in lds[i + returned]).  Reads at most 3 words past hi
// (the in-list arrays are padded).
__device__ __forceinline__ uint32_t dma_stage_words(uint32_t* lds, const uint32_t* w, uint32_t lo, uint32_t hi) {
    const char* p = reinterpret_cast<const char*>(w + lo);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    if (hi > lo) dma_copy<DMA_ONCE>(lds, p - mis, (hi - lo) * 4u + mis);
    return mis >> 2;
}

template <typename T>
__device__ __forceinline__ T ld_agent(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tile walks (speed only -- any placement is correct; every tile of the slab
// is visited exactly once).  Blocks with equal blockIdx % 8 share an XCD.
//   walk 0: XCD-contiguous eighths of the tile range;
//   walk 1: one global sweep (tile t -> block t % grid);
//   walk 2 (3D / Imp3D): x-window walk.  Each XCD owns an eighth of the slab's
//     x-planes, cut into windows of ~wx planes; inside a window the walk is
//     x-fastest: item u -> plane x = x_w + u % nx_w, k-th tile starting in that
//     plane.  The blocks resident on an XCD at one time then work on the same
//     in-plane position of ~wx consecutive planes (x+-1 neighbours) and of a few
//     consecutive k (y+-1 rows), so lattice gathers and the x+-1 byte planes hit
//     the XCD's L2 instead of HBM.
//   walk 3 (k_ps_tile): walk 2's items without the empty ones, listed per XCD
//     at create time (DevState::wtiles, build_walk_list, gp_plan.hpp) and
//     claimed in order from a per-XCD counter (one returning atomic per tile,
//     issued a tile ahead) on a grid of exactly the resident blocks.  The tiles
//     an XCD has in flight are then always ~160 consecutive items (20 in-plane
//     positions of 8 planes), and the tiles just finished are their y-1 / x+-1
//     neighbours; walk 2's static stride keeps items 2048 apart in flight, and
//     its item -> tile arithmetic (64-bit divisions) costs ~100 scalar
//     instructions per tile and wave.
struct TileWalk {
    uint32_t t, end, step;
    // walk 2
    uint32_t mode, tb, tend, g2, x0, xa, nxa, kp, nwin;
    // walk 3: this XCD's item counter and tile list
    uint32_t* qc;
    const uint32_t* wl;
    __device__ TileWalk(const RoundArgs& a) {
        const uint32_t G = gridDim.x;
        mode = a.walk;
        qc = nullptr;
        wl = nullptr;
        if (mode == 3 && (a.wt == nullptr || G < 8 || (G & 7) != 0)) mode = 1;
        if (mode == 3) {
            const uint32_t c = blockIdx.x & 7;
            qc = a.tq + c * TQ_STRIDE;
            wl = a.wt + a.wo[c];
            t = 0;
            end = a.wo[c + 1] - a.wo[c];
            step = 1;
        } else if (mode == 2 && a.G.g2 && G >= 8 && (G & 7) == 0) {
            const uint32_t c = blockIdx.x & 7;
            g2 = a.G.g2;
            tb = a.lo / TILE;
            tend = (uint32_t)(((uint64_t)a.lo + a.nloc + TILE - 1) / TILE);
            x0 = a.lo / g2;
            const uint32_t X0 = x0, nx = a.nloc / g2;
            xa = X0 + (uint32_t)((uint64_t)nx * c / 8);
            nxa = X0 + (uint32_t)((uint64_t)nx * (c + 1) / 8) - xa;
            kp = (g2 + TILE - 1) / TILE + 1;
            nwin = a.wx ? (nxa + a.wx - 1) / a.wx : 1u;
            if (nwin == 0) nwin = 1;
            t = blockIdx.x >> 3;
            end = nxa * kp;
            step = G >> 3;
        } else if (mode == 0 && G >= 8 && (G & 7) == 0) {
            mode = 0;
            const uint32_t x = blockIdx.x & 7, k = blockIdx.x >> 3;
            const uint32_t lo = (uint32_t)((uint64_t)a.ntiles * x / 8);
            end = (uint32_t)((uint64_t)a.ntiles * (x + 1) / 8);
            t = lo + k;
            step = G >> 3;
        } else {
            mode = 1;
            t = blockIdx.x;
            end = a.ntiles;
            step = G;
        }
    }
    // first global tile index of plane x (the slab's first tile may start below lo)
    __device__ __forceinline__ uint32_t first(uint32_t x) const {
        return x <= x0 ? tb : min((uint32_t)(((uint64_t)x * g2 + TILE - 1) / TILE), tend);
    }
    // tile (relative to lo / TILE) of walk item t; false: empty item (block-uniform)
    __device__ __forceinline__ bool tile(uint32_t& rel) const {
        if (mode == 3) {
            rel = ld_const(wl + t);
            return true;
        }
        if (mode != 2) {
            rel = t;
            return true;
        }
        // (the divisors opaque: their reciprocals are then computed here, per item, instead of being
        // hoisted out of the caller's tile loop into VGPRs that stay live across its node phase)
        uint32_t kp = this->kp, nwin = this->nwin, nxa = this->nxa;
        asm volatile("" : "+s"(kp), "+s"(nwin), "+s"(nxa));
        const uint32_t pl = t / kp;  // planes of this XCD before the item's window start (approx.)
        uint32_t v = (uint32_t)((uint64_t)pl * nwin / nxa);
        if (v >= nwin) v = nwin - 1;
        uint32_t xs = (uint32_t)((uint64_t)nxa * v / nwin);
        while (v > 0 && xs * kp > t) {
            --v;
            xs = (uint32_t)((uint64_t)nxa * v / nwin);
        }
        for (;;) {
            const uint32_t xe = (uint32_t)((uint64_t)nxa * (v + 1) / nwin);
            if (v + 1 >= nwin || xe * kp > t) break;
            ++v;
            xs = xe;
        }
        const uint32_t xe = (uint32_t)((uint64_t)nxa * (v + 1) / nwin);
        const uint32_t u = t - xs * kp, nxv = xe - xs;
        const uint32_t x = xa + xs + u % nxv, k = u / nxv;
        const uint32_t ti = first(x) + k;
        if (ti >= first(x + 1)) return false;
        rel = ti - tb;
        return true;
    }
};

__device__ __forceinline__ double2 ld_sw(const double2* p) { return *p; }

// v of another lane of the wave by DPP (CTRL 0x130 wave_shl:1 = lane + 1's,
// 0x138 wave_shr:1 = lane - 1's; the lane at the wave's end gets 0 -- bound_ctrl,
// so no zeroed destination register is needed)
template <int CTRL>
__device__ __forceinline__ double2 dpp_double2(double2 v) {
    auto mv = [](double d) {
        const uint64_t u = __builtin_bit_cast(uint64_t, d);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
        return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    };
    return make_double2(mv(v.x), mv(v.y));
}

// Next-round state is written once and not read again this round: non-temporal
// stores keep it from displacing the current round's (s, w) in the XCD's L2,
// where the neighbouring tiles' lattice gathers look for it.
__device__ __forceinline__ void st_stream(double2* p, double2 v) {
    __builtin_nontemporal_store(v.x, &p->x);
    __builtin_nontemporal_store(v.y, &p->y);
}
__device__ __forceinline__ void st_stream(uint32_t* p, uint32_t v) { __builtin_nontemporal_store(v, p); }

}  // namespace
}  // namespace gp
