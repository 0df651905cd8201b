// gp_tile_host.hip -- the host side of the tiled round kernels, independent of their size
// class: the kernels' arguments, the slab's tile and region arithmetic, walk 3's tile list,
// the three set-up kernels that prepare what the tile kernels read, and the entry point
// that picks the kernel of a round (gp_ps_tile.hip, gp_ps_tile_wide.hip, gp_gossip_tile.hip).
#include <algorithm>
#include <vector>

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

// Tiles covering the ids [lo, lo + nloc) (tiles sit on global multiples of TILE).
static uint32_t tiles_for(uint32_t lo, uint32_t nloc) {
    return (uint32_t)(((uint64_t)lo + nloc + TILE - 1) / TILE - lo / TILE);
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
    a.rmsg = S.rmsg;
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
#endif
    a.wx = S.tile_wx;
    a.fuse = S.fuse_finalize;
    a.wt = S.wtiles;
    for (int c = 0; c <= 8; ++c) a.wo[c] = S.woff[0][c];
    a.tq = S.tq + (round & 1) * 8 * TQ_STRIDE;
    a.tq_next = S.tq + ((round + 1) & 1) * 8 * TQ_STRIDE;
    return a;
}

// First plane (relative to the slab's) of region h of NR equal regions over nx planes.  (A last
// region half the size of the others measured within noise, profiles/r05/rejected/rlast.txt.)
uint32_t region_plane(uint32_t nx, int NR, int h) {
    if (h >= NR) return nx;
    return (uint32_t)((uint64_t)nx * h / NR);
}

// Region h of NR of a plane-aligned slab: planes [x0 + region_plane(h), x0 + region_plane(h + 1)),
// whose tiles (relative to lo / TILE) are [rb[h], rb[h + 1]) -- a tile belongs to the plane it
// starts in (the slab's first tile to the first plane).  False if the slab is not plane-aligned.
bool region_tiles(uint32_t lo, uint32_t nloc, uint64_t g2, int NR, uint32_t* rb) {
    if (!g2 || nloc % g2 || lo % g2 || NR < 1) return false;
    const uint32_t tb = lo / TILE;
    const uint32_t tend = (uint32_t)(((uint64_t)lo + nloc + TILE - 1) / TILE);
    const uint32_t x0 = (uint32_t)(lo / g2), nx = (uint32_t)(nloc / g2);
    for (int h = 0; h <= NR; ++h) {
        const uint64_t x = x0 + region_plane(nx, NR, h);
        rb[h] = (x <= x0 ? tb : (uint32_t)std::min<uint64_t>((x * g2 + TILE - 1) / TILE, tend)) - tb;
    }
    return true;
}

// Walk 3's visiting order (host, at create): walk 2's items (TileWalk, gp_tile.hpp) for each
// of the 8 XCDs, empty items dropped -- every tile of the slab exactly once.
// list: tiles relative to lo / TILE; woff[0][c]..woff[0][c + 1]: XCD c's items.
// NR > 1 (launch_round_regions): the planes of region h (region_tiles) dealt to the
// 8 XCDs in the same way, XCD c's items at woff[h][c]..woff[h][c + 1].
bool build_walk_list(const DevState& S, int NR, std::vector<uint32_t>& list, uint32_t woff[][9]) {
    const uint64_t g2 = S.G.g2;
    if (!g2 || S.nloc % g2 || S.lo % g2 || NR < 1 || NR > RREG_MAX) return false;
    const uint32_t tb = S.lo / TILE;
    const uint32_t tend = (uint32_t)(((uint64_t)S.lo + S.nloc + TILE - 1) / TILE);
    const uint32_t x0 = (uint32_t)(S.lo / g2), nx = (uint32_t)(S.nloc / g2);
    const uint32_t kp = (uint32_t)((g2 + TILE - 1) / TILE + 1);
    auto first = [&](uint32_t x) -> uint32_t {
        return x <= x0 ? tb : (uint32_t)std::min<uint64_t>((x * g2 + TILE - 1) / TILE, tend);
    };
    list.clear();
    for (int h = 0; h < NR; ++h) {
        const uint32_t r0 = x0 + region_plane(nx, NR, h);
        const uint32_t nr = x0 + region_plane(nx, NR, h + 1) - r0;
        for (uint32_t c = 0; c < 8; ++c) {
            woff[h][c] = (uint32_t)list.size();
            const uint32_t xa = r0 + (uint32_t)((uint64_t)nr * c / 8);
            const uint32_t nxa = r0 + (uint32_t)((uint64_t)nr * (c + 1) / 8) - xa;
            uint32_t nwin = S.tile_wx ? (nxa + S.tile_wx - 1) / S.tile_wx : 1u;
            if (nwin == 0) nwin = 1;
            for (uint32_t v = 0; v < nwin && nxa; ++v) {
                const uint32_t xs = (uint32_t)((uint64_t)nxa * v / nwin), xe = (uint32_t)((uint64_t)nxa * (v + 1) / nwin);
                for (uint32_t k = 0; k < kp; ++k)
                    for (uint32_t x = xa + xs; x < xa + xe; ++x) {
                        const uint32_t ti = first(x) + k;
                        if (ti < first(x + 1)) list.push_back(ti - tb);
                    }
            }
        }
        woff[h][8] = (uint32_t)list.size();
    }
    return list.size() == (size_t)(tend - tb);
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
