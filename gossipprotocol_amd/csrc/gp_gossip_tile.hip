// gp_gossip_tile.hip -- the gossip tile kernel for line / 3D / Imp3D (gfx950): one synchronous
// gossip round of SRS v1 in PULL form, a workgroup of 256 threads per tile of
// 1024 nodes, 4 per thread (the 1024-thread size class measured slower for gossip at every
// size and is not built, profiles/r04/tile_size_class.txt).  Per tile:
//
//   1. stage in LDS with LDS-DMA: the direction bytes of the tile and its +-g rows (y/z
//      neighbours, or +-1 for line), the x-1 and x+1 plane segments (3D), the tile's in-list
//      offsets (Imp3D); Imp3D in-edges decide "sent on its random edge" from the sender's
//      Philox draw and the ballot-packed bitmap, a byte per staged in-edge;
//   2. per node: count the lattice senders pointing here, the random-edge senders and the
//      injector; draw the next-round direction; node bytes leave through LDS as 32-bit
//      words, random-edge bits as one 64-bit ballot per wave.
#include "gp_tile.hpp"

namespace gp {

namespace {

constexpr int SRC_CAP = TILE * 3 / 2;       // gossip: staged in-list entries per tile (mean TILE)

struct TileLds {
    uint32_t rows[W_ROWS + DMA_SLACK];   // direction bytes of [j0 - H, j1 + H)
    uint32_t xm[W_PLANE + DMA_SLACK];    // direction bytes of [j0 - g^2, j1 - g^2)
    uint32_t xp[W_PLANE + DMA_SLACK];    // direction bytes of [j0 + g^2, j1 + g^2)
    uint32_t off[TILE + 1 + DMA_SLACK];  // in_off[j0 .. j1]
    uint32_t sent[SRC_CAP / 4];          // byte per staged in-edge: its sender used the random edge
    uint32_t out[TILE / 4];              // next-round node bytes, stored as words
    uint32_t red[2][TPB / 64];
};

}  // namespace

// Deliveries to j = lattice senders pointing here + Imp3D random-edge senders
// (bitmap) + the injector; all dropped if j was converged at round start.
template <int TOPO, bool REMOTE>
__global__ __launch_bounds__(TPB, GP_MINB) void k_gossip_tile(RoundArgs a, uint32_t r) {
    __shared__ TileLds L;
    Ctl* ctl = a.ctl;
    if (ld_agent(&ctl->done)) return;
    const long long inj = ld_agent(&ctl->inj_target);
    const Geom G = a.G;
    const uint32_t H = TOPO == LINE ? 1u : G.g;
    uint32_t alerts = 0;
    const int lane = threadIdx.x & 63;

    for (TileWalk tw(a); tw.t < tw.end; tw.t += tw.step) {
        uint32_t ti;
        if (!tw.tile(ti)) continue;
        // tiles sit on global multiples of TILE (4-aligned word I/O, 64-aligned
        // ballot words); the slab's first and last tile may be partial
        const uint32_t T = (a.lo / TILE + ti) * TILE;
        const uint32_t j0 = max(a.lo, T);
        const uint32_t j1 = min(a.lo + a.nloc, T + TILE);
        uint32_t e_lo = 0, e_hi = 0;
        if (TOPO == IMP3D) {
            e_lo = ld_const(a.in_off + j0);
            e_hi = ld_const(a.in_off + j1);
        }
        int32_t c0[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t j = T + k * TPB + threadIdx.x;
            c0[k] = (j >= j0 && j < j1) ? a.c[j] : (int32_t)GOSSIP_DONE;
        }
        const uint32_t b_rows = dma_stage_bytes(L.rows, a.nbc, (int64_t)j0 - H, (int64_t)j1 + H, a.ext_lo, a.ext_hi);
        uint32_t b_xm = 0, b_xp = 0;
        if (TOPO != LINE) {
            b_xm = dma_stage_bytes(L.xm, a.nbc, (int64_t)j0 - G.g2, (int64_t)j1 - G.g2, a.ext_lo, a.ext_hi);
            b_xp = dma_stage_bytes(L.xp, a.nbc, (int64_t)j0 + G.g2, (int64_t)j1 + G.g2, a.ext_lo, a.ext_hi);
        }
        const uint32_t cnt = e_hi - e_lo;
#ifdef GP_EXPERIMENTS
        // GP_STAGE_CAP lowers the limit, so tiles take the unstaged path (parity tests); never raises it
        const bool staged = cnt <= min((uint32_t)SRC_CAP, a.stage_cap);
#else
        const bool staged = cnt <= (uint32_t)SRC_CAP;
#endif
        int o_off = 0;  // L.off[jl + o_off] = in_off[T + jl]
        if (TOPO == IMP3D) {
            o_off = (int)dma_stage_words(L.off, a.in_off, j0, j1 + 1) - (int)(j0 - T);
            if (staged) {
                // all sender loads, then all bitmap loads, in flight together
                constexpr int FU = SRC_CAP / TPB;
                uint32_t isrc[FU];
#pragma unroll
                for (int m = 0; m < FU; ++m) {
                    const uint32_t q = threadIdx.x + m * TPB;
                    isrc[m] = q < cnt ? a.in_src[e_lo + q] : 0u;
                }
                // the senders' direction draws of round r as one Philox batch; the
                // bitmap (bit = active and the draw picks the random slot) is read
                // only where the draw picks it, ~1/7 of the in-edges, instead of a
                // random 128-byte line per in-edge
                uint32_t X[FU], Y[FU];
                philox2_batch<FU>(isrc, r, S_GOSSIP, a.k0, a.k1, X, Y);
                unsigned long long wv[FU];
#pragma unroll
                for (int m = 0; m < FU; ++m) {
                    const uint32_t q = threadIdx.x + m * TPB;
                    const uint32_t li = isrc[m] - a.lo;
                    const uint32_t di = popc6(present_mask<IMP3D>(isrc[m], G)) + 1u;
                    const bool pick = uniform_from(X[m], Y[m], di) == di - 1u;
                    wv[m] = q >= cnt ? 0ull
                            : (!REMOTE || li < a.nloc) ? (pick ? a.rbc[(isrc[m] >> 6) - (a.lo >> 6)] : 0ull)
                                          : (a.rtag[e_lo + q] == r ? ~0ull : 0ull);
                }
#pragma unroll
                for (int m = 0; m < FU; ++m) {
                    const uint32_t q = threadIdx.x + m * TPB;
                    if (q < cnt)
                        reinterpret_cast<uint8_t*>(L.sent)[q] = (uint8_t)((wv[m] >> (isrc[m] & 63)) & 1ull);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const uint32_t jl = k * TPB + threadIdx.x;
            const uint32_t j = T + jl;
            const bool valid = j >= j0 && j < j1;
            uint32_t dir = DIR_NONE;
            if (valid) {
                const uint32_t mask = present_mask<TOPO>(j, G);
                int32_t c1 = c0[k];
                if (c1 < (int32_t)GOSSIP_DONE) {
                    uint32_t inc = (long long)j == inj ? 1u : 0u;
                    if (TOPO == LINE) {
                        inc += (mask & 1u) && (lds_byte(L.rows, j - 1 - b_rows) & DIR_MASK) == 1u;
                        inc += (mask & 2u) && (lds_byte(L.rows, j + 1 - b_rows) & DIR_MASK) == 0u;
                    } else {
                        inc += (mask & 1u) && (lds_byte(L.xm, j - G.g2 - b_xm) & DIR_MASK) == 1u;
                        inc += (mask & 2u) && (lds_byte(L.xp, j + G.g2 - b_xp) & DIR_MASK) == 0u;
                        inc += (mask & 4u) && (lds_byte(L.rows, j + G.g - b_rows) & DIR_MASK) == 3u;
                        inc += (mask & 8u) && (lds_byte(L.rows, j - G.g - b_rows) & DIR_MASK) == 2u;
                        inc += (mask & 16u) && (lds_byte(L.rows, j + 1 - b_rows) & DIR_MASK) == 5u;
                        inc += (mask & 32u) && (lds_byte(L.rows, j - 1 - b_rows) & DIR_MASK) == 4u;
                    }
                    if (TOPO == IMP3D) {
                        const uint32_t e_b = L.off[jl + o_off], e_e = L.off[jl + 1 + o_off];
                        if (staged) {
                            for (uint32_t e = e_b; e < e_e; ++e) inc += lds_byte(L.sent, e - e_lo);
                        } else {
                            for (uint32_t e = e_b; e < e_e; ++e) {
                                const uint32_t i = a.in_src[e];
                                const uint32_t li = i - a.lo;
                                inc += (!REMOTE || li < a.nloc) ? (uint32_t)((a.rbc[(i >> 6) - (a.lo >> 6)] >> (i & 63)) & 1ull)
                                                   : (a.rtag[e] == r ? 1u : 0u);
                            }
                        }
                    }
                    if (inc) {
                        c1 += (int32_t)inc;
                        a.c[j] = c1;
                        alerts += c1 > 10;  // the receipt that finds rumours == 10 (Program.fs:92-94)
                    }
                }
                const bool active = ((j == a.seed_node) || c1 >= 1) && c1 <= 10;
                if (active) {
                    const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                    if (deg > 0) dir = slot_to_dir(mask, uniform(a.k0, a.k1, S_GOSSIP, j, r + 1, deg));
                }
                reinterpret_cast<uint8_t*>(L.out)[jl] = (uint8_t)dir;
            }
            if (TOPO == IMP3D) {
                const unsigned long long bits = __ballot(valid && dir == DIR_RANDOM);
                if (lane == 0) {  // the slab's first tile may start below lo: no word there
                    const int64_t wi = (int64_t)((T + k * TPB + (threadIdx.x & ~63u)) >> 6) - (int64_t)(a.lo >> 6);
                    if (wi >= 0) a.rbn[wi] = bits;
                }
            }
        }
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < (uint32_t)(TILE / 4); w += TPB) {
            const uint32_t jw = T + w * 4;
            if (jw >= j0 && jw + 4 <= j1) {
                reinterpret_cast<uint32_t*>(a.nbn + T)[w] = L.out[w];
            } else {
                for (uint32_t b = 0; b < 4; ++b)
                    if (jw + b >= j0 && jw + b < j1) a.nbn[jw + b] = reinterpret_cast<const uint8_t*>(L.out)[w * 4 + b];
            }
        }
        __syncthreads();
    }
    uint32_t x = alerts;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) L.red[0][threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        x = 0;
        for (int w = 0; w < TPB / 64; ++w) x += L.red[0][w];
        if (x) atomicAdd(&ctl->round_alerts, (unsigned long long)x);
    }
}

// Imp3D slabs of a multi-rank run (S.rtag) read the tagged slots of remote senders.
hipError_t launch_gossip_tile(const DevState& S, const RoundArgs& a, uint32_t round, int grid, hipStream_t st) {
    const dim3 g(grid), b(TPB);
    switch (S.topo) {
        case LINE: hipLaunchKernelGGL((k_gossip_tile<LINE, false>), g, b, 0, st, a, round); break;
        case GRID3D: hipLaunchKernelGGL((k_gossip_tile<GRID3D, false>), g, b, 0, st, a, round); break;
        default:
            if (S.rtag) hipLaunchKernelGGL((k_gossip_tile<IMP3D, true>), g, b, 0, st, a, round);
            else hipLaunchKernelGGL((k_gossip_tile<IMP3D, false>), g, b, 0, st, a, round);
            break;
    }
    return hipGetLastError();
}

}  // namespace gp
