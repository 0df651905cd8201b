// gp_ps_tile.hip -- the push-sum tile kernel for line / 3D / Imp3D (gfx950).
//
// One synchronous round of SRS v1 in PULL form: every node
// reads who sent to it and folds the messages in canonical order, then draws
// its own direction for the next round.  Layout per workgroup (256 threads,
// TILE = 1024 consecutive nodes, 4 per thread, lane-contiguous; gp_tile.hpp):
//
//   1. stage in LDS by LDS-DMA: the direction bytes of the tile and its +-g rows
//      (y/z neighbours, or +-1 for line), the x-1 and x+1 plane segments (3D),
//      the tile's nibble in-degrees (Imp3D: DevState::ind4; in_off itself is read
//      only for the tile's range and inside `wide` tiles);
//   2. per node: lattice senders are read from LDS and only the (s, w) of the
//      neighbours that actually sent here are gathered (independent loads, no
//      dependent byte loads); Imp3D in-edges decide "sent on its random edge"
//      from the sender's Philox draw (every node active) or from a ballot-packed
//      bitmap (activation phase), then gather;
//   3. fold in canonical order (own half, lattice slots, random edges by
//      ascending sender), ratio test (the next-round Philox draw runs under the slot's loads); node bytes leave
//      through LDS as 32-bit words, random-edge bits as one 64-bit ballot per
//      wave.
// Built with -ffp-contract=off: the fold must round exactly like the oracle.
#include <type_traits>

#include "gp_tile.hpp"

namespace gp {
#ifdef GP_TILE_WIDE
// gp_ps_tile_wide.hip: this file again with 1024-thread tiles of one node per thread (the
// small-population size class), line and 3D only, its host entry points in gp::wide
namespace wide {
#endif

// Measured choices of the push-sum tile kernel (the rejected alternatives and their
// records are in DESIGN.md §5.1 and profiles/; git history has their code):
//  * wave priority: raised (s_setprio PRIO) while a wave issues its memory operations --
//    the in-edge pass's gathers, the staging copies, each node slot's loads -- and dropped
//    for the fold and the direction draws, so waves about to issue loads win the SIMD over
//    waves with ALU work and more loads are in flight (P = 1e9, same box, alternated:
//    13.19-13.68 -> 12.93-13.15 ms/round, profiles/r04/setprio_ab.txt);
//  * walk 3 work stealing: a block whose XCD's queue is empty takes items from the other
//    XCDs' queues (12.85-12.87 -> 12.75-12.81 ms/round; W = 8 slab 1.714 -> 1.699 ms,
//    profiles/r04/walk_steal.txt);
//  * the j +- 1 messages from the neighbour lanes' registers by DPP, one node slot's loads
//    in flight at a time (two spilled), non-temporal staging loads and state stores;
//  * between a node slot's load issue and its wait: the node's next-round direction draw and
//    the next slot's sender tests, neither of which needs what the loads return (P = 1e9,
//    same box, alternated: 11.74-11.99 -> 11.49-11.64 ms/round, profiles/r08/slot_shadow/).
constexpr int PRIO = 1;  // the raised wave priority

namespace {

// k_ps_tile: the tile decides its in-edges itself.  The used in-edges' (s, w) are gathered by LDS-DMA straight into per-edge
// slots (edge q's message at slot q -- lane-linear, so one global_load_lds per
// edge batch, no registers, no compaction).  A tile with more than SLOTS
// in-edges takes the unstaged path, so the node fold reads LDS only (no global
// fallback inside its loop, whose join would cost a vmcnt(0) wait per message).
//
// One rank (SNDPF): the next tile's in-edge senders are LDS-DMA'd during this tile's node phase,
// so a tile's in-edge pass starts from LDS (C5, same box, alternated: 12.92-13.07 -> 12.78-12.86
// ms on one box, 12.78-12.82 -> 12.74-12.77 on another, profiles/r05/sndpf/).  Their buffer takes
// LDS from the slots: 1152 slots (a tile's in-degree is ~Poisson(1024); 4 sigma, ~4e-5 of tiles
// -- about 40 per C5 round -- take the unstaged path).  The REMOTE kernel (several ranks) has no
// such buffer (measured within noise there, profiles/r05/sndpf/w8.txt) and keeps 1216 slots (6
// sigma, ~2.5e-9 of tiles): both fill the LDS of 5 blocks per CU.
template <bool REMOTE>
struct PsSlots {
    static constexpr bool SNDPF = !REMOTE;
    static constexpr int SLOTS = SNDPF ? TILE + TILE / 8 : TILE + TILE / 8 + TILE / 16;
    static constexpr int FU = (SLOTS + TPB - 1) / TPB;  // in-edges per thread in the in-edge pass
};

template <bool REMOTE>
struct TileLdsP {
    static constexpr int SLOTS = PsSlots<REMOTE>::SLOTS, SLOT_FU = PsSlots<REMOTE>::FU;
    uint32_t rows[W_ROWS + DMA_SLACK];
    uint32_t xm[W_PLANE + DMA_SLACK];
    uint32_t xp[W_PLANE + DMA_SLACK];
    uint32_t ind[TILE / 8 + DMA_SLACK];  // in-degrees of the tile's nodes, a nibble each (DevState::ind4)
    unsigned long long bits[SLOT_FU * (TPB / 64) + 1];  // bit q: in-edge q (tile order) was used by its sender; then 0
    double2 msg[SLOTS];               // edge q's message at slot q
    uint32_t out[TILE / 4];
    uint32_t red[2][TPB / 64];
    uint32_t qn[2];                   // walk 3: the block's next item, by iteration parity
    double2 zb[TPB / 64][NPT][2];     // (s, w) across each wave's ends, slot k: [0] node - 1, [1] node + 64
};

}  // namespace

// ---------------------------------------------------------------- push-sum
// One synchronous push-sum round (SRS v1 B.4; Program.fs:101-131) over a
// lattice slab, in pull form.  REMOTE: some in-edge senders live on other
// ranks (multi-GPU slabs); the single-GPU build has no exchange-tag paths.
//
// Per tile:
//   1. in-edge pass (Imp3D): did each in-edge's sender use its random edge
//      this round?  Every node active: the sender's own Philox draw, redrawn --
//      the senders are streamed in at the tile's start, and the FU redraws of a
//      thread run as one straight-line batch so the chains interleave; during
//      activation: the ballot-packed bitmap.  Used edges' (s, w) are gathered by
//      LDS-DMA into slot q (edge order);
//   2. staging by LDS-DMA: node bytes of the tile, its +-g rows and +-g^2 plane
//      segments, (s, w) across each wave's ends, the tile's nibble in-degrees
//      (Imp3D), whose prefix sums give each node's in-edge range;
//   3. per node: lattice senders from the staged bytes, one gather per
//      direction (no sender: the zero sentinel), the canonical fold (own half,
//      lattice slots in slot order, random edges by ascending sender), the ratio
//      test (Program.fs:114-123);
//      Under the slot's loads (nothing here needs what they return): the node's next-round
//      direction, drawn unconditionally and kept only if the node is active after the fold,
//      and the next slot's sender tests;
//   4. node bytes out as words, random-edge bits as one ballot per wave.
template <int TOPO, bool REMOTE>
__device__ __forceinline__ void ps_tiles(const RoundArgs& a, uint32_t r, TileLdsP<REMOTE>& L, uint32_t* snd,
                                         bool all_active, uint32_t& alerts, uint32_t& newly, bool& tiny) {
    const double2* __restrict__ swc = a.swc;
    double2* __restrict__ swn = a.swn;
    const uint64_t* __restrict__ rbc = a.rbc;
    const uint32_t* __restrict__ in_src = a.in_src;
    const bool packed = a.in_srcd != nullptr;  // staged senders carry deg - 4 in bits 30-31
    const uint32_t* __restrict__ srcp = packed ? a.in_srcd : in_src;
    const Geom G = a.G;
    const uint32_t H = TOPO == LINE ? 1u : G.g;
    constexpr int FU = PsSlots<REMOTE>::FU;
    const uint32_t cap = min((uint32_t)PsSlots<REMOTE>::SLOTS, a.stage_cap);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;

    // loaded one tile ahead: the next tile's in-edge range (two uniform loads); the
    // staged tile's senders, FU words per thread (loaded at the tile's start)
    uint32_t pf_tile = 0xFFFFFFFFu, pf_lo = 0, pf_hi = 0;
    uint32_t snd_tile = 0xFFFFFFFFu, snd_off = 0;  // SNDPF: snd holds tile snd_tile's senders from word snd_off
    constexpr bool SNDPF = PsSlots<REMOTE>::SNDPF;
    uint32_t raw[FU];
#pragma unroll
    for (int m = 0; m < FU; ++m) raw[m] = 0u;
    TileWalk tw(a);
    const bool dyn = tw.mode == 3;  // block-uniform
    uint32_t it = 0;                // iteration: parity selects the LDS slot of the next claim
    if (dyn) {
        if (blockIdx.x == 0 && threadIdx.x < 8) a.tq_next[threadIdx.x * TQ_STRIDE] = 0u;  // next round's counters
        if (threadIdx.x == 0) L.qn[0] = atomicAdd(tw.qc, 1u);
        __syncthreads();
        tw.t = __builtin_amdgcn_readfirstlane(L.qn[0]);
        ++it;
    }
    // walk 3: once this XCD's list is exhausted, the block takes items from the other
    // XCDs' queues in turn (their tiles' lattice lines are in another L2, but only
    // the round's tail runs this way), so no XCD idles while another has work
    for (uint32_t victim = 0;;) {
    while (tw.t < tw.end) {
        uint32_t ti;
        // walk 3: thread 0 claims the next item now; it is published in LDS at the
        // staging barrier (which waits for the atomic anyway)
        uint32_t claim = 0;
        if (dyn && threadIdx.x == 0) claim = atomicAdd(tw.qc, 1u);
        if (!tw.tile(ti)) {  // an empty item (a plane has fewer tiles than kp)
            if (dyn) {
                if (threadIdx.x == 0) L.qn[it & 1] = claim;
                __syncthreads();
                tw.t = __builtin_amdgcn_readfirstlane(L.qn[it & 1]);
                ++it;
            } else {
                tw.t += tw.step;
            }
            continue;
        }
        // tiles sit on global multiples of TILE (4-aligned word I/O, 64-aligned
        // ballot words); the slab's first and last tile may be partial
        const uint32_t T = (a.lo / TILE + ti) * TILE;
        const uint32_t j0 = max(a.lo, T);
        const uint32_t j1 = min(a.lo + a.nloc, T + TILE);
        const bool have_pf = pf_tile == ti;  // block-uniform
        uint32_t e_lo = 0, e_hi = 0;
        if (TOPO == IMP3D) {
            if (have_pf) {
                e_lo = pf_lo;
                e_hi = pf_hi;
            } else {
                e_lo = ld_const(a.in_off + j0);
                e_hi = ld_const(a.in_off + j1);
            }
        }
        const uint32_t cnt = e_hi - e_lo;
        const bool staged = cnt <= cap;
        // static walks: the next tile's in-edge range (two uniform loads, consumed next tile).
        // (Walk 3 does the same below, once its next item is known; written out twice: as one
        // helper given the walk position, the Imp3D kernels' instructions changed,
        // profiles/tile_split/isa_diff.txt.)
        if (TOPO == IMP3D && !dyn) {
            TileWalk nw = tw;
            nw.t += nw.step;
            uint32_t nti;
            pf_tile = 0xFFFFFFFFu;
            if (nw.t < nw.end && nw.tile(nti)) {
                const uint32_t nT = (a.lo / TILE + nti) * TILE;
                pf_lo = ld_const(a.in_off + max(a.lo, nT));
                pf_hi = ld_const(a.in_off + min(a.lo + a.nloc, nT + TILE));
                pf_tile = nti;
            }
        }
        if constexpr (TOPO == IMP3D) {
            if (staged) {
                // in-edge q = m * TPB + wave * 64 + lane is bit `lane` of bitmap word
                // m * 4 + wave; its message (if used) lands in slot q
                if (SNDPF && snd_tile == ti) {  // (block-uniform) prefetched during the last tile
                    // (the thread index opaque: the thread's LDS address in snd is then formed here, not
                    // kept in a register across the tile loop, where it spilled)
                    uint32_t ts = threadIdx.x;
                    asm volatile("" : "+v"(ts));
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const uint32_t q = ts + m * TPB;
                        raw[m] = q < cnt ? snd[snd_off + q] : 0u;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const uint32_t q = threadIdx.x + m * TPB;
                        raw[m] = q < cnt ? __builtin_nontemporal_load(srcp + e_lo + q) : 0u;
                    }
                }
                // REMOTE: the list keys of the tile's in-edges (meaningful for remote senders),
                // issued with the senders so their latency hides behind the draws (round 5 loaded
                // them after the draws: live across the Philox batch they spilled then; at 96 VGPRs
                // now without spills, C5 W = 8 REMOTE kernel -1.5 %, profiles/r06/remote/)
                uint32_t rkv[REMOTE ? FU : 1];
                if constexpr (REMOTE) {
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const uint32_t q = threadIdx.x + m * TPB;
                        rkv[m] = q < cnt ? __builtin_nontemporal_load(a.rk + e_lo + q) : 0u;
                    }
                }
                uint32_t isrc[FU];
                bool sent[FU], pick[FU];
#pragma unroll
                for (int m = 0; m < FU; ++m) isrc[m] = packed ? raw[m] & 0x3FFFFFFFu : raw[m];
                if (all_active) {
                    // the first NPT edges per thread cover a tile's mean in-degree (TILE);
                    // the slots above are drawn only by waves that hold an edge there
                    // (a wave-uniform test: most tiles have fewer than TILE + 64 in-edges)
                    constexpr int F0 = FU < NPT ? FU : NPT;
                    uint32_t x[FU], y[FU];
                    {
                        uint32_t n0[F0], x0[F0], y0[F0];
#pragma unroll
                        for (int m = 0; m < F0; ++m) n0[m] = isrc[m];
                        philox2_batch<F0>(n0, r, S_PUSHSUM, a.k0, a.k1, x0, y0);
#pragma unroll
                        for (int m = 0; m < F0; ++m) {
                            x[m] = x0[m];
                            y[m] = y0[m];
                        }
                    }
#pragma unroll
                    for (int m = F0; m < FU; ++m) {
                        x[m] = y[m] = 0u;
                        if (cnt > (uint32_t)(m * TPB) + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u)) {
                            uint32_t n1[1] = {isrc[m]}, x1[1], y1[1];
                            philox2_batch<1>(n1, r, S_PUSHSUM, a.k0, a.k1, x1, y1);
                            x[m] = x1[0];
                            y[m] = y1[0];
                        }
                    }
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const uint32_t q = threadIdx.x + m * TPB;
                        const uint32_t di = packed ? (raw[m] >> 30) + 4u : popc6(present_mask<IMP3D>(isrc[m], G)) + 1u;
                        sent[m] = pick[m] = q < cnt && uniform_from(x[m], y[m], di) == di - 1u;
                    }
                } else {
                    // activation: the sender sends on its random edge iff its draw picks
                    // that slot AND it is active -- redraw first, then read the ballot
                    // bitmap (bit = dir == random, i.e. both) only for the ~1/7 of edges
                    // the draw selects, instead of a random bitmap read per edge
                    uint32_t x[FU], y[FU];
                    philox2_batch<FU>(isrc, r, S_PUSHSUM, a.k0, a.k1, x, y);
                    // picks first, then every pick's bitmap word in flight together: loads
                    // unconditional (non-picks read the slab's first word, one shared line),
                    // since under a branch each load was waited on at once
                    bool lpick[FU];
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const uint32_t q = threadIdx.x + m * TPB;
                        const uint32_t i = isrc[m];
                        const uint32_t di = packed ? (raw[m] >> 30) + 4u : popc6(present_mask<IMP3D>(i, G)) + 1u;
                        pick[m] = q < cnt && uniform_from(x[m], y[m], di) == di - 1u;
                        lpick[m] = pick[m] && (!REMOTE || i - a.lo < a.nloc);
                    }
                    unsigned long long wbits[FU];
#pragma unroll
                    for (int m = 0; m < FU; ++m) wbits[m] = rbc[lpick[m] ? (isrc[m] >> 6) - (a.lo >> 6) : 0u];
                    // (the asm consumes every loaded word, so no load can be sunk into a
                    // branch on pick; its memory clobber keeps all loads ahead of the first)
#pragma unroll
                    for (int m = 0; m < FU; ++m) asm volatile("" : "+v"(wbits[m])::"memory");
#pragma unroll
                    for (int m = 0; m < FU; ++m) wbits[m] = lpick[m] ? wbits[m] : 0ull;
#pragma unroll
                    for (int m = 0; m < FU; ++m) sent[m] = (wbits[m] >> (isrc[m] & 63)) & 1ull;
                }
                // sender on another rank: its rank's list for this one says whether it used the
                // edge (the header word's bit) and where its message is (the word's base +
                // the used entries below it).  Only the drawn / picked edges (~1/7) read a
                // header word; the others load word 0 (one shared line), unconditionally,
                // so no load waits under a branch.
                uint32_t ridx[REMOTE ? FU : 1];
                if constexpr (REMOTE) {
                    uint2 hm[FU];
                    uint32_t hb[FU];
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        const bool cand = pick[m] && isrc[m] - a.lo >= a.nloc;
                        const XHdr* hp = a.xhdr + (cand ? rkv[m] >> 6 : 0u);
                        hm[m] = *reinterpret_cast<const uint2*>(&hp->mask);
                        hb[m] = hp->base;
                    }
#pragma unroll
                    for (int m = 0; m < FU; ++m) asm volatile("" : "+v"(hm[m].x), "+v"(hm[m].y), "+v"(hb[m])::"memory");
#pragma unroll
                    for (int m = 0; m < FU; ++m) {
                        ridx[m] = 0u;
                        if (pick[m] && isrc[m] - a.lo >= a.nloc) {
                            const unsigned long long mk = ((unsigned long long)hm[m].y << 32) | hm[m].x;
                            const uint32_t bit = rkv[m] & 63u;
                            sent[m] = (mk >> bit) & 1ull;
                            ridx[m] = min(hb[m] + (uint32_t)__popcll(mk & ((1ull << bit) - 1ull)), a.xnv - 1u);
                        }
                    }
                }
                __builtin_amdgcn_s_setprio(PRIO);
#pragma unroll
                for (int m = 0; m < FU; ++m) {
                    const unsigned long long bal = __ballot(sent[m]);
                    if (lane == 0) L.bits[m * (TPB / 64) + wv] = bal;
                    if (sent[m]) {
                        const double2* src;
                        if constexpr (REMOTE) {
                            // (the index opaque: hoisted out of the tile loop, per-lane addresses
                            // were spilled, and each reload waited vmcnt(0))
                            uint32_t xi = ridx[m];
                            asm volatile("" : "+v"(xi));
                            src = isrc[m] - a.lo >= a.nloc ? a.xvals + xi : swc + isrc[m];
                        } else {
                            src = swc + isrc[m];
                        }
                        __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(L.msg + (m * TPB + wv * 64)), 16,
                                                         0, DMA_ONCE);
                    }
                }
                if (threadIdx.x == 0) {
                    // (the zero made here: as a loop invariant it was kept in a register pair across the
                    // tile loop, and spilled)
                    unsigned long long z = 0ull;
                    asm volatile("" : "+v"(z));
                    L.bits[FU * (TPB / 64)] = z;
                }
            }
        }
        // own (s, w): loaded with the node's lattice gathers (ahead of the staging
        // copies it kept 12 more VGPRs live and measured slower)
        double2 own[NPT];
        // every staging copy of the tile in flight at once (LDS-DMA)
        const uint32_t b_rows = dma_stage_bytes(L.rows, a.nbc, (int64_t)j0 - H, (int64_t)j1 + H, a.ext_lo, a.ext_hi);
        uint32_t b_xm = 0, b_xp = 0;
        if (TOPO != LINE) {
            b_xm = dma_stage_bytes(L.xm, a.nbc, (int64_t)j0 - G.g2, (int64_t)j1 - G.g2, a.ext_lo, a.ext_hi);
            b_xp = dma_stage_bytes(L.xp, a.nbc, (int64_t)j0 + G.g2, (int64_t)j1 + G.g2, a.ext_lo, a.ext_hi);
        }
        // (s, w) across every wave's ends, slot k: node T + k*TPB + 64 wave - 1 and + 64
        // (clamped into the node arrays; used only where that neighbour sent)
        {
            // (the thread index opaque: the lane's and the wave's parts of the index and the wave's LDS
            // address are then computed here, per tile, not kept in registers across the tile loop,
            // where they spilled)
            uint32_t zt = threadIdx.x;
            asm volatile("" : "+v"(zt));
            const uint32_t zl = zt & 63u, zw = zt >> 6;
            if (zl < 2u * NPT) {
                int64_t jn = (int64_t)T + (int64_t)((zl >> 1) * TPB + zw * 64u) + ((zl & 1u) ? 64 : -1);
                if (jn < (int64_t)a.ext_lo) jn = a.ext_lo;
                if (jn > (int64_t)a.ext_hi) jn = a.ext_hi;
                __builtin_amdgcn_global_load_lds((gvoid_t*)(swc + jn), (lvoid_t*)&L.zb[zw][0][0], 16, 0, 0);
            }
        }
        // the tile's in-degrees, a nibble per node (512 bytes; the slab's arrays
        // cover whole tiles, ids outside the slab are 0)
        if (TOPO == IMP3D) {
            // (the tile's base and the thread index opaque: otherwise a.ind4 + the thread's offset, or
            // the offset, is kept as a 64-bit value across the tile loop, and spilled.  dma_copy's
            // one pass written out: 16 bytes per lane of the first TILE / 32 threads)
            const uint8_t* ip = a.ind4 + T / 2;
            asm volatile("" : "+s"(ip));
            uint32_t nt = threadIdx.x;
            asm volatile("" : "+v"(nt));
            if (nt < (uint32_t)(TILE / 32))
                __builtin_amdgcn_global_load_lds((gvoid_t*)(ip + nt * 16u), (lvoid_t*)L.ind, 16, 0, DMA_ONCE);
        }
        if (dyn && threadIdx.x == 0) L.qn[it & 1] = claim;
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();  // staging copies, in-edge bitmap and gathered messages retired
        // Imp3D: node jl's in-edges are [e_lo + pre(jl), + d(jl)), pre = exclusive
        // prefix of the nibble in-degrees.  Every wave sums all 16 64-node chunks
        // (lane L: nodes 16L..16L+15) and keeps the prefixes of its own chunks
        // 4k + wave (scalars); the lane part comes from ballots in the node loop.
        // A tile holding a node of in-degree >= 15 (nibble 15, ~1e-12 of nodes)
        // reads in_off from HBM instead.
        uint32_t cinc = 0;
        bool wide = false;
        if (TOPO == IMP3D) {
            const uint2 w2 = reinterpret_cast<const uint2*>(L.ind)[lane];
            auto nsum = [](uint32_t w) { return (((w & 0x0F0F0F0Fu) + ((w >> 4) & 0x0F0F0F0Fu)) * 0x01010101u) >> 24; };
            auto has15 = [](uint32_t w) { return (w & (w >> 1) & (w >> 2) & (w >> 3) & 0x11111111u) != 0u; };
            uint32_t incl = nsum(w2.x) + nsum(w2.y);
            wide = __ballot(has15(w2.x) || has15(w2.y)) != 0ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o, 64);
                if (lane >= (uint32_t)o) incl += t;
            }
            // exclusive chunk prefix at lane 4c (read per slot in the node loop)
            const uint32_t ex = __shfl_up(incl, 1, 64);
            cinc = lane == 0 ? 0u : ex;
        }
        uint32_t t_next = tw.t + tw.step;
        if (dyn) {
            // (block-uniform, and known to be: the next tile's in-list range is then two scalar
            // loads, not vector loads whose wait at the next tile's start also waited for this
            // tile's state stores)
            t_next = __builtin_amdgcn_readfirstlane(L.qn[it & 1]);
            ++it;
            // the next tile's in-edge range (two uniform loads, consumed next tile)
            if (TOPO == IMP3D) {
                TileWalk nw = tw;
                nw.t = t_next;
                uint32_t nti;
                pf_tile = 0xFFFFFFFFu;
                if (nw.t < nw.end && nw.tile(nti)) {
                    const uint32_t nT = (a.lo / TILE + nti) * TILE;
                    pf_lo = ld_const(a.in_off + max(a.lo, nT));
                    pf_hi = ld_const(a.in_off + min(a.lo + a.nloc, nT + TILE));
                    pf_tile = nti;
                }
            }
        }

        // The node phase, the direction draws and the byte write-out are compiled twice.  FULL: the
        // tile lies wholly inside the slab and (Imp3D) is staged and not `wide` -- all but the
        // slab's first and last tile and the ~4e-5 of tiles above the staging cap.  Every node
        // is then valid: no range tests, no clamp of the own index, no loads for j +- 1 outside
        // the range, only the bitmap-window in-edge walk; the z +- 1 sender tests take the
        // neighbour lanes' direction byte by DPP.  !FULL serves every other tile.
        bool full = j0 == T && j1 == T + TILE && (TOPO != IMP3D || (staged && !wide));  // block-uniform
#ifdef GP_EXPERIMENTS
        if (a.no_full) full = false;  // GP_NO_FULLTILE=1: every tile through the general body (A/B, parity tests)
#endif
        // SHADOW: a slot's work that needs nothing its loads return -- the node's next-round
        // direction draw, and deciding the next slot -- runs between the loads' issue and their
        // wait.
        auto tile_body = [&](auto full_c, auto shadow_c) {
        constexpr bool FULL = decltype(full_c)::value;
        constexpr bool SHADOW = decltype(shadow_c)::value;
        // the thread index is opaque to each body: what a body derives from it (lane tests, byte
        // offsets, per-thread address parts) is computed once per tile, not hoisted out of the tile
        // loop into registers that stay live across the in-edge pass (two bodies' worth spilled)
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const uint32_t lane = tid & 63u, wv = tid >> 6;
        // per node, 16 bits (two nodes per word).  SHADOW: the next-round node byte -- bits 0-2 the
        // candidate direction parked before the fold, raised to DIR_NONE after it if the node does
        // not send, bits 3-6 the flags.  Otherwise: bits 0-5 lattice mask, bit 6 draw a next-round
        // direction, bits 7-10 the node byte's flag bits 3-6
        uint32_t pend[(NPT + 1) / 2];
#pragma unroll
        for (int k = 0; k < (NPT + 1) / 2; ++k) pend[k] = 0u;
        {
            // Lattice coordinates of the WAVE's first node of slot k (wave-uniform, so
            // scalar), advanced by TPB per slot.  A wave whose 64 nodes are all
            // interior (no lattice boundary; ~93 % of waves at g = 1000) takes mask =
            // 63 without per-lane coordinates; the others compute each node's mask.
            const uint32_t wbase = __builtin_amdgcn_readfirstlane(tid & ~63u);
            uint32_t wcx = 0, wcy = 0, wcz = 0;
            if (TOPO != LINE) {
                const uint32_t jw = T + wbase;
                wcx = fastdiv(jw, G.div_g2);
                const uint32_t rem = jw - wcx * G.g2;
                wcy = fastdiv(rem, G.div_g);
                wcz = rem - wcy * G.g;
            }
            // lattice directions gathered from HBM / L2; the j +- 1 ones (z +- 1, or both
            // line neighbours) are the neighbour lanes' own (s, w)
            constexpr uint32_t NDG = TOPO == LINE ? 0u : 4u;
            // A slot in two parts.  decide(k): what the staged LDS bytes and the wave coordinates
            // settle -- the node's in-edge range (all lanes take part in the ballots), its byte,
            // present mask and lattice senders, packed as byte | mask << 8 | from << 14 |
            // in-degree << 20 (one register) -- and the coordinate step to slot k.  Then the issue:
            // own (s, w) and one gather per direction, whose addresses `from` picks.
            auto decide = [&](const int k, uint32_t& gst, uint32_t& epre) {
                epre = 0u;
                uint32_t edeg = 0u;
                if (TOPO == IMP3D) {
                    const uint32_t jl = k * TPB + tid;
                    const uint32_t d = (lds_byte(L.ind, jl >> 1) >> ((jl & 1u) * 4u)) & 15u;
                    uint32_t ex = mbcnt64(__ballot(d & 1u)) + 2u * mbcnt64(__ballot(d & 2u));
                    if (__ballot(d >= 4u)) ex += 4u * mbcnt64(__ballot(d & 4u)) + 8u * mbcnt64(__ballot(d & 8u));
                    const int wvu = __builtin_amdgcn_readfirstlane((int)wv);
                    epre = (uint32_t)__builtin_amdgcn_readlane((int)cinc, 16 * k + 4 * wvu) + ex;
                    edeg = d;
                }
                const uint32_t j = T + k * TPB + tid;
                if (TOPO != LINE && k > 0) {
                    wcz += TPB;
                    if (wcz >= G.g) {
                        const uint32_t q = fastdiv(wcz, G.div_g);
                        wcz -= q * G.g;
                        wcy += q;
                        if (wcy >= G.g) {
                            const uint32_t q2 = fastdiv(wcy, G.div_g);
                            wcy -= q2 * G.g;
                            wcx += q2;
                        }
                    }
                }
                const uint32_t jr = j - b_rows;
                const uint32_t gbv = lds_byte(L.rows, jr);
                uint32_t mask;
                if (TOPO == LINE) {
                    mask = present_mask<TOPO>(j, G);
                } else {
                    const uint32_t gm = G.g - 1u;
                    const bool interior = wcz >= 1u && wcz + 64u < gm && wcy >= 1u && wcy < gm && wcx >= 1u && wcx < gm;
                    mask = interior ? 63u : present_mask<TOPO>(j, G);
                }
                uint32_t from = 0;
                if (TOPO == LINE) {
                    from |= ((mask & 1u) && (lds_byte(L.rows, (mask & 1u) ? jr - 1 : jr) & DIR_MASK) == 1u) ? 1u : 0u;
                    from |= ((mask & 2u) && (lds_byte(L.rows, (mask & 2u) ? jr + 1 : jr) & DIR_MASK) == 0u) ? 2u : 0u;
                } else {
                    // absent neighbours read a harmless in-range byte and are masked out
                    const uint32_t bxm = lds_byte(L.xm, (mask & 1u) ? j - G.g2 - b_xm : 0u);
                    const uint32_t bxp = lds_byte(L.xp, (mask & 2u) ? j + G.g2 - b_xp : 0u);
                    const uint32_t byp = lds_byte(L.rows, (mask & 4u) ? jr + G.g : jr);
                    const uint32_t bym = lds_byte(L.rows, (mask & 8u) ? jr - G.g : jr);
                    uint32_t bzp, bzm;
                    if constexpr (FULL) {
                        // z +- 1 are lanes +- 1: their direction byte by DPP (every lane is
                        // active in a full tile); across the wave's ends one LDS byte: lane 63
                        // reads j + 1, lane 0 j - 1 (index kept >= 0: node 0 has no z - 1), the
                        // lanes between read j - 1 as well and do not use it
                        const uint32_t be = lds_byte(L.rows, lane == 63u ? jr + 1u : max(jr, 1u) - 1u);
                        bzp = (uint32_t)__builtin_amdgcn_mov_dpp((int)gbv, 0x130, 0xF, 0xF, true);
                        bzm = (uint32_t)__builtin_amdgcn_mov_dpp((int)gbv, 0x138, 0xF, 0xF, true);
                        if (lane == 63u) bzp = be;
                        if (lane == 0u) bzm = be;
                    } else {
                        bzp = lds_byte(L.rows, (mask & 16u) ? jr + 1 : jr);
                        bzm = lds_byte(L.rows, (mask & 32u) ? jr - 1 : jr);
                    }
                    from =((bxm & DIR_MASK) == 1u ? 1u : 0u) | ((bxp & DIR_MASK) == 0u ? 2u : 0u) |
                           ((byp & DIR_MASK) == 3u ? 4u : 0u) | ((bym & DIR_MASK) == 2u ? 8u : 0u) |
                           ((bzp & DIR_MASK) == 5u ? 16u : 0u) | ((bzm & DIR_MASK) == 4u ? 32u : 0u);
                    from &= mask;
                }
                if (!FULL && !(j >= j0 && j < j1)) from = 0u;
                gst = gbv | (mask << 8) | (from << 14) | (edeg << 20);
            };
            // SHADOW: slot k + 1 is decided while slot k's loads are in flight, and only its packed
            // word and in-edge prefix are carried to its issue; slot 0 is decided here, after the
            // staging barrier.  One node slot's loads are in flight at a time (two at 5 waves/SIMD
            // spilled 49 VGPRs).
            constexpr bool AHEAD = SHADOW;
            uint32_t gst_n = 0u, epre_n = 0u;
            if (AHEAD) {
                __builtin_amdgcn_s_setprio(PRIO);
                decide(0, gst_n, epre_n);
            }
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                __builtin_amdgcn_s_setprio(PRIO);
                // phase A: decide (above), then one gather per direction -- a direction without a
                // sender reads the zero sentinel swc[ext_hi] (adding +0.0 is exact)
                uint32_t gst, epre;
                if (AHEAD) {
                    gst = gst_n;
                    epre = epre_n;
                } else {
                    decide(k, gst, epre);
                }
                const uint32_t jl = k * TPB + tid;
                const uint32_t j = T + jl;
                double2 m[NDG > 0 ? NDG : 1];
                {
                    const uint32_t from = (gst >> 14) & 63u;
                    // unconditional (index clamped into the tile's valid range; invalid lanes'
                    // values are never used): a load under a branch made the compiler wait
                    // for it before issuing the lattice gathers
                    own[k] = swc[FULL ? j : min(max(j, j0), j1 - 1u)];
#pragma unroll
                    for (uint32_t d = 0; d < NDG; ++d)
                        m[d] = ld_sw(swc + ((from >> d) & 1u ? nbr<TOPO>(j, d, G) : a.ext_hi));
                }
                __builtin_amdgcn_s_setprio(0);
                // SHADOW: everything from here to the second barrier needs nothing the slot's loads
                // return and runs while they are in flight; the scheduler may neither hoist it above
                // their issue nor sink it below the wait
                if (SHADOW) __builtin_amdgcn_sched_barrier(0);
                // phase B: canonical fold (own half, lattice slots in slot order, random
                // edges by ascending sender; every message contributes the sender's half),
                // ratio test, next-round state
                {
                    const bool valid = FULL || (j >= j0 && j < j1);
                    // Imp3D, staged tile: the node's window of the used-in-edge bitmap and its first
                    // used in-edge's message, read from LDS while the slot's loads are in flight (the
                    // fold needed both after the loads, one LDS round trip after the other).  A node's
                    // in-edges fit one 32-bit window (in-degree <= 14 outside `wide` tiles).
                    uint32_t pwin = 0u, pqb = 0u;
                    if (TOPO == IMP3D && (FULL || (staged && !wide))) {
                        const uint32_t* bw = reinterpret_cast<const uint32_t*>(L.bits);
                        pqb = epre;
                        const uint32_t nd = gst >> 20;
                        pwin = __builtin_amdgcn_alignbit(bw[(pqb >> 5) + 1], bw[pqb >> 5], pqb & 31u) & ((1u << nd) - 1u);
                    }
                    if (SHADOW) {
                        // the node's next-round draw depends on its id, the round and its degree alone:
                        // drawn unconditionally, reduced to the candidate direction and parked in the
                        // direction bits of the node's half of `pend`; whether the node sends at all
                        // is known only after the fold
                        uint32_t x, y;
                        philox2(j, r + 1, S_PUSHSUM, a.k0, a.k1, x, y);
                        const uint32_t mask = (gst >> 8) & 63u;
                        const uint32_t cand = slot_to_dir_fast(mask, uniform_from(x, y, popc6(mask) + (TOPO == IMP3D ? 1u : 0u)));
                        pend[k >> 1] |= cand << (16 * (k & 1));
                        if (AHEAD && k + 1 < NPT) decide(k + 1, gst_n, epre_n);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // j + 1 / j - 1: the neighbour lane's own (s, w) by DPP (all lanes active
                    // here), across the wave's ends from the values staged in L.zb; a load
                    // only where that lane's node is outside the tile's valid range
                    // (partial tiles at slab ends)
                    double2 zP = make_double2(0.0, 0.0), zM = zP;
                    {
                        constexpr uint32_t dP = TOPO == LINE ? 1u : 4u, dM = TOPO == LINE ? 0u : 5u;
                        const uint32_t from = (gst >> 14) & 63u;
                        zP = dpp_double2<0x130>(own[k]);  // wave_shl:1 -- lane + 1's (s, w)
                        zM = dpp_double2<0x138>(own[k]);  // wave_shr:1 -- lane - 1's (s, w)
                        if (lane == 63u) zP = L.zb[wv][k][1];
                        if (lane == 0u) zM = L.zb[wv][k][0];
                        if (!((from >> dP) & 1u)) zP = make_double2(0.0, 0.0);
                        else if (!FULL && lane != 63u && j + 1u >= j1) zP = ld_sw(swc + j + 1);
                        if (!((from >> dM) & 1u)) zM = make_double2(0.0, 0.0);
                        else if (!FULL && lane != 0u && j <= j0) zM = ld_sw(swc + j - 1);
                    }
                    // every load of the slot retired here, on all paths: the slot's state store is then the
                    // only memory operation the next slot's loads could wait for, and they do not
                    // (without it the compiler waited vmcnt(0) before every slot's gathers -- a lane
                    // range with no valid node skips the fold that consumes the loads)
                    __builtin_amdgcn_s_waitcnt(vmcnt_enc(0));
                    if (valid) {
                        const uint32_t b = gst & 0xFFu, mask = (gst >> 8) & 63u, from = (gst >> 14) & 63u;
                        const uint32_t deg = popc6(mask) + (TOPO == IMP3D ? 1u : 0u);
                        bool active = (b & B_ACTIVE) != 0;
                        const double2 sv = own[k];

                        const bool halve = active && deg > 0;
                        const double hf = halve ? 0.5 : 1.0;  // exact either way
                        double acc_s = sv.x * hf;
                        double acc_w = sv.y * hf;
                        // fused: fma(m, 0.5, acc) rounds once, exactly like the specification's
                        // acc + m * 0.5 whenever m * 0.5 is exact, i.e. |m| >= 2^-1021; every
                        // node checks its own round-start (s, w) -- the values its messages
                        // carry this round -- against 2^-1020 (Ctl::tiny, gp_step fails)
                        auto fold = [&](const double2 mi) {
                            acc_s = __builtin_fma(mi.x, 0.5, acc_s);
                            acc_w = __builtin_fma(mi.y, 0.5, acc_w);
                        };
                        tiny |= (sv.y < 0x1p-1020) | (sv.x != 0.0 && sv.x < 0x1p-1020);
                        bool recv = from != 0;
                        // lattice slots in slot order: line j-1, j+1; 3D x-1, x+1, y+1, y-1, z+1, z-1
                        if (TOPO == LINE) {
                            fold(zM);
                            fold(zP);
                        } else {
#pragma unroll
                            for (uint32_t d = 0; d < NDG; ++d) fold(m[d]);
                            fold(zP);
                            fold(zM);
                        }
                        if (TOPO == IMP3D) {
                            uint32_t e_b = e_lo + epre, e_e = e_b + (gst >> 20);
                            if (!FULL && wide) {
                                e_b = a.in_off[j];
                                e_e = a.in_off[j + 1];
                            }
                            if (FULL || (staged && !wide)) {
                                // the window and first message read above; the rest set bit by set
                                // bit (ascending sender = canonical order), edge q's message at slot q
                                uint32_t win = pwin;
                                while (win) {
                                    const uint32_t q = pqb + (uint32_t)__builtin_ctz(win);
                                    win &= win - 1u;
                                    fold(L.msg[q]);
                                    recv = true;
                                }
                            } else if (staged) {
                                // the node's used in-edges: its window of the tile bitmap, 32 bits
                                // at a time (funnel shift of two LDS words), walked set bit by set
                                // bit (ascending sender = canonical order); edge q's message is at
                                // slot q
                                const uint32_t* bw = reinterpret_cast<const uint32_t*>(L.bits);
                                const uint32_t qe = e_e - e_lo;
                                for (uint32_t q0 = e_b - e_lo; q0 < qe; q0 += 32u) {
                                    uint32_t win = __builtin_amdgcn_alignbit(bw[(q0 >> 5) + 1], bw[q0 >> 5], q0 & 31u);
                                    if (qe - q0 < 32u) win &= (1u << (qe - q0)) - 1u;
                                    while (win) {
                                        const uint32_t q = q0 + (uint32_t)__builtin_ctz(win);
                                        win &= win - 1u;
                                        fold(L.msg[q]);
                                        recv = true;
                                    }
                                }
                            } else {  // rare: tile in-degree above SLOTS
                                for (uint32_t e = e_b; e < e_e; ++e) {
                                    const uint32_t i = in_src[e];
                                    bool sent;
                                    double2 mi = make_double2(0.0, 0.0);
                                    const bool rem = REMOTE && i - a.lo >= a.nloc;
                                    uint32_t xi = 0;
                                    if (rem) {  // the sender's list entry (see the in-edge pass)
                                        const uint32_t k = a.rk[e];
                                        const XHdr h = a.xhdr[k >> 6];
                                        sent = (h.mask >> (k & 63u)) & 1ull;
                                        xi = min(h.base + (uint32_t)__popcll(h.mask & ((1ull << (k & 63u)) - 1ull)),
                                                 a.xnv - 1u);
                                    } else if (all_active) {
                                        const uint32_t di = popc6(present_mask<IMP3D>(i, G)) + 1u;
                                        sent = uniform(a.k0, a.k1, S_PUSHSUM, i, r, di) == di - 1u;
                                    } else {
                                        sent = (rbc[(i >> 6) - (a.lo >> 6)] >> (i & 63)) & 1ull;
                                    }
                                    if (sent) mi = rem ? a.xvals[xi] : ld_sw(swc + i);
                                    if (sent) {
                                        fold(mi);
                                        recv = true;
                                    }
                                }
                            }
                        }
                        uint32_t flags = b & (B_ACTIVE | B_CONV | (3u << CNT_SHIFT));
                        if (recv) {
                            if (!(b & B_CONV)) {
                                uint32_t cnt3 = (b >> CNT_SHIFT) & 3u;
                                cnt3 = ratio_moved(sv.x, sv.y, acc_s, acc_w) ? 0u : cnt3 + 1u;
                                flags = (flags & ~(3u << CNT_SHIFT)) | (cnt3 << CNT_SHIFT);
                                if (cnt3 == 3) {
                                    flags |= B_CONV;
                                    ++alerts;
                                }
                            }
                            if (!active) {
                                ++newly;
                                flags |= B_ACTIVE;
                                active = true;
                            }
                        }
                        if (SHADOW) {
                            // the parked candidate stands if the node sends; DIR_NONE (all three bits) otherwise
                            pend[k >> 1] |= ((active && deg > 0 ? 0u : (uint32_t)DIR_NONE) | (flags & 0x78u)) << (16 * (k & 1));
                        } else {
                            // next-round direction drawn below, one Philox batch for the thread's nodes
                            pend[k >> 1] |= (mask | (active && deg > 0 ? 64u : 0u) | ((flags >> 3) << 7)) << (16 * (k & 1));
                        }
                        st_stream(swn + j, make_double2(acc_s, acc_w));
                    }
                }
                // SNDPF: after the first node slot (the next tile's in-edge range has arrived by
                // then), its senders by LDS-DMA; this tile's were read in its in-edge pass, and the
                // tile's closing barrier retires the copy before the next tile reads it
                if (SNDPF && TOPO == IMP3D && k == 0) {
                    snd_tile = 0xFFFFFFFFu;
                    if (pf_tile != 0xFFFFFFFFu && pf_hi - pf_lo <= cap) {
                        snd_off = dma_stage_words(snd, srcp, pf_lo, pf_hi);
                        snd_tile = pf_tile;
                    }
                }
            }
        }
        // next-round node bytes of this thread's nodes (SHADOW: as the slots left them; otherwise
        // the directions are drawn here, one Philox batch)
        {
            uint32_t node[NPT], x[NPT], y[NPT];
#pragma unroll
            for (int k = 0; k < NPT; ++k) node[k] = T + k * TPB + tid;
            if (!SHADOW) philox2_batch<NPT>(node, r + 1, S_PUSHSUM, a.k0, a.k1, x, y);
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                const uint32_t jl = k * TPB + tid;
                const bool valid = FULL || (node[k] >= j0 && node[k] < j1);
                const uint32_t pk = pend[k >> 1] >> (16 * (k & 1));
                uint32_t dir, nb;
                if (SHADOW) {
                    dir = pk & DIR_MASK;
                    nb = pk & 0x7Fu;
                } else {
                    const uint32_t mask = pk & 63u;
                    dir = DIR_NONE;
                    if (pk & 64u) dir = slot_to_dir_fast(mask, uniform_from(x[k], y[k], popc6(mask) + (TOPO == IMP3D ? 1u : 0u)));
                    nb = (((pk >> 7) & 15u) << 3) | dir;
                }
                if (valid) reinterpret_cast<uint8_t*>(L.out)[jl] = (uint8_t)nb;
                if (TOPO == IMP3D) {
                    const unsigned long long bits = __ballot(valid && dir == DIR_RANDOM);
                    if (lane == 0) {  // the slab's first tile may start below lo: no word there
                        const int64_t wi = (int64_t)((T + k * TPB + (tid & ~63u)) >> 6) - (int64_t)(a.lo >> 6);
                        if (wi >= 0) a.rbn[wi] = bits;
                    }
                }
            }
        }
        __syncthreads();
        // node bytes out as words (allocations are padded past P)
        for (uint32_t w = tid; w < (uint32_t)(TILE / 4); w += TPB) {
            const uint32_t jw = T + w * 4;
            if (FULL || (jw >= j0 && jw + 4 <= j1)) {
                st_stream(reinterpret_cast<uint32_t*>(a.nbn + T) + w, L.out[w]);
            } else {
                for (uint32_t b = 0; b < 4; ++b)
                    if (jw + b >= j0 && jw + b < j1) a.nbn[jw + b] = reinterpret_cast<const uint8_t*>(L.out)[w * 4 + b];
            }
        }
        };
#ifdef GP_EXPERIMENTS
        if (!a.slot_shadow) {  // GP_SLOT_SHADOW=0: the batch draw at the tile's end, every slot decided at its start (A/B)
            if (full) tile_body(std::true_type{}, std::false_type{});
            else tile_body(std::false_type{}, std::false_type{});
        } else
#endif
        if (full) tile_body(std::true_type{}, std::true_type{});
        else tile_body(std::false_type{}, std::true_type{});
        // no barrier here: the next tile's in-edge pass and staging copies write
        // bits / msg / rows / xm / xp / ind, none of which this byte output reads,
        // and its node phase writes L.out only after its staging barrier
        tw.t = t_next;
    }
        if (!dyn || ++victim >= 8u) break;
        const uint32_t c = (blockIdx.x + victim) & 7u;
        tw.qc = a.tq + c * TQ_STRIDE;
        tw.wl = a.wt + a.wo[c];
        tw.end = a.wo[c + 1] - a.wo[c];
        if (threadIdx.x == 0) L.qn[it & 1] = atomicAdd(tw.qc, 1u);
        __syncthreads();
        tw.t = __builtin_amdgcn_readfirstlane(L.qn[it & 1]);
        ++it;
    }
}

// Block sums of this block's alerts / newly active nodes (valid in thread 0).
// Uses L.red; the barrier also orders the block's last byte output before any
// later LDS reuse.
__device__ __forceinline__ void block_counts(uint32_t (*red)[TPB / 64], uint32_t& x, uint32_t& y) {
    // (the thread index opaque: lane and wave are then formed here, at the kernel's end, not kept
    // in registers across the caller's tile loop)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63u, wv = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x += __shfl_xor(x, o, 64);
        y += __shfl_xor(y, o, 64);
    }
    if (lane == 0) {
        red[0][wv] = x;
        red[1][wv] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        x = 0;
        y = 0;
        for (int w = 0; w < TPB / 64; ++w) {
            x += red[0][w];
            y += red[1][w];
        }
    }
}

// Thread 0: add the block's counts to the round accumulators with returning
// atomics and wait for them, so they are performed before the block arrives
// at the round close.
__device__ __forceinline__ void add_round_counts(Ctl* ctl, uint32_t x, uint32_t y) {
    unsigned long long d = 0;
    if (x) d += __hip_atomic_fetch_add(&ctl->round_alerts, (unsigned long long)x, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    if (y) d += __hip_atomic_fetch_add(&ctl->round_active, (unsigned long long)y, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"v"(d));
    __builtin_amdgcn_s_waitcnt(0);
}

template <int TOPO, bool REMOTE>
__global__ __launch_bounds__(TPB, GP_MINB) void k_ps_tile(RoundArgs a, uint32_t r) {
    __shared__ TileLdsP<REMOTE> L;
    // one rank: the next tile's in-edge senders, LDS-DMA'd during this tile's node phase.  An LDS
    // object of its own, so the compiler can tell that the node phase's LDS reads do not read it
    // and does not wait for the copy before each of them
    __shared__ uint32_t snd[PsSlots<REMOTE>::SNDPF ? PsSlots<REMOTE>::SLOTS + DMA_SLACK : 1];
    Ctl* ctl = a.ctl;
    if (ld_agent(&ctl->done)) return;
    const bool all_active = ld_agent(&ctl->all_active) != 0;
    uint32_t alerts = 0, newly = 0;
    bool tiny = false;
    ps_tiles<TOPO, REMOTE>(a, r, L, snd, all_active, alerts, newly, tiny);
    if (__ballot(tiny) && (threadIdx.x & 63u) == 0) atomicOr(&ctl->tiny, 1u);
    block_counts(L.red, alerts, newly);
    if (threadIdx.x == 0) {
        if (a.fuse == 2) {
            block_done_close_sharded(ctl, a.G.P, a.G.T, r, alerts, newly);
        } else if (a.fuse) {
            add_round_counts(ctl, alerts, newly);
            block_done_close(ctl, a.G.P, a.G.T, r);
        } else {
            if (alerts) atomicAdd(&ctl->round_alerts, (unsigned long long)alerts);
            if (newly) atomicAdd(&ctl->round_active, (unsigned long long)newly);
        }
    }
}


// The kernel of a topology (remote: the Imp3D slab of a multi-rank run, whose in-edge
// senders may live on other ranks); null where this size class does not build one.
using PsTileKernel = void (*)(RoundArgs, uint32_t);
static PsTileKernel ps_tile_kernel(int topo, bool remote) {
    if (topo == LINE) return k_ps_tile<LINE, false>;
    if (topo == GRID3D) return k_ps_tile<GRID3D, false>;
#ifndef GP_TILE_WIDE
    if (topo == IMP3D) return remote ? k_ps_tile<IMP3D, true> : k_ps_tile<IMP3D, false>;
#endif
    return nullptr;
}

// Resident blocks of the push-sum tile kernel on this device (walk 3 runs exactly
// that grid); 0 if unknown.
int ps_tile_resident_blocks(int topo, bool remote, int device) {
    const PsTileKernel f = ps_tile_kernel(topo, remote);
    int per_cu = 0, cus = 0;
    if (!f) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(f), TPB, 0) != hipSuccess)
        return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    return per_cu * cus;
}

// The push-sum half of launch_round_tile (gp_tile_host.hip).
hipError_t launch_ps_tile(const DevState& S, const RoundArgs& a, uint32_t round, int grid, hipStream_t st) {
    const PsTileKernel f = ps_tile_kernel(S.topo, S.rk != nullptr);
    if (!f || (S.topo == IMP3D && !S.ind4)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3(grid), dim3(TPB), 0, st, a, round);
    return hipGetLastError();
}

#ifdef GP_TILE_WIDE
}  // namespace wide
#else
// Launch h of round `round` when the round kernel runs region by region (DevState::rregions;
// Imp3D push-sum across ranks): region h's tiles, its own pair of queue counters by launch parity.
hipError_t launch_round_tile_region(const DevState& S, uint32_t round, uint32_t h, int grid, hipStream_t st) {
    if (S.alg != PUSHSUM || S.topo != IMP3D || !S.rk || !S.ind4 || !S.wtiles || S.tile_walk != 3 ||
        h >= S.rregions || (grid & 7))
        return hipErrorInvalidValue;
    RoundArgs a = make_round_args(S, round);
    for (int c = 0; c <= 8; ++c) a.wo[c] = S.woff[h][c];
    const uint64_t L = (uint64_t)round * S.rregions + h;
    a.tq = S.tq + (L & 1) * 8 * TQ_STRIDE;
    a.tq_next = S.tq + ((L + 1) & 1) * 8 * TQ_STRIDE;
    hipLaunchKernelGGL((k_ps_tile<IMP3D, true>), dim3(grid), dim3(TPB), 0, st, a, round);
    return hipGetLastError();
}
#endif
}  // namespace gp
