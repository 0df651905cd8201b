// gp_block_plan.hpp -- the box grid of the LDS-resident push-sum kernel (gp_block.hip).
// Host-only and free of HIP headers, so that a plain C++ program can evaluate the plan for
// any (cus, g) (tests/helpers/block_plan_check.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>

namespace gp {

constexpr int BK_THREADS = 1024;  // threads of a box's workgroup
constexpr int BK_NPT = 5;         // nodes per thread: boxes of at most 5120 nodes
constexpr uint32_t BK_LDS_MAX = 150 * 1024;  // dynamic LDS a box may ask for (a CU has 160 KiB)

// KERNEL_BLOCK (gp_block.hip): the lattice cut into nbx * nby * nbz boxes, one per workgroup.
struct BlockPlan {
    uint32_t nbx, nby, nbz;  // boxes per axis
    uint32_t vmax, fmax;     // largest box (nodes) and largest face
    uint32_t lds;            // dynamic LDS bytes per workgroup
};

// The box grid of a g^3 lattice for `cus` workgroups: the most boxes (at most one per
// CU, a box of at most BK_NPT * 1024 nodes) with the smallest largest box, whose LDS
// (17 bytes per node and per halo node) fits; false if none does.
inline bool block_plan(uint32_t g, int cus, BlockPlan& p) {
    bool found = false;
    uint64_t best_v = ~0ull;
    for (uint32_t nx = 1; nx <= g && nx <= (uint32_t)cus; ++nx)
        for (uint32_t ny = 1; ny <= g && nx * ny <= (uint32_t)cus; ++ny)
            for (uint32_t nz = 1; nz <= g && nx * ny * nz <= (uint32_t)cus; ++nz) {
                const uint64_t bx = (g + nx - 1) / nx, by = (g + ny - 1) / ny, bz = (g + nz - 1) / nz;
                const uint64_t v = bx * by * bz;
                const uint64_t f = std::max(by * bz, std::max(bx * bz, bx * by));
                const uint64_t ns = v + 6 * f + 1;
                const uint64_t lds = 16 * ns + ((ns + 3) & ~3ull) + ((v + 3) & ~3ull) + 4 * v + 64;
                if (v > (uint64_t)BK_NPT * BK_THREADS || lds > BK_LDS_MAX || bx > 1023 || by > 1023 || bz > 1023)
                    continue;
                // estimated round time: node slots per thread (ceil(v / 1024)) plus a grid barrier
                // (~3 slots) when there are several boxes; then the fewest boxes (less face traffic)
                const uint64_t nbk = (uint64_t)nx * ny * nz;
                const uint64_t key = (((v + BK_THREADS - 1) / BK_THREADS + (nbk > 1 ? 3 : 0)) << 32) | nbk;
                if (!found || key < best_v) {
                    found = true;
                    best_v = key;
                    p.nbx = nx;
                    p.nby = ny;
                    p.nbz = nz;
                    p.vmax = (uint32_t)v;
                    p.fmax = (uint32_t)f;
                    p.lds = (uint32_t)lds;
                }
            }
    return found;
}

}  // namespace gp
