// gp_kernel_plan.hpp -- which round kernel a run gets: kernel variant, tile walk, grid, size class,
// whether rounds run region by region, and with the kernel the form in which its messages cross
// ranks (kernel_plan), decided from the run's shape, a handful of
// integers the device and the compiled kernels report (KernelFacts, gathered by
// gather_kernel_facts) and the experiments build's overrides (KernelOverrides, read once at create
// by read_overrides, gp_setup.hip).  The rules are measured defaults; the position of each
// override between them is part of the plan.  Host-only and free of HIP headers, like gp_plan.hpp
// and gp_block_plan.hpp: tests/helpers/plan_check.cpp evaluates it on the CPU, and
// tests/test_plan.py replays recorded decisions against it (tests/golden/kernel_plan.json).
#pragma once

#include <cerrno>
#include <cstdlib>
#include <optional>
#include <string>

#include "gp_block_plan.hpp"
#include "gp_plan.hpp"

namespace gp {

enum KernelVariant : int { KERNEL_TILE = 1, KERNEL_COL = 2, KERNEL_BLOCK = 3 };
enum Mode : int { MODE_SINGLE = 0, MODE_VIRTUAL = 1, MODE_RCCL = 2 };
constexpr int BULK_THREADS = 256;  // threads of a workgroup of the column and set-up kernels

// What is run: values as in the C ABI (gossip_hip.h) and in gp_device.hpp's enums.
struct RunShape {
    enum : int { Line = 0, Full = 1, Grid3D = 2, Imp3D = 3 };
    enum : int { Gossip = 0, PushSum = 1 };
    int topology = Line, algorithm = Gossip;
    int64_t g = 0;
    int world = 1;
    int mode = MODE_SINGLE;
    std::vector<uint32_t> bounds;  // world + 1 slab boundaries (slab_bounds)

    bool lattice() const { return topology == Grid3D || topology == Imp3D; }
    bool push() const { return algorithm == PushSum; }
    int64_t nloc_max() const {
        int64_t n = 0;
        for (int w = 0; w < world; ++w) n = std::max<int64_t>(n, bounds[w + 1] - bounds[w]);
        return n;
    }
    // the push-sum tile kernel's instantiation whose occupancy the rules ask for
    int tile_topo() const { return topology == Line ? Line : topology == Grid3D ? Grid3D : Imp3D; }
    bool tile_remote() const { return world > 1 && tile_topo() == Imp3D; }
};

// What the rules need from the device and the compiled kernels; a query the run's path does not
// make leaves its field 0 (gather_kernel_facts).
struct KernelFacts {
    int cus = 0;                  // compute units (hipDeviceProp_t::multiProcessorCount)
    int col_blocks_per_cu = 0;    // the column kernel's occupancy
    int res4 = 0;                 // resident blocks of the 4-nodes-per-thread push-sum tile kernel (tile_topo, tile_remote)
    int res_wide = 0;             // ... of the wide class
    bool block_resident = false;  // the box grid block_plan(g, cus) gives is co-resident
};

// The experiments build's overrides, parsed; an empty field: not set.
struct KernelOverrides {
    std::optional<int> kernel;         // GP_KERNEL: a KernelVariant, 0 for any other text (selects nothing)
    std::optional<uint32_t> xsegs;     // GP_XSEGS
    std::optional<uint32_t> walk, wx;  // GP_WALK, GP_WX
    std::optional<bool> wide;          // GP_WIDE
    std::optional<int> rregions;       // GP_RREGIONS
    std::optional<int> xregions;       // GP_XREGIONS (only 8 counts)
    std::optional<uint32_t> fuse;      // GP_FUSE
    std::optional<uint32_t> stage_cap; // GP_STAGE_CAP
    std::optional<bool> no_full;       // GP_NO_FULLTILE
    std::optional<std::string> grid;   // GP_GRID, its text
};

struct KernelPlan {
    int kernel = KERNEL_TILE;
    XKind xkind = XKind::None;   // the exchange across ranks (exchange_kind)
    uint32_t col_xsegs = 1;
    uint32_t walk = 0, wx = 8, wide = 0;
    int grid = 1;
    uint32_t rregions = 1;       // round kernel launches per round (DevState::rregions)
    int xregions = 1;            // exchange regions of a slab's senders (exchange_regions)
    uint32_t fuse_finalize = 0;
    uint32_t stage_cap = 0xFFFFFFFFu;
    uint32_t no_full = 0;
    BlockPlan bplan{};
    bool grid_override = false;  // a GP_GRID was present on a tiled lattice / line kernel (the name's @grid suffix)
};

// GP_GRID: not a grid of 1..grid_max blocks.
struct KernelPlanError {
    bool bad_grid = false;
    int grid_max = 0;
};

// Exchange regions of this run's slabs (gp_plan.hpp).  GP_XREGIONS=8 (experiments): the eight
// regions of two ranks with large slabs at any slab size and world, Imp3D push-sum only; any
// other value is ignored.
inline int exchange_regions(const RunShape& r, const KernelOverrides& ov) {
    const bool imp3d = r.topology == RunShape::Imp3D;
    if (ov.xregions && r.push() && imp3d && r.world > 1 && *ov.xregions == 8) return 8;
    return exchange_regions(r.push(), imp3d, r.world, r.bounds);
}

// Round kernel launches per round (DevState::rregions).  Imp3D push-sum across ranks runs the
// round kernel region by region (launch_round_regions): region h's lists are packed and travel
// while the later regions compute.  C5 modelled from virtual ranks, same box, against one launch
// per round with the lists packed and sent after it (profiles/r05/rregions/): W = 2 12.92 ->
// 10.50 ms at 128 GB/s per link and direction, 17.97 -> 12.48 at 64; W = 4 5.46 -> 5.48 and
// 6.76 -> 5.81; W = 8 2.75 -> 2.74 and 2.96 -> 2.83 (the round kernel itself +2-5 %: four launch
// tails).  Small slabs (< RREG_MIN_NODES) move little and keep one launch per round: their rounds
// are launch-bound, and rank processes sharing one GPU (the tests) run them several times slower
// with four persistent launches per round.  The experiments build's GP_RREGIONS=0/1 overrides.
inline uint32_t round_regions(const RunShape& r, const KernelOverrides& ov, int kernel, uint32_t walk) {
    if (r.world < 2 || r.topology != RunShape::Imp3D || !r.push() || kernel != KERNEL_TILE || walk != 3) return 1;
    int on = round_regions_on(r.world, r.bounds) ? 1 : 0;
    if (ov.rregions) on = *ov.rregions;
    const int NH = exchange_regions(r, ov);
    return on && round_regions_fit(r.world, r.bounds, (uint64_t)r.g * r.g, NH) ? (uint32_t)NH : 1u;
}

// ---- the first steps of the plan, which also decide what is asked of the device
// 3D push-sum on one rank whose lattice fits the chip's LDS (C2: g = 100): one cooperative
// launch per batch, the state resident in LDS (gp_block.hip) -- if a box grid exists (and, the
// device's answer, is co-resident: KernelFacts::block_resident)
inline bool block_plan_wanted(const RunShape& r, int cus, BlockPlan& bp) {
    return r.topology == RunShape::Grid3D && r.push() && r.world == 1 && r.g >= 2 && block_plan((uint32_t)r.g, cus, bp);
}

inline int plan_variant(const RunShape& r, bool block_ok, const KernelOverrides& ov) {
    // (measured: gossip on a large lattice -> column march, profiles/r01; push-sum and
    // small lattices and line -> tiled; the push-sum column march was measured slower,
    // profiles/r03 and DESIGN.md §5.1)
    int kernel = KERNEL_TILE;
    if (r.lattice() && r.g >= 200 && !r.push()) kernel = KERNEL_COL;
    if (block_ok) kernel = KERNEL_BLOCK;
    if (ov.kernel) {
        if (*ov.kernel == KERNEL_TILE) kernel = KERNEL_TILE;
        else if (*ov.kernel == KERNEL_COL && r.lattice() && !r.push()) kernel = KERNEL_COL;
        else if (*ov.kernel == KERNEL_BLOCK && block_ok) kernel = KERNEL_BLOCK;
    }
    return kernel;
}

// How this run's random-edge / full-topology messages cross ranks (XKind, gp_plan.hpp).  kernel:
// plan_variant's answer, overrides applied -- the gossip column kernel sets bits itself, the tile
// kernel reads in-edge tags.
inline XKind exchange_kind(const RunShape& r, int kernel) {
    if (r.world < 2) return XKind::None;
    if (r.topology == RunShape::Imp3D)
        return r.push() ? XKind::Lists : kernel == KERNEL_COL ? XKind::Bits : XKind::Slots;
    if (r.topology == RunShape::Full) return r.push() ? XKind::FullBins : XKind::Slots;
    return XKind::None;  // line / 3D: halo planes only
}

// The walk and its x-window, before walk 3 has been checked against the resident grid.
inline void plan_walk(const RunShape& r, int kernel, const KernelOverrides& ov, uint32_t& walk, uint32_t& wx) {
    // tile walk: x-windows of 8 planes once every XCD gets a few windows (measured,
    // profiles/r01: 18.2 -> 17.2 ms/round at P = 1e9), else XCD-contiguous eighths
    walk = (r.lattice() && r.g / r.world >= 64) ? 2u : 0u;
    // push-sum: the same x-windows claimed from per-XCD counters on exactly the
    // resident grid (walk 3; measured, profiles/r02/walk3.txt)
    if (walk == 2 && kernel == KERNEL_TILE && r.push()) walk = 3;
    // x-window of 8 planes (walk 2); 16 for walk 3 since round 4, where the wave priority
    // of the tile kernel moved the optimum: P = 1e9, same box, 8 / 12 / 16 / 24 / 32 planes
    // 13.34-13.36 / 13.17-13.28 / 13.17-13.22 / 13.22-13.25 / 13.15-13.17 ms/round
    // (profiles/r04/walk_window_nt.txt)
    wx = walk == 3 ? 16 : 8;
    if (ov.walk) walk = *ov.walk;
    if (ov.wx) wx = *ov.wx;
}

// size class of the tiled kernels: line / 3D push-sum on a slab with at most two tiles per
// resident block of the 4-nodes-per-thread kernel (~2500 tiles, P <~ 2.6e6 per slab) runs the
// 1024-thread, one-node-per-thread build (gp_ps_tile_wide.hip): its node phase is one memory
// round trip per tile instead of four, which is what bounds a round with few tiles per block
// (C2, 3D push-sum P = 1e6: 26.5 -> 20.7 us per round; line push-sum n = 1000: 10.2 -> 8.8).
// Imp3D push-sum (its in-edge pass spills at 8 waves) and the gossip tile kernel measured
// slower in that build at every size (profiles/r04/tile_size_class.txt)
inline bool size_class_applies(const RunShape& r, int kernel) {
    return kernel == KERNEL_TILE && r.push() && r.topology != RunShape::Imp3D;
}
inline uint32_t plan_wide(const RunShape& r, int kernel, int res4, const KernelOverrides& ov) {
    if (!size_class_applies(r, kernel)) return 0;
    const int64_t tiles = (r.nloc_max() + 1023) / 1024 + 1;
    uint32_t wide = res4 > 0 && tiles <= 2 * (int64_t)res4 ? 1u : 0u;
    if (ov.wide) wide = *ov.wide ? 1u : 0u;
    return wide;
}

// The facts of a run, asking `q` (cus(), block_resident(bp, cus), col_blocks_per_cu(), res4(),
// res_wide()) only for what the run's path through the rules reads: the box grid's residency only
// where a box grid exists, the column kernel's occupancy only for the column kernel, the tile
// kernels' only for the size class and for walk 3.
template <typename Q>
KernelFacts gather_kernel_facts(const RunShape& r, const KernelOverrides& ov, Q&& q) {
    KernelFacts f;
    f.cus = q.cus();
    BlockPlan bp{};
    f.block_resident = block_plan_wanted(r, f.cus, bp) && q.block_resident(bp, f.cus);
    const int kernel = plan_variant(r, f.block_resident, ov);
    if (r.topology != RunShape::Full && kernel == KERNEL_COL) f.col_blocks_per_cu = q.col_blocks_per_cu();
    uint32_t walk, wx;
    plan_walk(r, kernel, ov, walk, wx);
    if (size_class_applies(r, kernel) || walk == 3) f.res4 = q.res4();
    if (walk == 3 && plan_wide(r, kernel, f.res4, ov)) f.res_wide = q.res_wide();
    return f;
}

// Kernel variant and grid for this run (measured defaults; GP_KERNEL / GP_XSEGS / GP_WALK /
// GP_WX / GP_WIDE / GP_GRID override them in the experiments build).  err.bad_grid: a GP_GRID the
// run cannot take.
inline KernelPlan kernel_plan(const RunShape& r, const KernelFacts& f, const KernelOverrides& ov, KernelPlanError& err) {
    KernelPlan p;
    err = KernelPlanError{};
    const int64_t g = r.g, nloc_max = r.nloc_max();
    int64_t blocks = (nloc_max + BULK_THREADS - 1) / BULK_THREADS;
    // 64 workgroups per CU: measured best for the tiled round kernels (tools/ablate.py:
    // 2048 -> 27.5, 8192 -> 22.1, 16384 -> 21.2 ms/round at P = 1e9)
    int64_t cap = (int64_t)f.cus * 64;
    const bool block_ok = block_plan_wanted(r, f.cus, p.bplan) && f.block_resident;
    p.kernel = plan_variant(r, block_ok, ov);
    p.xkind = exchange_kind(r, p.kernel);
    if (r.topology != RunShape::Full && p.kernel == KERNEL_COL) {
        // gossip: exactly the resident grid (a persistent sweep), a multiple of the 8 XCDs
        cap = (int64_t)f.cus * f.col_blocks_per_cu;
        // x segments per patch: enough work items for every resident wave, >= 16 planes each
        const int64_t patches = ((g + 63) / 64) * ((g + 3) / 4);
        const int64_t slots = cap * (BULK_THREADS / 64);
        const int64_t planes = std::max<int64_t>(1, g / r.world);
        int64_t xs = std::max<int64_t>(1, slots / std::max<int64_t>(1, patches));
        xs = std::min<int64_t>(xs, std::max<int64_t>(1, planes / 16));
        p.col_xsegs = (uint32_t)xs;
    }
    if (p.kernel == KERNEL_TILE)  // 1024-node tiles (+1: a slab may start mid-tile), a multiple of the 8 XCDs
        blocks = ((nloc_max + 1023) / 1024 + 1 + 7) / 8 * 8;
    if (ov.xsegs) p.col_xsegs = *ov.xsegs;
    p.grid = (int)std::max<int64_t>(1, std::min(p.kernel == KERNEL_COL ? cap : blocks, cap));
    plan_walk(r, p.kernel, ov, p.walk, p.wx);
    p.wide = plan_wide(r, p.kernel, f.res4, ov);
    if (p.walk == 3) {  // exactly the resident grid, a multiple of the 8 XCDs; without eight resident blocks: walk 2
        const int64_t res = (p.wide ? f.res_wide : f.res4) / 8 * 8;
        if (res >= 8) p.grid = (int)std::min<int64_t>(p.grid, res);
        else p.walk = 2;
    }
    p.rregions = round_regions(r, ov, p.kernel, p.walk);
    // GP_GRID (experiments; tests/test_gpu_tile_sequence.py): fewer blocks for the tiled round
    // kernels than the rule above gives, so that a block walks several tiles of a small slab and
    // carries its prefetches, its claims and its LDS from one tile to the next -- which the rule
    // allows only from ~1.7e7 nodes on.  It only lowers the grid: everything else launched with
    // it (k_init, k_rbits_init, the set-up, pack, injector and recount kernels) strides over its
    // range by the grid, and the round kernels' walks and round close take any grid.  A value
    // that is no number, below 1 or above the grid chosen is an error, so a test cannot run the
    // default grid unnoticed; region rounds take multiples of 8 only (launch_round_tile_region)
    // and ignore any other value.
    if (ov.grid && p.kernel == KERNEL_TILE && r.topology != RunShape::Full) {
        p.grid_override = true;
        const char* e = ov.grid->c_str();
        char* end = nullptr;
        errno = 0;
        const long v = std::strtol(e, &end, 10);
        if (errno || end == e || *end != '\0' || v < 1 || v > (long)p.grid) {
            err.bad_grid = true;
            err.grid_max = p.grid;
            return p;
        }
        if (p.rregions <= 1 || v % 8 == 0) p.grid = (int)v;
    }
    p.xregions = exchange_regions(r, ov);
    // single-rank lattice push-sum: the round kernel's last block closes the
    // round (no injector, nothing to exchange), saving a k_finalize launch per round
    // (2: arrivals sharded over 8 counters; a single counter -- 1, experiments
    // only -- serialises ~16k returning atomics per round: measured 1.93 vs
    // 0.40 ms/round at P = 2.7e7, profiles/r02/round_close.txt)
    p.fuse_finalize = (r.mode == MODE_SINGLE && r.push() && r.topology != RunShape::Full) ? 2u : 0u;
    if (ov.fuse) p.fuse_finalize = p.fuse_finalize ? *ov.fuse : 0u;
    if (ov.stage_cap) p.stage_cap = *ov.stage_cap;
    if (ov.no_full) p.no_full = *ov.no_full ? 1u : 0u;
    return p;
}

}  // namespace gp
