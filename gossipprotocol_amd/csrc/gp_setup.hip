// gp_setup.hip -- everything a simulation needs before round 0 (create_common / build_sim): the
// slab plan and kernel choice, every slab's device state and the halo buffers; then the Imp3D
// topology build (gp_topology.hip) and the exchange buffers (gp_xlayout.hip).  The plan's
// arithmetic is gp_plan.hpp.
#include "gp_host.hpp"

namespace {

// Slab boundaries and halo width (slab_bounds, gp_plan.hpp).
int make_bounds(gp_sim* s) {
    const int W = s->world;
    const int topo = s->cfg.topology;
    const SlabCut cut = topo == GP_FULL ? SlabCut::Full : topo == GP_LINE ? SlabCut::Line : SlabCut::Planes;
    switch (slab_bounds(s->P, s->g, W, cut, s->bounds, s->halo)) {
    case BoundsError::None:
        return GP_OK;
    case BoundsError::TooManyRanks:
        set_err("at most %d ranks are supported (got %d)", XMAXW, W);
        break;
    case BoundsError::FewerNodesThanRanks:
        if (topo == GP_FULL) set_err("full topology with %lld nodes cannot be split over %d ranks", (long long)s->P, W);
        else set_err("line with %lld nodes cannot be split over %d ranks", (long long)s->P, W);
        break;
    case BoundsError::FewerPlanesThanRanks:
        set_err("a %lld^3 lattice has fewer planes than ranks (%d)", (long long)s->g, W);
        break;
    }
    return GP_EINVAL;
}

// Device state of slab `r` (rank r): ids [bounds[r], bounds[r+1]) plus halos.
int alloc_slab(gp_sim* s, Slab& sl, int r) {
    DevState& S = sl.S;
    const int W = s->world;
    sl.rank = r;
    const uint32_t lo = s->bounds[r], hi = s->bounds[r + 1];
    sl.hi = hi;
    S.topo = s->cfg.topology;
    S.alg = s->cfg.algorithm;
    S.G.P = (uint32_t)s->P;
    S.G.T = (uint32_t)s->T;
    S.G.g = (uint32_t)s->g;
    S.G.g2 = (uint32_t)(s->g * s->g);
    S.G.div_g = make_fastdiv(S.G.g ? S.G.g : 1);
    S.G.div_g2 = make_fastdiv(S.G.g2 ? S.G.g2 : 1);
    S.k0 = (uint32_t)s->cfg.seed;
    S.k1 = (uint32_t)(s->cfg.seed >> 32);
    // choice = Random().Next(0, nodes) (Program.fs:193,221,263)
    S.seed_node = uniform(S.k0, S.k1, S_START, 0, 0, (uint32_t)s->T);
    S.lo = lo;
    S.nloc = hi - lo;
    S.ext_lo = r > 0 ? lo - s->halo : lo;
    S.ext_hi = r < W - 1 ? hi + s->halo : hi;
    S.base = S.ext_lo & ~3u;  // 4-aligned: the tile kernels move node bytes as words
    S.rtag = nullptr;
    S.rmsg = nullptr;
    S.rk = nullptr;
    S.rtg = nullptr;
    S.sbits = nullptr;
    S.xhdr[0] = S.xhdr[1] = nullptr;
    S.xvals[0] = S.xvals[1] = nullptr;
    S.xnv = 0;
    int rc;
    const size_t next = (size_t)(S.ext_hi - S.base) + 1024;  // node arrays (+ word-I/O padding)
    const size_t nl = S.nloc;
    if ((rc = dev_alloc_t(s, &S.ctl, 1))) return rc;
    if ((rc = dev_alloc_t(s, &S.tq, 2 * 8 * TQ_STRIDE))) return rc;
    HIP_TRY(hipMemsetAsync(S.tq, 0, sizeof(uint32_t) * 2 * 8 * TQ_STRIDE, s->stream));
    if (S.alg == PUSHSUM) {
        if ((rc = dev_alloc_t(s, &S.sw[0], next)) || (rc = dev_alloc_t(s, &S.sw[1], next)) ||
            (rc = dev_alloc_t(s, &S.nb[0], next)))
            return rc;
        if (S.topo != FULL && (rc = dev_alloc_t(s, &S.nb[1], next))) return rc;
        // zero sentinel just past the ids the slab holds: the tile kernels gather it for
        // lattice directions without a sender (never written by any round)
        for (int bb = 0; bb < 2; ++bb)
            HIP_TRY(hipMemsetAsync(S.sw[bb] + (S.ext_hi - S.base), 0, sizeof(double2), s->stream));
    } else {
        if ((rc = dev_alloc_t(s, &S.c, nl))) return rc;
        if (S.topo == FULL) {
            if ((rc = dev_alloc_t(s, &S.inc, nl))) return rc;
        } else {
            if ((rc = dev_alloc_t(s, &S.nb[0], next)) || (rc = dev_alloc_t(s, &S.nb[1], next))) return rc;
            S.nchunks = (uint32_t)((s->T + INJ_CHUNK - 1) / INJ_CHUNK);
            if ((rc = dev_alloc_t(s, &S.live_bits, (size_t)S.nchunks * (INJ_CHUNK / 32))) ||
                (rc = dev_alloc_t(s, &S.chunk_live, S.nchunks)))
                return rc;
        }
    }
    if (S.topo == FULL && S.alg == PUSHSUM) {  // LDS-binned message staging of this rank's receivers (gp_fullbin.hip)
        const FullBinPlan fp = full_bin_plan(S.nloc, W == 1);
        S.fb_nb2 = fp.nb2;
        S.fb_cap2 = fp.cap2;
        // (GP_FB_CAP2 / GP_FB_CAP1, experiments: smaller bins, to put a round's fullest fine tile /
        // coarse bin exactly at and one past its capacity; tests/test_gpu_fullbin_edges.py)
        if (const char* e = exp_env("GP_FB_CAP2")) S.fb_cap2 = std::min<uint32_t>(FB_CAP2, (uint32_t)std::max(1, std::atoi(e)));
        const size_t m2 = (size_t)fp.nb2 * S.fb_cap2;
        if ((rc = dev_alloc_t(s, &S.fb_cnt2, fp.nb2)) || (rc = dev_alloc_t(s, &S.fb_hdr2, m2)) ||
            (rc = dev_alloc_t(s, &S.fb_pay2, m2)))
            return rc;
        if (W == 1) {
            // one rank: coarse bins hdr1 / pay1; the fold of round r bins round r+1's messages
            // into them (k_fb_fold<FOLD_SEND>; GP_FB_FUSED=0, experiments: three passes)
            bool fused = true;
            if (const char* e = exp_env("GP_FB_FUSED")) fused = e[0] == '1';
            const FullBinPlan f1 = full_bin_plan(S.nloc, fused);
            S.fb_s1 = f1.s1;
            S.fb_nb1 = f1.nb1;
            S.fb_cap1 = f1.cap1;
            if (const char* e = exp_env("GP_FB_CAP1")) S.fb_cap1 = std::min<uint32_t>(f1.cap1, (uint32_t)std::max(1, std::atoi(e)));
            S.fb_fused = fused && f1.nb1 <= full_bin_fused_max_bins() ? 1u : 0u;
            const size_t m1 = (size_t)f1.nb1 * S.fb_cap1;
            // (+ FB_JUNK: the fold's write-out sends lanes without a message to the slots past the
            // last bin, so every thread issues the same number of stores)
            if ((rc = dev_alloc_t(s, &S.fb_cnt1, f1.nb1)) || (rc = dev_alloc_t(s, &S.fb_hdr1, m1 + FB_JUNK)) ||
                (rc = dev_alloc_t(s, &S.fb_pay1, m1 + FB_JUNK)))
                return rc;
        } else {
            // several ranks (round 6): the coarse bins are the exchange buffers (setup_exchange) --
            // the fold bins the next round's messages by destination rank and coarse bin into them,
            // and each rank's split reads them where they arrive (k_fb_fold<FOLD_SEND_RANKS>)
            S.fb_s1 = full_bin_multi_s1(s->bounds.data(), W);
            S.fb_nb1 = full_coarse_bins(s->bounds, r, S.fb_s1);
            S.fb_cap1 = 0;
            S.fb_fused = 1;
            S.fb_cnt1 = S.fb_hdr1 = nullptr;
            S.fb_pay1 = nullptr;
        }
    }
    if (col_gossip_counts(S)) {  // senders count their random-edge deliveries at the target (k_gossip_col)
        // byte counters, four per word (C3: 0.632 -> 0.600 ms per round, reads 16.5 -> 11.7 and
        // writes 11.2 -> 9.8 B/node; profiles/r04/c3_byte_counters.txt)
        S.rq8 = 1;
        if (const char* e = exp_env("GP_RQ8")) S.rq8 = e[0] == '1' ? 1u : 0u;
        for (int q = 0; q < 2; ++q) {
            if ((rc = dev_alloc_t(s, &S.rq[q], (size_t)S.nloc + 64))) return rc;
            HIP_TRY(hipMemsetAsync(S.rq[q], 0, sizeof(uint32_t) * ((size_t)S.nloc + 64), s->stream));
        }
    }
    // random-edge bitmaps of the tile kernels (the column kernel counts deliveries instead)
    if (S.topo == IMP3D && !col_gossip_counts(S)) {
        S.rbits_words = rbits_words_for(S.lo, S.nloc);
        if ((rc = dev_alloc_t(s, &S.rbits[0], S.rbits_words)) || (rc = dev_alloc_t(s, &S.rbits[1], S.rbits_words)))
            return rc;
    }
    return GP_OK;
}

// Push-sum on a 3D / Imp3D lattice over several ranks: the halo planes' (s, w) travel compacted
// (only the senders toward the neighbour, HaloArgs in gp_xchg.hpp): C5 at W = 8, 16 MB -> 3.9 MB
// per direction and round.
int setup_halo(gp_sim* s) {
    s->halo_slots = 0;
    const bool lattice = s->cfg.topology == GP_3D || s->cfg.topology == GP_IMP3D;
    if (!lattice || s->cfg.algorithm != GP_PUSHSUM || s->world < 2 || s->halo < HALO_CHUNK) return GP_OK;
    s->halo_cap = halo_chunk_cap((uint32_t)s->g, s->cfg.topology == GP_IMP3D);
    // (GP_HALO_CAP, experiments: fewer slots per chunk, to put a round's fullest chunk at the last
    // slot or one past it -- never more than the plan's)
    if (const char* e = exp_env("GP_HALO_CAP")) s->halo_cap = std::min<uint32_t>(s->halo_cap, (uint32_t)std::max(1, std::atoi(e)));
    s->halo_slots = halo_buf_slots(s->halo, s->halo_cap);
    int rc;
    for (Slab& sl : s->slab) {
        for (int k = 0; k < 2; ++k) {
            const bool has = k == 0 ? sl.rank > 0 : sl.rank < s->world - 1;
            if (!has) continue;
            if ((rc = dev_alloc_t(s, &sl.hsend[k], s->halo_slots)) || (rc = dev_alloc_t(s, &sl.hrecv[k], s->halo_slots)))
                return rc;
        }
    }
    return GP_OK;
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
uint32_t round_regions(const gp_sim* s, int kernel, uint32_t walk) {
    if (s->world < 2 || s->cfg.topology != GP_IMP3D || s->cfg.algorithm != GP_PUSHSUM || kernel != KERNEL_TILE ||
        walk != 3)
        return 1;
    int on = round_regions_on(s->world, s->bounds) ? 1 : 0;
    if (const char* e = exp_env("GP_RREGIONS")) on = std::atoi(e);
    const int NH = exchange_regions(s);
    return on && round_regions_fit(s->world, s->bounds, (uint64_t)s->g * s->g, NH) ? (uint32_t)NH : 1u;
}

// Kernel variant and grid for this run (measured defaults; GP_KERNEL / GP_XSEGS / GP_WALK /
// GP_WX / GP_WIDE / GP_GRID override them in the experiments build).  GP_EINVAL: a GP_GRID the
// run cannot take.
int choose_kernel(gp_sim* s, int64_t nloc_max, int& kernel, uint32_t& col_xsegs, uint32_t& walk, uint32_t& wx,
                   uint32_t& wide) {
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, s->device);
    s->cus = std::max(1, prop.multiProcessorCount);
    const gp_config* cfg = &s->cfg;
    const int64_t g = s->g;
    int64_t blocks = (nloc_max + BULK_THREADS - 1) / BULK_THREADS;
    // 64 workgroups per CU: measured best for the tiled round kernels (tools/ablate.py:
    // 2048 -> 27.5, 8192 -> 22.1, 16384 -> 21.2 ms/round at P = 1e9)
    int64_t cap = (int64_t)prop.multiProcessorCount * 64;
    // (measured: gossip on a large lattice -> column march, profiles/r01; push-sum and
    // small lattices and line -> tiled; the push-sum column march was measured slower,
    // profiles/r03 and DESIGN.md §5.1)
    kernel = KERNEL_TILE;
    const bool lattice = cfg->topology == GP_3D || cfg->topology == GP_IMP3D;
    const bool push = cfg->algorithm == GP_PUSHSUM;
    if (lattice && g >= 200 && !push) kernel = KERNEL_COL;
    // 3D push-sum on one rank whose lattice fits the chip's LDS (C2: g = 100): one cooperative
    // launch per batch, the state resident in LDS (gp_block.hip)
    BlockPlan bp{};
    const bool block_ok = cfg->topology == GP_3D && push && s->world == 1 && g >= 2 &&
                          block_plan((uint32_t)g, prop.multiProcessorCount, bp) &&
                          block_plan_resident(bp, prop.multiProcessorCount);
    if (block_ok) kernel = KERNEL_BLOCK;
    if (const char* e = exp_env("GP_KERNEL")) {
        if (!std::strcmp(e, "tile")) kernel = KERNEL_TILE;
        else if (!std::strcmp(e, "col") && lattice && !push) kernel = KERNEL_COL;
        else if (!std::strcmp(e, "block") && block_ok) kernel = KERNEL_BLOCK;
    }
    s->bplan = bp;
    col_xsegs = 1;
    if (cfg->topology != GP_FULL && kernel == KERNEL_COL) {
        // gossip: exactly the resident grid (a persistent sweep), a multiple of the 8 XCDs
        cap = (int64_t)prop.multiProcessorCount * col_blocks_per_cu(cfg->topology, cfg->algorithm);
        // x segments per patch: enough work items for every resident wave, >= 16 planes each
        const int64_t patches = ((g + 63) / 64) * ((g + 3) / 4);
        const int64_t slots = cap * (BULK_THREADS / 64);
        const int64_t planes = std::max<int64_t>(1, g / s->world);
        int64_t xs = std::max<int64_t>(1, slots / std::max<int64_t>(1, patches));
        xs = std::min<int64_t>(xs, std::max<int64_t>(1, planes / 16));
        col_xsegs = (uint32_t)xs;
    }
    if (kernel == KERNEL_TILE)  // 1024-node tiles (+1: a slab may start mid-tile), a multiple of the 8 XCDs
        blocks = ((nloc_max + 1023) / 1024 + 1 + 7) / 8 * 8;
    if (const char* e = exp_env("GP_XSEGS")) col_xsegs = (uint32_t)std::max(1, std::atoi(e));
    s->grid = (int)std::max<int64_t>(1, std::min(kernel == KERNEL_COL ? cap : blocks, cap));
    // tile walk: x-windows of 8 planes once every XCD gets a few windows (measured,
    // profiles/r01: 18.2 -> 17.2 ms/round at P = 1e9), else XCD-contiguous eighths
    walk = (lattice && g / s->world >= 64) ? 2u : 0u;
    // push-sum: the same x-windows claimed from per-XCD counters on exactly the
    // resident grid (walk 3; measured, profiles/r02/walk3.txt)
    if (walk == 2 && kernel == KERNEL_TILE && cfg->algorithm == GP_PUSHSUM) walk = 3;
    // x-window of 8 planes (walk 2); 16 for walk 3 since round 4, where the wave priority
    // of the tile kernel moved the optimum: P = 1e9, same box, 8 / 12 / 16 / 24 / 32 planes
    // 13.34-13.36 / 13.17-13.28 / 13.17-13.22 / 13.22-13.25 / 13.15-13.17 ms/round
    // (profiles/r04/walk_window_nt.txt)
    wx = walk == 3 ? 16 : 8;
    if (const char* e = exp_env("GP_WALK")) walk = (uint32_t)std::atoi(e);
    if (const char* e = exp_env("GP_WX")) wx = (uint32_t)std::max(1, std::atoi(e));
    // size class of the tiled kernels: line / 3D push-sum on a slab with at most two tiles per
    // resident block of the 4-nodes-per-thread kernel (~2500 tiles, P <~ 2.6e6 per slab) runs the
    // 1024-thread, one-node-per-thread build (gp_ps_tile_wide.hip): its node phase is one memory
    // round trip per tile instead of four, which is what bounds a round with few tiles per block
    // (C2, 3D push-sum P = 1e6: 26.5 -> 20.7 us per round; line push-sum n = 1000: 10.2 -> 8.8).
    // Imp3D push-sum (its in-edge pass spills at 8 waves) and the gossip tile kernel measured
    // slower in that build at every size (profiles/r04/tile_size_class.txt)
    wide = 0;
    if (kernel == KERNEL_TILE && push && cfg->topology != GP_IMP3D) {
        const int topo = cfg->topology == GP_LINE ? LINE : cfg->topology == GP_3D ? GRID3D : IMP3D;
        const int64_t tiles = (nloc_max + 1023) / 1024 + 1;
        const int64_t res4 = ps_tile_resident_blocks(topo, s->world > 1 && topo == IMP3D, s->device);
        wide = res4 > 0 && tiles <= 2 * res4 ? 1u : 0u;
        if (const char* e = exp_env("GP_WIDE")) wide = e[0] == '1' ? 1u : 0u;
    }
    if (walk == 3) {
        const int topo = cfg->topology == GP_LINE ? LINE : cfg->topology == GP_3D ? GRID3D : IMP3D;
        const bool rem = s->world > 1 && topo == IMP3D;
        const int64_t res = (wide ? wide::ps_tile_resident_blocks(topo, rem, s->device)
                                  : ps_tile_resident_blocks(topo, rem, s->device)) / 8 * 8;
        if (res >= 8) s->grid = (int)std::min<int64_t>(s->grid, res);
        else walk = 2;
    }
    // GP_GRID (experiments; tests/test_gpu_tile_sequence.py): fewer blocks for the tiled round
    // kernels than the rule above gives, so that a block walks several tiles of a small slab and
    // carries its prefetches, its claims and its LDS from one tile to the next -- which the rule
    // allows only from ~1.7e7 nodes on.  It only lowers the grid: everything else launched with
    // it (k_init, k_rbits_init, the set-up, pack, injector and recount kernels) strides over its
    // range by the grid, and the round kernels' walks and round close take any grid.  A value
    // that is no number, below 1 or above the grid chosen is an error, so a test cannot run the
    // default grid unnoticed; region rounds take multiples of 8 only (launch_round_tile_region)
    // and ignore any other value.
    if (const char* e = exp_env("GP_GRID")) {
        if (kernel == KERNEL_TILE && cfg->topology != GP_FULL) {
            char* end = nullptr;
            errno = 0;
            const long v = std::strtol(e, &end, 10);
            if (errno || end == e || *end != '\0' || v < 1 || v > (long)s->grid) {
                set_err("GP_GRID=%s: not a grid of 1..%d blocks", e, s->grid);
                return GP_EINVAL;
            }
            if (round_regions(s, kernel, walk) <= 1 || v % 8 == 0) s->grid = (int)v;
        }
    }
    return GP_OK;
}

// Everything after the handle exists: slabs, topology, initial state, round 0.
int build_sim(gp_sim* s) {
    int rc;
    if ((rc = make_bounds(s))) return rc;
    int64_t nloc_max = 0;
    for (int w = 0; w < s->world; ++w) nloc_max = std::max<int64_t>(nloc_max, s->bounds[w + 1] - s->bounds[w]);
    int kernel;
    uint32_t col_xsegs, walk, wx, wide;
    if ((rc = choose_kernel(s, nloc_max, kernel, col_xsegs, walk, wx, wide))) return rc;
    const uint32_t rreg = round_regions(s, kernel, walk);
    if (s->mode == MODE_VIRTUAL) {
        s->slab.resize(s->world);
        for (int w = 0; w < s->world; ++w) s->slab[w].rank = w;
    } else {
        s->slab.resize(1);
        s->slab[0].rank = s->rank;
    }
    for (Slab& sl : s->slab) {
        sl.S.kernel = kernel;
        sl.S.tile_wide = wide;
        sl.S.col_xsegs = col_xsegs;
        sl.S.tile_walk = walk;
        sl.S.tile_wx = wx;
        sl.S.tile_stage_cap = 0xFFFFFFFFu;
        // single-rank lattice push-sum: the round kernel's last block closes the
        // round (no injector, nothing to exchange), saving a k_finalize launch per round
        // (2: arrivals sharded over 8 counters; a single counter -- 1, experiments
        // only -- serialises ~16k returning atomics per round: measured 1.93 vs
        // 0.40 ms/round at P = 2.7e7, profiles/r02/round_close.txt)
        sl.S.fuse_finalize = (s->mode == MODE_SINGLE && s->cfg.algorithm == GP_PUSHSUM &&
                              s->cfg.topology != GP_FULL) ? 2u : 0u;
        sl.S.bplan = s->bplan;
        sl.S.bface = sl.S.bscratch = nullptr;
        if (kernel == KERNEL_BLOCK) {  // face exchange buffers + barrier / accumulator scratch
            if ((rc = dev_alloc(s, &sl.S.bface, block_face_bytes(s->bplan))) || (rc = dev_alloc(s, &sl.S.bscratch, BLOCK_SCRATCH_BYTES)))
                return rc;
            HIP_TRY(block_kernel_setup(s->bplan));
        }
        if (const char* e = exp_env("GP_FUSE")) sl.S.fuse_finalize = sl.S.fuse_finalize ? (uint32_t)(e[0] - '0') : 0u;
        if (const char* e = exp_env("GP_STAGE_CAP")) sl.S.tile_stage_cap = (uint32_t)std::max(0, std::atoi(e));
#ifdef GP_EXPERIMENTS
        sl.S.tile_no_full = 0u;
        if (const char* e = exp_env("GP_NO_FULLTILE")) sl.S.tile_no_full = e[0] == '1' ? 1u : 0u;
#endif
        if ((rc = alloc_slab(s, sl, sl.rank))) return rc;
        sl.S.rregions = rreg;
        if (sl.S.tile_walk == 3) {  // the tile list of the per-XCD queues
            std::vector<uint32_t> list;
            if (!build_walk_list(sl.S.lo, sl.S.nloc, sl.S.G.g2, sl.S.tile_wx, (int)sl.S.rregions, list, sl.S.woff)) {
                set_err("internal: walk-3 tile list does not cover the slab");
                return GP_EINVAL;
            }
            if ((rc = dev_alloc_t(s, &sl.S.wtiles, list.size() + 1))) return rc;
            HIP_TRY(hipMemcpy(sl.S.wtiles, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice));
        }
    }
    if (s->cfg.topology == GP_IMP3D && (rc = build_imp3d(s))) return rc;
    if ((s->cfg.topology == GP_IMP3D || s->cfg.topology == GP_FULL) && s->world > 1 && (rc = setup_exchange(s)))
        return rc;
    if ((rc = setup_halo(s))) return rc;
    if (s->world > 1) build_transfers(s);
    if (hipHostMalloc((void**)&s->host_ctl, sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
        set_err("hipHostMalloc failed");
        return GP_ENOMEM;
    }
    Ctl& init = *s->host_ctl;
    std::memset(&init, 0, sizeof init);
    init.active_total = 1;  // the seed
    init.all_active = s->P <= 1 ? 1u : 0u;
    init.inj_target = -1;
    init.inj_pick = -1;
    for (Slab& sl : s->slab) {
        DevState& S = sl.S;
        HIP_TRY(hipMemcpyAsync(S.ctl, &init, sizeof(Ctl), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(launch_init(S, s->grid, s->stream));
        if (S.topo == IMP3D)
            HIP_TRY(col_gossip_counts(S) ? launch_col_seed_init(S, s->stream) : launch_rbits_init(S, s->grid, s->stream));
        if (S.alg == GOSSIP && S.topo != FULL) HIP_TRY(launch_injector_init(S, s->grid, s->stream));
    }
    if ((rc = exchange(s, 0))) return rc;     // halos and random edges of round 0
    if ((rc = finalize(s, 0, 0))) return rc;  // prepare round 0
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        set_err("initialisation failed: %s", hipGetErrorString(e));
        return GP_EHIP;
    }
    if (s->timing) {
        s->ev.resize((size_t)2 * BATCH * round_launches(s));
        for (auto& x : s->ev) HIP_TRY(hipEventCreate(&x));
    }
    return GP_OK;
}

}  // namespace

int create_common(const gp_config* cfg, int mode, int world, int rank, const uint8_t* uid, gp_sim** out) {
    if (!cfg || !out) {
        set_err("gp_create: null argument");
        return GP_EINVAL;
    }
    *out = nullptr;
    if (cfg->algorithm != GP_GOSSIP && cfg->algorithm != GP_PUSHSUM) {
        set_err("option invalid: algorithm id %d", cfg->algorithm);
        return GP_EINVAL;
    }
    int64_t P, T, g;
    int rc = gp_resolve(cfg->num_nodes, cfg->topology, &P, &T, &g);
    if (rc) return rc;
    if ((rc = check_device(cfg->device))) return rc;
    gp_sim* s = new gp_sim();
    s->cfg = *cfg;
    s->device = cfg->device;
    s->P = P;
    s->T = T;
    s->g = g;
    s->mode = mode;
    s->world = world;
    s->rank = rank;
    s->timing = (cfg->flags & GP_FLAG_KERNEL_TIMING) != 0;
    if (hipSetDevice(s->device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        set_err("hipSetDevice/hipStreamCreate failed on device %d", s->device);
        gp_destroy(s);
        return GP_EHIP;
    }
    if (mode == MODE_RCCL) {
        ncclUniqueId id;
        std::memcpy(id.internal, uid, NCCL_UNIQUE_ID_BYTES);
        ncclResult_t r = ncclCommInitRank(&s->comm, world, id, rank);
        if (r != ncclSuccess) {
            set_err("ncclCommInitRank(rank %d of %d) failed: %s", rank, world, ncclGetErrorString(r));
            s->comm = nullptr;
            gp_destroy(s);
            return GP_ENCCL;
        }
    }
    rc = build_sim(s);
    if (rc) {
        const std::string msg = g_err;
        gp_destroy(s);
        g_err = msg;
        return rc;
    }
    *out = s;
    return GP_OK;
}
