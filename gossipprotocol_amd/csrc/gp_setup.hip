// gp_setup.hip -- everything a simulation needs before round 0 (create_common / build_sim): the
// experiments build's overrides (read_overrides, their one reader), the slab plan, the device's
// answers to what the kernel plan asks (plan_kernels), every slab's device state and the halo
// buffers; then the Imp3D topology build (gp_topology.hip) and the exchange buffers
// (gp_xlayout.hip).  The plans' arithmetic and rules are gp_plan.hpp and gp_kernel_plan.hpp.
#include "gp_host.hpp"

namespace {

// The experiments build (-DGP_EXPERIMENTS, libgossip_hip_exp.so) reads the GP_* environment
// overrides the kernel-variant tests use; the product library reads none (nullptr: every
// override below folds away, its name included -- tests/test_abi.py checks the strings).
inline const char* exp_env(const char* name) {
#ifdef GP_EXPERIMENTS
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

}  // namespace

// Every GP_* override, parsed: read when a handle is created (gp_sim::exp), and by gp_create_rank
// for GP_FORCE_RCCL, which counts before one exists.
ExpOverrides read_overrides() {
    auto count = [](const char* name, int least) -> std::optional<uint32_t> {  // a number, at least `least`
        const char* e = exp_env(name);
        if (!e) return std::nullopt;
        return (uint32_t)std::max(least, std::atoi(e));
    };
    auto number = [](const char* name) -> std::optional<int> {
        const char* e = exp_env(name);
        if (!e) return std::nullopt;
        return std::atoi(e);
    };
    auto is_one = [](const char* name) -> std::optional<bool> {
        const char* e = exp_env(name);
        if (!e) return std::nullopt;
        return e[0] == '1';
    };
    ExpOverrides o;
    KernelOverrides& k = o.kernel;
    if (const char* e = exp_env("GP_KERNEL"))
        k.kernel = !std::strcmp(e, "tile") ? KERNEL_TILE : !std::strcmp(e, "col") ? KERNEL_COL : !std::strcmp(e, "block") ? KERNEL_BLOCK : 0;
    k.xsegs = count("GP_XSEGS", 1);
    if (const auto v = number("GP_WALK")) k.walk = (uint32_t)*v;
    k.wx = count("GP_WX", 1);
    k.wide = is_one("GP_WIDE");
    k.rregions = number("GP_RREGIONS");
    k.xregions = number("GP_XREGIONS");
    if (const char* e = exp_env("GP_FUSE")) k.fuse = (uint32_t)(e[0] - '0');
    k.stage_cap = count("GP_STAGE_CAP", 0);
    k.no_full = is_one("GP_NO_FULLTILE");
    if (const char* e = exp_env("GP_GRID")) k.grid = e;
    o.fb_cap1 = count("GP_FB_CAP1", 1);
    o.fb_cap2 = count("GP_FB_CAP2", 1);
    o.fb_fused = is_one("GP_FB_FUSED");
    o.rq8 = is_one("GP_RQ8");
    o.halo_cap = count("GP_HALO_CAP", 1);
    o.xcap = count("GP_XCAP", 1);
    o.no_pack = is_one("GP_NO_PACK");
    o.ind4_wide = count("GP_IND4_WIDE", 1);
    o.slot_shadow = is_one("GP_SLOT_SHADOW");
    o.force_rccl = is_one("GP_FORCE_RCCL");
    o.check_close = exp_env("GP_CHECK_CLOSE") != nullptr;
    return o;
}

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
        if (s->exp.fb_cap2) S.fb_cap2 = std::min<uint32_t>(FB_CAP2, *s->exp.fb_cap2);
        const size_t m2 = (size_t)fp.nb2 * S.fb_cap2;
        if ((rc = dev_alloc_t(s, &S.fb_cnt2, fp.nb2)) || (rc = dev_alloc_t(s, &S.fb_hdr2, m2)) ||
            (rc = dev_alloc_t(s, &S.fb_pay2, m2)))
            return rc;
        if (W == 1) {
            // one rank: coarse bins hdr1 / pay1; the fold of round r bins round r+1's messages
            // into them (k_fb_fold<FOLD_SEND>; GP_FB_FUSED=0, experiments: three passes)
            const bool fused = s->exp.fb_fused.value_or(true);
            const FullBinPlan f1 = full_bin_plan(S.nloc, fused);
            S.fb_s1 = f1.s1;
            S.fb_nb1 = f1.nb1;
            S.fb_cap1 = f1.cap1;
            if (s->exp.fb_cap1) S.fb_cap1 = std::min<uint32_t>(f1.cap1, *s->exp.fb_cap1);
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
        S.rq8 = s->exp.rq8.value_or(true) ? 1u : 0u;  // (GP_RQ8=0, experiments: word counters)
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
    if (s->exp.halo_cap) s->halo_cap = std::min<uint32_t>(s->halo_cap, *s->exp.halo_cap);
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

// The kernel plan of this run (kernel_plan, gp_kernel_plan.hpp) into s->kplan / grid / cus, from
// the device's answers to what the plan asks.  GP_EINVAL: a GP_GRID the run cannot take.
int plan_kernels(gp_sim* s) {
    static_assert(RunShape::Line == GP_LINE && RunShape::Full == GP_FULL && RunShape::Grid3D == GP_3D &&
                      RunShape::Imp3D == GP_IMP3D && RunShape::Gossip == GP_GOSSIP && RunShape::PushSum == GP_PUSHSUM &&
                      RunShape::Line == LINE && RunShape::Grid3D == GRID3D && RunShape::Imp3D == IMP3D,
                  "the plan's topology and algorithm values are the C ABI's and the kernels'");
    RunShape shape;
    shape.topology = s->cfg.topology;
    shape.algorithm = s->cfg.algorithm;
    shape.g = s->g;
    shape.world = s->world;
    shape.mode = s->mode;
    shape.bounds = s->bounds;
    struct Device {
        const gp_sim* s;
        const RunShape& r;
        int cus() const {
            hipDeviceProp_t prop;
            (void)hipGetDeviceProperties(&prop, s->device);
            return prop.multiProcessorCount;
        }
        bool block_resident(const BlockPlan& bp, int cus) const { return block_plan_resident(bp, cus); }
        int col_blocks_per_cu() const { return gp::col_blocks_per_cu(s->cfg.topology, s->cfg.algorithm); }
        int res4() const { return ps_tile_resident_blocks(r.tile_topo(), r.tile_remote(), s->device); }
        int res_wide() const { return wide::ps_tile_resident_blocks(r.tile_topo(), r.tile_remote(), s->device); }
    };
    const KernelFacts facts = gather_kernel_facts(shape, s->exp.kernel, Device{s, shape});
    KernelPlanError err;
    s->kplan = kernel_plan(shape, facts, s->exp.kernel, err);
    s->cus = std::max(1, facts.cus);
    s->grid = s->kplan.grid;
#ifdef GP_EXPERIMENTS  // (only an override can be refused; the product library does not carry its name)
    if (err.bad_grid) {
        set_err("GP_GRID=%s: not a grid of 1..%d blocks", s->exp.kernel.grid->c_str(), err.grid_max);
        return GP_EINVAL;
    }
#endif
    return GP_OK;
}

// Everything after the handle exists: slabs, topology, initial state, round 0.
int build_sim(gp_sim* s) {
    int rc;
    if ((rc = make_bounds(s))) return rc;
    if ((rc = plan_kernels(s))) return rc;
    const KernelPlan& kp = s->kplan;
    if (s->mode == MODE_VIRTUAL) {
        s->slab.resize(s->world);
        for (int w = 0; w < s->world; ++w) s->slab[w].rank = w;
    } else {
        s->slab.resize(1);
        s->slab[0].rank = s->rank;
    }
    for (Slab& sl : s->slab) {
        sl.S.kernel = kp.kernel;
        sl.S.tile_wide = kp.wide;
        sl.S.col_xsegs = kp.col_xsegs;
        sl.S.tile_walk = kp.walk;
        sl.S.tile_wx = kp.wx;
        sl.S.tile_stage_cap = kp.stage_cap;
        sl.S.fuse_finalize = kp.fuse_finalize;
        sl.S.bplan = kp.bplan;
        sl.S.bface = sl.S.bscratch = nullptr;
        if (kp.kernel == KERNEL_BLOCK) {  // face exchange buffers + barrier / accumulator scratch
            if ((rc = dev_alloc(s, &sl.S.bface, block_face_bytes(kp.bplan))) || (rc = dev_alloc(s, &sl.S.bscratch, BLOCK_SCRATCH_BYTES)))
                return rc;
            HIP_TRY(block_kernel_setup(kp.bplan));
        }
#ifdef GP_EXPERIMENTS
        sl.S.tile_no_full = kp.no_full;
        sl.S.tile_slot_shadow = s->exp.slot_shadow.value_or(true) ? 1u : 0u;
#endif
        if ((rc = alloc_slab(s, sl, sl.rank))) return rc;
        sl.S.rregions = kp.rregions;
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
    s->exp = read_overrides();
    s->device = cfg->device;
    s->P = P;
    s->T = T;
    s->g = g;
    s->mean = (double)(P - 1) * 0.5;
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
