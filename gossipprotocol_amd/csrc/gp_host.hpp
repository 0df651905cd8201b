// gp_host.hpp -- what the host units of libgossip_hip.so share: gp_setup.hip, gp_topology.hip and
// gp_xlayout.hip (before round 0), gp_exchange.hip (one round across ranks), gp_api.hip (C ABI,
// gp_step batch loop) and, for the error slot and device check, gp_ensemble_api.hip.  Hidden
// symbols: not the library's surface.  What a run over several ranks allocates and addresses is
// decided by gp_plan.hpp, which round kernel it gets by gp_kernel_plan.hpp; these units carry it
// out.  The experiments build's GP_* overrides are read once, at create, into gp_sim::exp
// (ExpOverrides; read_overrides, gp_setup.hip).
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <rccl/rccl.h>

#include "../../include/gossip_hip.h"
#include "gp_internal.hpp"
#include "gp_full.hpp"
#include "gp_fullbin.hpp"

#include "gp_xchg.hpp"

#pragma GCC visibility push(hidden)
#include "gp_values.hpp"
using namespace gp;

// The calling thread's gp_last_error() message: one slot per thread for all units (gp_api.hip).
extern thread_local std::string g_err;
void set_err(const char* fmt, ...);
int check_device(int device);

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return GP_EHIP;                                                             \
        }                                                                               \
    } while (0)

#define NCCL_TRY(expr)                                                                  \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess) {                                                        \
            set_err("%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
            return GP_ENCCL;                                                            \
        }                                                                               \
    } while (0)

constexpr int64_t BATCH = 1024;  // rounds queued per host synchronisation (<= HIST)
static_assert(BATCH <= HIST, "alert ring must cover a batch");

// The GP_* environment overrides of the experiments build (-DGP_EXPERIMENTS,
// libgossip_hip_exp.so), which the kernel-variant tests use, as they stood when the handle was
// created; the product library reads none, so there every field is empty.  An empty field: not set.
struct ExpOverrides {
    KernelOverrides kernel;                        // what the kernel plan takes (gp_kernel_plan.hpp)
    std::optional<uint32_t> fb_cap1, fb_cap2;      // GP_FB_CAP1 / GP_FB_CAP2
    std::optional<bool> fb_fused;                  // GP_FB_FUSED
    std::optional<bool> rq8;                       // GP_RQ8
    std::optional<uint32_t> halo_cap;              // GP_HALO_CAP
    std::optional<uint32_t> xcap;                  // GP_XCAP
    std::optional<bool> no_pack;                   // GP_NO_PACK
    std::optional<uint32_t> ind4_wide;             // GP_IND4_WIDE
    std::optional<bool> slot_shadow;               // GP_SLOT_SHADOW (k_ps_tile; 0: the ordering before DESIGN.md 5.1.0b)
    std::optional<bool> force_rccl;                // GP_FORCE_RCCL
    bool check_close = false;                      // GP_CHECK_CLOSE (set to anything)
};
ExpOverrides read_overrides();  // gp_setup.hip

// One inter-rank transfer of a slab: `bytes` at `ptr`, sent to or received from rank `peer`
// (build_transfers / run_transfers, gp_exchange.hip).
struct Xfer { bool send; int peer; uint8_t* ptr; size_t bytes; };

// One rank's share of the network.
struct Slab {
    DevState S{};
    int rank = 0;
    uint32_t hi = 0;  // one past the last owned id
    // random-edge / full-topology exchange (W > 1; which form: gp_sim::kplan.xkind)
    // Imp3D gossip on the tile kernel (XKind::Slots): per local sender, its in-edge slot at the
    // owner of its random edge's target and that owner's rank (k_make_pos; k_pack)
    uint32_t* pos = nullptr;
    uint8_t* xdst = nullptr;
    uint8_t* xsend = nullptr;
    uint8_t* xrecv = nullptr;
    uint32_t nedges = 0;
    XLayout xl;                        // capacities and byte layout of xsend / xrecv / xown (setup_exchange)
    unsigned int* overflow = nullptr;  // device flag
    // Imp3D push-sum over several ranks: sender-ordered lists (gp_xchg.hpp)
    uint32_t nt = 0;                   // the slab's tiles
    uint32_t tb[XMAXH + 1] = {};       // region h: tiles [tb[h], tb[h + 1])
    uint32_t* gw = nullptr;            // [tile * W + d]: first header word of the tile's segment
    uint16_t* xdr = nullptr;           // [id - lo]: d << 10 | rank in the tile's list for d (static)
    uint8_t* lwt = nullptr;            // [tile * (W + 1) + d]: the tile's LDS word layout in k_list_pack
    uint32_t* xcnt = nullptr;          // [h * W + d]: reservation counters of the send chunks
    // full push-sum over several ranks: this rank's own share of region h's bins, by round parity:
    // parity 0 in xrecv (its receive region from itself), parity 1 in xown -- the fold of round r
    // fills parity r + 1 while the split of round r has read parity r, and a round's counters are
    // all cleared at its start (launch_round_full_multi)
    uint8_t* xown = nullptr;
    // Imp3D gossip (column kernel) over several ranks: random-edge sends as bitmaps (gp_xchg.hpp)
    uint32_t* rbits_in = nullptr;      // receive bitmap: source a's chunk at bit ro[a]
    uint32_t* tgt = nullptr;           // local target of every receive-bitmap bit
    BitsLayout bl;                     // the chunks of the send and receive bitmaps (build_bits)
    // push-sum halo planes (3D / Imp3D, W > 1): the senders' (s, w) toward each neighbour, compacted
    // ([0]: lower neighbour, [1]: upper; k_halo_pack / k_halo_expand, gp_xchg.hpp)
    double2* hsend[2] = {nullptr, nullptr};
    double2* hrecv[2] = {nullptr, nullptr};
    // every transfer of a round, by the parity of the round it prepares (build_transfers): the
    // halo planes, and region h's random-edge / full-topology messages
    std::vector<Xfer> xhalo[2];
    std::vector<std::vector<Xfer>> xplan[2];  // [parity][h]
};

// (the C ABI's handle type: default visibility, like its declaration in include/gossip_hip.h)
#pragma GCC visibility pop
struct gp_sim {
    gp_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    ExpOverrides exp;  // the experiments build's overrides, read at create
    KernelPlan kplan;  // kernel variant, walk, grid, regions (gp_kernel_plan.hpp)
    int grid = 1;      // kplan.grid
    int cus = 1;       // compute units of the device
    int64_t P = 0, T = 0, g = 0;
    int mode = MODE_SINGLE;
    int world = 1, rank = 0;  // ranks sharing the population; this process's rank (RCCL)
    std::vector<uint32_t> bounds;  // world + 1 slab boundaries (global ids)
    uint32_t halo = 0;             // ids per halo side
    std::vector<Slab> slab;        // MODE_VIRTUAL: all ranks; otherwise this rank's
    ncclComm_t comm = nullptr;
    int64_t rounds_done = 0;
    int64_t alerts_total = 0;
    bool done = false;
    Ctl* host_ctl = nullptr;  // pinned mirror of slab 0's control block (global bookkeeping)
    std::vector<void*> allocs;
    // kernel timing
    bool timing = false;
    std::vector<hipEvent_t> ev;
    double kernel_ms = 0.0;
    int64_t launches = 0;
    // exchange buffers per rank pair: xhalves regions (2: full-topology push-sum, whose exchange runs
    // in two halves of each rank's senders on xstream, overlapped with the send / coarse passes)
    int xhalves = 1;
    size_t halo_slots = 0;  // push-sum halo planes travel compacted (setup_halo): slots per buffer, else 0
    uint32_t halo_cap = 0;  // ... slots per 1024-node chunk (halo_chunk_cap)
    // Imp3D push-sum lists: header words of chunk (h, a -> b) at [(a * xhalves + h) * world + b],
    // every slab's (each rank computes the whole table from the global random edges)
    std::vector<uint32_t> list_nw;
    hipStream_t xstream = nullptr;
    hipEvent_t ev_send[XMAXH] = {}, ev_xfer[XMAXH] = {};
    // gp_summary_take (gp_summary.hip): partial records and gather buffer, allocated at the first call
    void* sum_scratch = nullptr;
    size_t sum_scratch_bytes = 0;
    // SRS v1-V (gp_values.hip): mu, the value the summaries' error fields are measured against --
    // (P - 1) / 2 unless gp_set_mean changed it; the staging of gp_set_values; values_dirty: values
    // were set on a handle whose round-0 exchange has run (gp_step repeats it before round 0)
    double mean = 0.0;
    ValStage vstage;
    bool values_dirty = false;
};
#pragma GCC visibility push(hidden)

inline int dev_alloc(gp_sim* s, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        set_err("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return GP_ENOMEM;
    }
    s->allocs.push_back(*p);
    return GP_OK;
}

template <typename T>
int dev_alloc_t(gp_sim* s, T** p, size_t count) {
    void* v = nullptr;
    int rc = dev_alloc(s, &v, count * sizeof(T));
    *p = static_cast<T*>(v);
    return rc;
}

// Setup temporaries: freed when the scope ends, on success and on every error return.
struct Scratch {
    std::vector<void*> ptrs;
    template <typename T>
    hipError_t alloc(T** p, size_t count) {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, count * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(v);
        *p = static_cast<T*>(v);
        return e;
    }
    ~Scratch() {
        for (void* v : ptrs) (void)hipFree(v);
    }
};

// Imp3D gossip on the column kernel: random-edge deliveries are counted at their targets a
// round ahead (rq) -- by local senders' atomics, and for senders on other ranks from the received
// bitmaps (XKind::Bits, k_apply_bits); no random-edge bits, in-edge tags or slots.  Selects kernel
// behaviour (the rq arrays and their seeding); the exchange is selected by kplan.xkind.
inline bool col_gossip_counts(const DevState& S) { return S.topo == IMP3D && S.alg == GOSSIP && S.kernel == KERNEL_COL; }

// gp_setup.hip
int create_common(const gp_config* cfg, int mode, int world, int rank, const uint8_t* uid, gp_sim** out);

// gp_topology.hip: the Imp3D in-lists and, across ranks, the lists / bitmaps / slots of the random edges
int build_imp3d(gp_sim* s);

// gp_xlayout.hip: the exchange buffers of the random-edge / full-topology messages
int setup_exchange(gp_sim* s);

// gp_exchange.hip
void build_transfers(gp_sim* s);
int exchange(gp_sim* s, uint32_t rn);
int finalize(gp_sim* s, uint32_t round_done, uint32_t round_next);
uint32_t round_launches(const gp_sim* s);
int launch_round(gp_sim* s, uint32_t r, hipEvent_t* ev);
#pragma GCC visibility pop
