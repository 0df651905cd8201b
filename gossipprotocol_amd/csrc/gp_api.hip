// gp_api.hip -- C-ABI of libgossip_hip.so (include/gossip_hip.h): argument checks, the
// calling thread's error slot, and the gp_step batch loop.  The host side behind it:
// gp_setup.hip, gp_topology.hip and gp_xlayout.hip (everything before round 0) and
// gp_exchange.hip (one round across ranks), sharing gp_host.hpp.
//
// Replaces, in /root/reference/Project2/Program.fs:
//   * actor population + topology build (Program.fs:169-176,180-191,209-216,238-261)
//     -> gp_create / gp_create_rank (gp_setup.hip): SoA device state per slab, implicit
//     neighbours, Imp3D receiver-sorted in-lists;
//   * message loop + scheduler (Program.fs:41-61,84-131,141-163) -> gp_step / gp_run:
//     per round the bulk round kernel, the inter-rank exchange and the
//     finalize kernel(s) (gp_exchange.hip launch_round), queued in batches with one
//     host synchronisation per batch (never per round).
#include "gp_host.hpp"

thread_local std::string g_err;

void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        set_err("no HIP device visible (libgossip_hip needs an MI355X / gfx950)");
        return GP_ENODEV;
    }
    if (device < 0 || device >= n) {
        set_err("device %d out of range (%d visible)", device, n);
        return GP_EINVAL;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err("device %d is %s; libgossip_hip is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return GP_ENODEV;
    }
    return GP_OK;
}

static double alg_bytes(const gp_sim* s) {
    const DevState& S = s->slab[0].S;
    if (S.alg == PUSHSUM) {
        // sw r+w 32, node byte r+w 2 (+ Imp3D: in-degree nibble 0.5 + sender 4 of the
        // in-list, and the random-edge message payload, 16 B for the ~1/7 of senders
        // that use the random edge -- a random gather, moved as a 128-B line)
        if (S.topo == IMP3D) return 38.5 + 16.0 / 7.0;
        if (S.kernel == KERNEL_BLOCK) {
            // LDS-resident: per round only the boxes' boundary layers move (17 B per face node,
            // written once, read once by the neighbour), through L2 / Infinity Cache
            const BlockPlan& p = S.bplan;
            const double g = S.G.g;
            const double faces = g * g * ((p.nbx - 1) + (p.nby - 1) + (p.nbz - 1)) * 2.0;
            return 2.0 * 17.0 * faces / (double)S.G.P;
        }
        if (S.topo != FULL) return 34.0;
        // send: byte 1 (sweep 1) + byte 1 + own (s, w) 16 + message write 20; split: sender
        // id 4 (sweep 1) + message r+w 40; fold: message 20 + own (s, w) r+w 32 + byte r+w 2
        // (gp_fullbin.hip, range binning).  One rank: the fold writes the next round's
        // messages from the state it just computed, so the send's reads (18) go.
        if (S.fb_fused) return 20.0 + 4.0 + 40.0 + 20.0 + 32.0 + 2.0;
        return 1.0 + 1.0 + 16.0 + 20.0 + 4.0 + 40.0 + 20.0 + 32.0 + 2.0;
    }
    // gossip: counter r+w 8, direction byte r+w 2; Imp3D:
    //   column kernel (counts random-edge sends at their targets a round ahead): rnd 4 +
    //   delivery count read (a byte since round 4; was 4 B), its zeroing where non-zero
    //   and the senders' atomic increments (~1/7 of nodes each, a 4-B word atomic) ->
    //   15 + 5/7 (4-B counts: 18 + 8/7; several ranks: the remote 7/8 of the increments
    //   arrive as bits, counted by k_apply_bits instead);
    //   tile kernel: in-list 8
    if (S.topo == IMP3D) return S.rq[0] ? (S.rq8 ? 15.0 + 5.0 / 7.0 : 18.0 + 8.0 / 7.0) : 18.0;
    if (S.topo != FULL) return 10.0;
    return 4.0 + 8.0 + 8.0 + 8.0;  // send: c + atomic RMW; recv: inc r+w, c r+w
}

extern "C" {

int gp_version(void) { return GP_VERSION; }

const char* gp_last_error(void) { return g_err.c_str(); }

int gp_parse_topology(const char* t) {
    if (!t) return GP_EINVAL;
    if (!std::strcmp(t, "line")) return GP_LINE;
    if (!std::strcmp(t, "full")) return GP_FULL;
    if (!std::strcmp(t, "3D")) return GP_3D;
    if (!std::strcmp(t, "Imp3D") || !std::strcmp(t, "imp3D")) return GP_IMP3D;
    set_err("unknown topology '%s' (line | full | 3D | Imp3D)", t);
    return GP_EINVAL;
}

int gp_parse_algorithm(const char* a) {
    if (!a) return GP_EINVAL;
    if (!std::strcmp(a, "gossip")) return GP_GOSSIP;
    if (!std::strcmp(a, "push-sum")) return GP_PUSHSUM;
    set_err("option invalid: algorithm '%s' (gossip | push-sum)", a);
    return GP_EINVAL;
}

int gp_resolve(int64_t n, int32_t topology, int64_t* P, int64_t* T, int64_t* g) {
    if (!P || !T || !g) {
        set_err("gp_resolve: null output");
        return GP_EINVAL;
    }
    if (n < 1) {
        set_err("num_nodes must be >= 1 (got %lld)", (long long)n);
        return GP_EINVAL;
    }
    if (topology == GP_LINE || topology == GP_FULL) {
        *P = n + 1;
        *T = n;
        *g = 0;
    } else if (topology == GP_3D || topology == GP_IMP3D) {
        int64_t gg = (int64_t)std::cbrt((double)n);  // exact integer ceil(cbrt(n)) (Q3)
        while (gg > 0 && gg * gg * gg >= n) --gg;
        while (gg * gg * gg < n) ++gg;
        *g = gg;
        *P = gg * gg * gg;
        *T = *P;
    } else {
        set_err("unknown topology id %d", topology);
        return GP_EINVAL;
    }
    if (*P > (int64_t)GP_MAX_POPULATION) {
        set_err("population %lld exceeds the 32-bit node-id range", (long long)*P);
        return GP_EINVAL;
    }
    return GP_OK;
}

int gp_create(const gp_config* cfg, gp_sim** out) {
    if (!cfg || !out) {
        set_err("gp_create: null argument");
        return GP_EINVAL;
    }
    if (cfg->num_gpus > 1) {
        if (cfg->flags & GP_FLAG_VIRTUAL_RANKS) return create_common(cfg, MODE_VIRTUAL, cfg->num_gpus, 0, nullptr, out);
        set_err("num_gpus > 1: one process per GPU -- launch `gossip <n> <topology> <algorithm> --gpus %d` "
                "(or GOSSIP_GPUS=%d), which joins every rank through gp_rendezvous_id + gp_create_rank; "
                "GP_FLAG_VIRTUAL_RANKS runs the slabs in this process on one GPU", cfg->num_gpus, cfg->num_gpus);
        return GP_EINVAL;
    }
    return create_common(cfg, MODE_SINGLE, 1, 0, nullptr, out);
}

int gp_get_unique_id(uint8_t unique_id[128]) {
    if (!unique_id) {
        set_err("gp_get_unique_id: null buffer");
        return GP_EINVAL;
    }
    static_assert(NCCL_UNIQUE_ID_BYTES == 128, "RCCL unique id size");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(unique_id, id.internal, NCCL_UNIQUE_ID_BYTES);
    return GP_OK;
}

int gp_rendezvous_id(int32_t rank, const char* path, int32_t timeout_ms, uint8_t unique_id[128]) {
    if (!path || !*path || !unique_id || rank < 0) {
        set_err("gp_rendezvous_id: bad argument");
        return GP_EINVAL;
    }
    const size_t N = 128;
    // GOSSIP_RDV_NONCE (set by the launchers, one value per launch): rank 0 writes it after
    // the id and readers accept only a file that carries theirs, so a file a crashed run
    // left at a caller-chosen path is never read as this run's id
    const char* nv = std::getenv("GOSSIP_RDV_NONCE");
    const std::string nonce = nv ? std::string(nv).substr(0, 64) : std::string();
    if (rank == 0) {  // publish: write a private name, then rename (readers never see a partial id)
        struct stat st;
        if (::stat(path, &st) == 0) {
            set_err("gp_rendezvous_id: '%s' already exists (left by an earlier run?); the path must be fresh", path);
            return GP_ESTATE;
        }
        int rc = gp_get_unique_id(unique_id);
        if (rc) return rc;
        const std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid());
        const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0600);
        if (fd < 0) {
            set_err("gp_rendezvous_id: cannot create '%s': %s", tmp.c_str(), std::strerror(errno));
            return GP_EINVAL;
        }
        std::string blob(reinterpret_cast<const char*>(unique_id), N);
        blob += nonce;
        const bool ok = ::write(fd, blob.data(), blob.size()) == (ssize_t)blob.size() && ::fsync(fd) == 0;
        ::close(fd);
        if (!ok || ::rename(tmp.c_str(), path) != 0) {
            set_err("gp_rendezvous_id: cannot publish '%s': %s", path, std::strerror(errno));
            ::unlink(tmp.c_str());
            return GP_EINVAL;
        }
        return GP_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {  // wait for rank 0's file (with this launch's nonce)
        const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
        if (fd >= 0) {
            char buf[128 + 65];
            const ssize_t got = ::read(fd, buf, sizeof buf);
            ::close(fd);
            if (got < (ssize_t)N) {
                set_err("gp_rendezvous_id: '%s' holds %zd bytes, expected %zu", path, got, N);
                return GP_EINVAL;
            }
            if (std::string(buf + N, (size_t)got - N) == nonce) {
                std::memcpy(unique_id, buf, N);
                return GP_OK;
            }
            // another launch's file: keep waiting for ours (rank 0 refuses to overwrite it,
            // so this ends at the timeout with the error below)
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (timeout_ms >= 0 && ms >= timeout_ms) {
            set_err("gp_rendezvous_id: rank %d waited %d ms for rank 0's id at '%s'%s", rank, timeout_ms, path,
                    fd >= 0 ? " (the file there carries another launch's nonce)" : "");
            return GP_ESTATE;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
}

int gp_create_rank(const gp_config* cfg, int32_t rank, int32_t world, const uint8_t unique_id[128], gp_sim** out) {
    if (!cfg || !out || world < 1 || rank < 0 || rank >= world) {
        set_err("gp_create_rank: bad argument (rank %d, world %d)", rank, world);
        return GP_EINVAL;
    }
    // GP_FORCE_RCCL=1 (experiments): a one-rank RCCL communicator (test of the RCCL transport
    // on a single GPU: init, bookkeeping all-reduce, teardown)
    const bool force = read_overrides().force_rccl.value_or(false);
    if (world == 1 && !force) return create_common(cfg, MODE_SINGLE, 1, 0, nullptr, out);
    if (!unique_id) {
        set_err("gp_create_rank: null unique id");
        return GP_EINVAL;
    }
    return create_common(cfg, MODE_RCCL, world, rank, unique_id, out);
}

int64_t gp_step(gp_sim* s, int64_t nrounds, int64_t* alerts_out) {
    if (!s) {
        set_err("gp_step: null handle");
        return GP_EINVAL;
    }
    if (nrounds < 0) {
        set_err("gp_step: negative round count");
        return GP_EINVAL;
    }
    if (hipSetDevice(s->device) != hipSuccess) {
        set_err("hipSetDevice failed");
        return GP_EHIP;
    }
    if (s->vstage.bytes) values_stage_free(s->vstage);  // (values are the initial state: no use for the staging from here on)
    if (s->values_dirty) {  // gp_set_values after create's round-0 exchange: halo planes and lists again (SRS v1-V)
        s->values_dirty = false;
        if (s->rounds_done == 0) {
            const int rc = exchange(s, 0);
            if (rc) return rc;
        }
    }
    int64_t executed = 0;
    while (executed < nrounds && !s->done) {
        int64_t batch = std::min<int64_t>(nrounds - executed, BATCH);
        if (s->cfg.max_rounds > 0) batch = std::min<int64_t>(batch, s->cfg.max_rounds - s->rounds_done);
        if (batch <= 0) break;
        const bool block = s->slab[0].S.kernel == KERNEL_BLOCK;
        if (block) {  // the whole batch in one cooperative launch (gp_block.hip)
            const DevState& S = s->slab[0].S;
            if (s->timing) HIP_TRY(hipEventRecord(s->ev[0], s->stream));
            const hipError_t le = launch_round_block(S, S.bplan, (uint32_t)s->rounds_done, (uint32_t)batch, S.bface,
                                                     S.bscratch, s->stream);
            if (le != hipSuccess) {
                set_err("the LDS-resident round kernel's cooperative launch failed: %s (its %u workgroups must be "
                        "resident on the device at once)",
                        hipGetErrorString(le), S.bplan.nbx * S.bplan.nby * S.bplan.nbz);
                return GP_EHIP;
            }
            if (s->timing) HIP_TRY(hipEventRecord(s->ev[1], s->stream));
            unsigned int flags[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(flags, S.bscratch, sizeof flags, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            if (flags[1]) {
                set_err("the LDS-resident round kernel's grid barrier timed out (a workgroup never arrived); "
                        "the rounds of this batch are invalid");
                return GP_ESTATE;
            }
        } else {
            const size_t nl = round_launches(s);
            for (int64_t k = 0; k < batch; ++k) {
                const uint32_t r = (uint32_t)(s->rounds_done + k);
                int rc = launch_round(s, r, s->timing ? &s->ev[2 * nl * k] : nullptr);
                if (rc) return rc;
            }
        }
        HIP_TRY(hipMemcpyAsync(s->host_ctl, s->slab[0].S.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        const Ctl& hc = *s->host_ctl;
        if (hc.tiny) {
            set_err("a push-sum (s, w) value fell below 2^-1020, where the tile kernel's fused fold "
                    "(v_fma_f64(m, 0.5, acc)) is no longer guaranteed to round like the specification's "
                    "acc + m * 0.5; the rounds of this batch are invalid");
            return GP_ESTATE;
        }
        if (hc.overflow) {
            set_err("message buffer overflow (an exchange buffer or a message bin exceeded its capacity = "
                    "expected + 12 sigma); the rounds of this batch are invalid");
            return GP_ESTATE;
        }
        int64_t cum = s->alerts_total, ex = 0;
        for (int64_t k = 0; k < batch; ++k) {
            const int64_t r = s->rounds_done + k;
            const int64_t a = (int64_t)hc.hist[r % HIST];
            cum += a;
            if (alerts_out) alerts_out[executed + ex] = a;
            ++ex;
            if (cum >= s->T) break;
        }
        if (hc.done ? (cum != (int64_t)hc.alerts_total || cum < s->T)
                    : (ex != batch || cum != (int64_t)hc.alerts_total)) {
            set_err("round bookkeeping mismatch (device %llu alerts, host %lld)", hc.alerts_total, (long long)cum);
            return GP_ESTATE;
        }
        if (s->timing && block) {  // one launch for the batch: its time over the rounds it ran
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
            s->kernel_ms += ms;
            s->launches += ex;
        } else if (s->timing) {  // per round: the sum over its round kernel launches
            const size_t nl = round_launches(s);
            for (int64_t k = 0; k < ex; ++k) {
                for (size_t h = 0; h < nl; ++h) {
                    float ms = 0.f;
                    HIP_TRY(hipEventElapsedTime(&ms, s->ev[2 * (nl * k + h)], s->ev[2 * (nl * k + h) + 1]));
                    s->kernel_ms += ms;
                }
                ++s->launches;
            }
        }
        s->rounds_done += ex;
        s->alerts_total = cum;
        s->done = hc.done != 0;
        executed += ex;
        if (s->mode != MODE_RCCL && s->exp.check_close) {  // (GP_CHECK_CLOSE) tests: recount the alerts from the state
            Scratch tmp;
            unsigned long long* d = nullptr;
            HIP_TRY(tmp.alloc(&d, 1));
            HIP_TRY(hipMemsetAsync(d, 0, sizeof(unsigned long long), s->stream));
            for (Slab& sl : s->slab) {
                const DevState& S = sl.S;
                const uint8_t* nb = nullptr;
                if (S.alg == PUSHSUM) nb = (S.topo == FULL ? S.nb[0] : S.nb[s->rounds_done & 1]) + (S.lo - S.base);
                HIP_TRY(launch_count_alerted(nb, S.alg == PUSHSUM ? nullptr : S.c, S.nloc, d, s->grid, s->stream));
            }
            unsigned long long h = 0;
            HIP_TRY(hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            if ((int64_t)h != cum) {
                set_err("round close check: %llu alerted nodes in the state, %lld counted by the round closes", h,
                        (long long)cum);
                return GP_ESTATE;
            }
        }
    }
    return executed;
}

int gp_run(gp_sim* s, gp_result* out) {
    if (!s || !out) {
        set_err("gp_run: null argument");
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int64_t r0 = s->rounds_done;
    const auto t0 = std::chrono::steady_clock::now();
    while (!s->done) {
        if (s->cfg.max_rounds > 0 && s->rounds_done >= s->cfg.max_rounds) break;
        int64_t n = gp_step(s, BATCH, nullptr);
        if (n < 0) return (int)n;
        if (n == 0) break;
    }
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    const int64_t rounds = s->rounds_done - r0;
    out->rounds = s->rounds_done;
    out->converged = s->alerts_total;
    out->population = s->P;
    out->threshold = s->T;
    out->elapsed_ms = ms;
    out->node_updates_per_s = ms > 0 ? (double)s->P * (double)rounds / (ms * 1e-3) : 0.0;
    out->hbm_bytes_alg = alg_bytes(s) * (double)s->P * (double)rounds;
    out->status = s->done ? GP_STATUS_CONVERGED : GP_STATUS_MAX_ROUNDS;
    out->reserved = 0;
    return GP_OK;
}

int gp_read_state(gp_sim* s, int64_t first, int64_t count, int32_t* c, double* sv, double* wv, uint8_t* flags) {
    if (!s) {
        set_err("gp_read_state: null handle");
        return GP_EINVAL;
    }
    if (first < 0 || count < 0 || first + count > s->P) {
        set_err("gp_read_state: range [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + count),
                (long long)s->P);
        return GP_EINVAL;
    }
    if (count == 0) return GP_OK;
    if (s->mode == MODE_RCCL) {
        const Slab& sl = s->slab[0];
        if (first < sl.S.lo || first + count > sl.hi) {
            set_err("gp_read_state: range [%lld, %lld) outside this rank's slab [%u, %u)", (long long)first,
                    (long long)(first + count), sl.S.lo, sl.hi);
            return GP_EINVAL;
        }
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int cur = (int)(s->rounds_done & 1);
    for (const Slab& sl : s->slab) {
        const DevState& S = sl.S;
        const int64_t a = std::max<int64_t>(first, S.lo), b = std::min<int64_t>(first + count, sl.hi);
        if (a >= b) continue;
        const int64_t n = b - a, q0 = a - first;
        if (S.alg == PUSHSUM) {
            std::vector<double2> sw((size_t)n);
            std::vector<uint8_t> nb((size_t)n);
            HIP_TRY(hipMemcpy(sw.data(), S.sw[cur] + (a - S.base), sizeof(double2) * n, hipMemcpyDeviceToHost));
            const uint8_t* nbsrc = S.topo == FULL ? S.nb[0] : S.nb[cur];
            HIP_TRY(hipMemcpy(nb.data(), nbsrc + (a - S.base), n, hipMemcpyDeviceToHost));
            for (int64_t q = 0; q < n; ++q) {
                if (c) c[q0 + q] = 0;
                if (sv) sv[q0 + q] = sw[q].x;
                if (wv) wv[q0 + q] = sw[q].y;
                if (flags) {
                    const uint8_t bb = nb[q];
                    flags[q0 + q] = (uint8_t)(((bb & B_ACTIVE) ? 1 : 0) | ((bb & B_CONV) ? 2 : 0) |
                                              (((bb >> CNT_SHIFT) & 3) << 2));
                }
            }
        } else {
            std::vector<int32_t> cc((size_t)n);
            HIP_TRY(hipMemcpy(cc.data(), S.c + (a - S.lo), sizeof(int32_t) * n, hipMemcpyDeviceToHost));
            for (int64_t q = 0; q < n; ++q) {
                const int64_t i = a + q;
                const int32_t ci = cc[q];
                if (c) c[q0 + q] = ci;
                if (sv) sv[q0 + q] = 0.0;
                if (wv) wv[q0 + q] = 0.0;
                if (flags) {
                    const bool act = (i == (int64_t)S.seed_node || ci >= 1) && ci <= 10;
                    flags[q0 + q] = (uint8_t)((act ? 1 : 0) | (ci >= 11 ? 2 : 0));
                }
            }
        }
    }
    return GP_OK;
}

int gp_neighbors(gp_sim* s, int64_t node, int64_t* out, int64_t cap) {
    if (!s || node < 0 || node >= s->P) {
        set_err("gp_neighbors: bad handle or node");
        return GP_EINVAL;
    }
    const DevState& S = s->slab[0].S;
    const uint32_t j = (uint32_t)node;
    std::vector<int64_t> nb;
    if (S.topo == FULL) {
        const int64_t deg = s->P - 1;
        for (int64_t k = 0; k < std::min(deg, cap); ++k) out[k] = full_target(j, (uint32_t)k);
        return (int)deg;
    }
    uint32_t mask = S.topo == LINE ? present_mask<LINE>(j, S.G) : present_mask<GRID3D>(j, S.G);
    for (uint32_t d = 0; d < 6; ++d)
        if (mask & (1u << d)) nb.push_back(S.topo == LINE ? nbr<LINE>(j, d, S.G) : nbr<GRID3D>(j, d, S.G));
    if (S.topo == IMP3D) nb.push_back(uniform(S.k0, S.k1, S_TOPO, j, 0, S.G.P - 1));  // Program.fs:259
    for (int64_t k = 0; k < std::min<int64_t>((int64_t)nb.size(), cap); ++k) out[k] = nb[(size_t)k];
    return (int)nb.size();
}

int gp_get_info(gp_sim* s, gp_info* o) {
    if (!s || !o) {
        set_err("gp_get_info: null argument");
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(s->host_ctl, s->slab[0].S.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    o->population = s->P;
    o->threshold = s->T;
    o->grid = s->g;
    o->seed_node = s->slab[0].S.seed_node;
    o->rounds = s->rounds_done;
    o->alerts_total = s->alerts_total;
    o->active = s->slab[0].S.alg == PUSHSUM ? (int64_t)s->host_ctl->active_total : -1;
    o->topology = s->cfg.topology;
    o->algorithm = s->cfg.algorithm;
    o->device = s->device;
    o->num_gpus = s->world;
    if (s->mode == MODE_RCCL) {
        o->slab_first = s->slab[0].S.lo;
        o->slab_count = s->slab[0].S.nloc;
    } else {
        o->slab_first = 0;
        o->slab_count = s->P;
    }
    return GP_OK;
}

#ifdef GP_EXPERIMENTS
// Experiments build, tests: round kernel launches per round (DevState::rregions), -1 without a handle.
int gp_debug_round_regions(gp_sim* s) { return s && !s->slab.empty() ? (int)s->slab[0].S.rregions : -1; }
#endif

int gp_sync(gp_sim* s) {
    if (!s) {
        set_err("gp_sync: null handle");
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GP_OK;
}

int gp_kernel_stats(gp_sim* s, double* total_ms, int64_t* launches, char* name, int32_t name_cap, int32_t reset) {
    if (!s) {
        set_err("gp_kernel_stats: null handle");
        return GP_EINVAL;
    }
    if (total_ms) *total_ms = s->kernel_ms;
    if (launches) *launches = s->launches;
    if (name && name_cap > 0) {
        const DevState& S = s->slab[0].S;
        // (GP_GRID, experiments: the grid the tiled round kernels run on after the name, as
        // k_ps_tile<IMP3D>@8 -- the tests' proof that the override reached kernel_plan)
        if (s->kplan.grid_override)
            std::snprintf(name, (size_t)name_cap, "%s@%d", bulk_kernel_name(S), s->grid);
        else std::snprintf(name, (size_t)name_cap, "%s", bulk_kernel_name(S));
    }
    if (reset) {
        s->kernel_ms = 0.0;
        s->launches = 0;
    }
    return GP_OK;
}

double gp_alg_bytes_per_node(gp_sim* s) { return s ? alg_bytes(s) : 0.0; }

void gp_destroy(gp_sim* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->xstream) (void)hipStreamSynchronize(s->xstream);
    for (auto& e : s->ev) (void)hipEventDestroy(e);
    for (int h = 0; h < XMAXH; ++h) {
        if (s->ev_send[h]) (void)hipEventDestroy(s->ev_send[h]);
        if (s->ev_xfer[h]) (void)hipEventDestroy(s->ev_xfer[h]);
    }
    if (s->comm) (void)ncclCommDestroy(s->comm);
    for (void* p : s->allocs) (void)hipFree(p);
    values_stage_free(s->vstage);
    if (s->host_ctl) (void)hipHostFree(s->host_ctl);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    if (s->xstream) (void)hipStreamDestroy(s->xstream);
    delete s;
}

}  // extern "C"
