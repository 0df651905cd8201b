// gp_ensemble_api.hip -- C-ABI of ensemble runs (include/gossip_hip.h, gp_ensemble_*):
// argument checks, the members' stored state in HBM, and the launch loop that hands
// the unfinished members to gp_ensemble.hip in chunks of rounds.  DESIGN.md §9.
#include <new>

#include "gp_host.hpp"
#include "gp_ensemble.hpp"
#include "gp_graph.hpp"
#pragma GCC visibility push(hidden)
#include "gp_summary_dev.hpp"
#pragma GCC visibility pop

namespace {

// Rounds one launch may run.  Every kernel loop is bounded by its launch's round
// count, and a launch should stay well under a second.  Measured on an MI355X
// (DESIGN.md §9.4, 256 members): a round takes 0.5-4.4 us at n = 1000 and 2.2-40 us
// at the population cap (8 node slots per thread; slowest: Imp3D push-sum, 5832
// nodes), so 8192 rounds are 4-36 ms at n = 1000 and at most 0.33 s at the cap,
// while the longest runs of the report's range (line push-sum, ~13000 rounds) still
// take only two launches.  When there are more members than CUs (256; a CU holds at
// least one workgroup), the workgroups run in waves, so the chunk shrinks by the
// number of waves, down to a floor of 256 rounds, below which the launch overhead
// (~10 us and the record copy) would show.
// The failure kernels keep the constant: measured at their own caps,
// 256 members, the slowest round is 43.5 us (Imp3D push-sum, 5832 nodes), so 8192
// rounds are at most 0.36 s.
constexpr int64_t ENS_LAUNCH_ROUNDS = 8192;
constexpr int64_t ENS_LAUNCH_ROUNDS_MIN = 256;
constexpr int64_t ENS_CUS = 256;

int64_t launch_rounds(size_t members) {
    const int64_t waves = ((int64_t)members + ENS_CUS - 1) / ENS_CUS;
    return std::max(ENS_LAUNCH_ROUNDS_MIN, ENS_LAUNCH_ROUNDS / std::max<int64_t>(1, waves));
}

bool pair_ok(int32_t topology, int32_t algorithm) {
    if (topology < GP_LINE || topology > GP_IMP3D) {
        set_err("unknown topology id %d", topology);
        return false;
    }
    if (algorithm != GP_GOSSIP && algorithm != GP_PUSHSUM) {
        set_err("unknown algorithm id %d", algorithm);
        return false;
    }
    return true;
}

// SRS v1-G: the LDS image of a member on `graph` (gp_ensemble_shape.hpp), or -1 with the message set when
// the graph is inadmissible (gp_graph.hpp) or its image does not fit.  Host only.
int64_t graph_image(const gp_graph* graph, int32_t algorithm, EnsVariant v) {
    std::string why;
    if (graph_validate(graph, (int64_t)ENS_GRAPH_POP_MAX, &why) != GRAPH_OK) {
        set_err("%s", why.c_str());
        return -1;
    }
    const int64_t e_in = graph_in_entries(graph);
    const uint64_t bytes =
        ens_graph_lds_bytes(algorithm, (uint64_t)graph->num_nodes, (uint64_t)graph->num_edges, (uint64_t)e_in, v);
    if (bytes > ENS_LDS_MAX) {
        set_err("graph: the LDS image of %lld nodes, %lld out-entries and %lld in-entries takes %llu bytes%s%s, more than "
                "the %u a member may take (the adjacency must fit in one workgroup's LDS)",
                (long long)graph->num_nodes, (long long)graph->num_edges, (long long)e_in, (unsigned long long)bytes,
                v.faults ? ", failure layout" : "", v.trace ? ", trace layout" : "", ENS_LDS_MAX);
        return -1;
    }
    return (int64_t)bytes;
}

// A trace buffer may take this much HBM (nseeds x capacity rows of 32 bytes).
constexpr int64_t ENS_TRACE_BYTES_MAX = 1ll << 30;

// p in [0, 1] -> q = floor(p * 2^32), exact in double; an event happens iff x < q.
uint64_t fault_threshold(double p) { return (uint64_t)std::floor(p * 4294967296.0); }

}  // namespace

struct gp_ensemble {
    gp_config cfg{};
    int64_t P = 0, T = 0, g = 0;
    int64_t nseeds = 0;
    uint32_t nwords = 0;
    hipStream_t stream = nullptr;
    // v.faults: failure model (gp_ensemble_create_faults; SRS v1-F), parameters in args.f;
    // v.trace: trace (gp_ensemble_create_traced; SRS v1-T), in args.t with the capacity
    // resolved (never 0 for "everything"); the rows stay on the device until read
    EnsVariant v{};
    EnsArgs args{};
    uint32_t* d_idx = nullptr;
    std::vector<void*> allocs;
    std::vector<gp_member> rec;    // host copy of the member records, refreshed after every launch
    std::vector<uint32_t> running; // unfinished members, in member order
    SumAcc* d_sum = nullptr;       // gp_ensemble_summary: one record per member, allocated at the first call
    std::vector<EnsFaultRec> frec; // v.faults: host copy of args.f.frec, refreshed after every launch
    double mean = 0.0;             // mu of the summaries and the trace: (P - 1) / 2 unless values were given (SRS v1-V)
    GraphCsr csr;                  // GP_GRAPH: the two CSRs until they are uploaded (SRS v1-G)
    uint32_t graph_lds = 0;        // GP_GRAPH: the member's LDS image, adjacency included
};

namespace {

template <typename T>
int ens_alloc(gp_ensemble* e, T** p, size_t count) {
    void* v = nullptr;
    const size_t bytes = std::max<size_t>(16, count * sizeof(T));
    const hipError_t err = hipMalloc(&v, bytes);
    if (err != hipSuccess) {
        set_err("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(err));
        return GP_ENOMEM;
    }
    e->allocs.push_back(v);
    *p = static_cast<T*>(v);
    return GP_OK;
}

// One launch over the running members: up to nrounds rounds each (init: set them up
// from their seeds instead).  Refreshes the records and the running list.
int launch(gp_ensemble* e, int64_t nrounds, bool init) {
    const size_t n = e->running.size();
    HIP_TRY(hipMemcpyAsync(e->d_idx, e->running.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    e->args.nrounds = nrounds;
    e->args.init = init ? 1 : 0;
    HIP_TRY(ens_launch(e->v, e->cfg.topology, e->cfg.algorithm, e->args, (uint32_t)n, e->stream));
    if (e->v.faults)
        HIP_TRY(hipMemcpyAsync(e->frec.data(), e->args.f.frec, e->frec.size() * sizeof(EnsFaultRec),
                                   hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(e->rec.data(), e->args.rec, e->rec.size() * sizeof(gp_member), hipMemcpyDeviceToHost,
                               e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    size_t keep = 0;
    for (size_t q = 0; q < n; ++q)
        if (e->rec[e->running[q]].status == GP_STATUS_RUNNING) e->running[keep++] = e->running[q];
    e->running.resize(keep);
    return GP_OK;
}

// One array of a CSR onto the device, padded with zeros to the multiple of 8 bytes the kernels stage.
template <typename T>
int upload_padded(gp_ensemble* e, const T** dev, std::vector<T>& host) {
    host.resize((ens_up8((uint32_t)(host.size() * sizeof(T)))) / sizeof(T), T(0));
    T* d = nullptr;
    const int rc = ens_alloc(e, &d, host.size());
    if (rc) return rc;
    if (!host.empty())
        HIP_TRY(hipMemcpyAsync(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, e->stream));
    *dev = d;
    return GP_OK;
}

// GP_GRAPH: both CSRs go up once; every launch stages them from there into LDS.
int upload_graph(gp_ensemble* e) {
    EnsArgs& a = e->args;
    GraphCsr& c = e->csr;
    a.g_eout = (uint32_t)c.out_nbr.size();
    a.g_ein = (uint32_t)c.in_nbr.size();
    int rc = upload_padded(e, &a.g_out_off, c.out_off);
    if (!rc) rc = upload_padded(e, &a.g_out_nbr, c.out_nbr);
    if (!rc) rc = upload_padded(e, &a.g_in_off, c.in_off);
    if (!rc) rc = upload_padded(e, &a.g_in_nbr, c.in_nbr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (the host copies go away)
    c = GraphCsr{};
    return GP_OK;
}

int create(gp_ensemble* e, const uint64_t* seeds, const gp_values* values) {
    const int topo = e->cfg.topology, alg = e->cfg.algorithm;
    const size_t n = (size_t)e->nseeds, P = (size_t)e->P;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIP_TRY(ens_setup(e->v, topo, alg, (uint32_t)P, e->graph_lds));
    EnsArgs& a = e->args;
    int rc = ens_alloc(e, &a.rec, n);
    if (!rc && topo == GP_GRAPH) rc = upload_graph(e);
    if (!rc && e->v.trace) {
        // (the kernels write a row before anybody may read it, and the set-up launch every record)
        rc = ens_alloc(e, &a.t.rows, n * (size_t)a.t.capacity);
        if (!rc) rc = ens_alloc(e, &a.t.trec, n);
    }
    if (!rc && e->v.faults) {
        rc = ens_alloc(e, &a.f.frec, n);
        e->frec.assign(n, EnsFaultRec{});  // (the set-up launch writes every record)
    }
    if (!rc) rc = ens_alloc(e, &e->d_idx, n);
    if (alg == GP_GOSSIP) {
        if (!rc) rc = ens_alloc(e, &a.c, n * P);
        if (!rc && topo != GP_FULL) rc = ens_alloc(e, &a.bits, n * e->nwords);
    } else {
        if (!rc) rc = ens_alloc(e, &a.s, n * P);
        if (!rc) rc = ens_alloc(e, &a.w, n * P);
        if (!rc) rc = ens_alloc(e, &a.fl, n * P);
    }
    if (rc) return rc;
    if (values) {  // SRS v1-V: checked on the device (gp_values.hip), then kept for the set-up launch
        double *x0 = nullptr, *w0 = nullptr;
        if ((rc = ens_alloc(e, &x0, P)) || (values->w && (rc = ens_alloc(e, &w0, P)))) return rc;
        struct Sink : ValSink {  // the staged chunk, once it has passed the check, into the two arrays
            double *x0, *w0;
            int write(const void* staged, bool weighted, int64_t c0, int64_t c1, hipStream_t st) override {
                HIP_TRY(launch_values_split(staged, weighted, (uint32_t)(c1 - c0), x0 + c0, weighted ? w0 + c0 : nullptr,
                                            (int)ENS_CUS, st));
                return GP_OK;
            }
        } sink;
        sink.x0 = x0;
        sink.w0 = w0;
        ValStage stage;
        rc = values_stream(stage, e->stream, (int)ENS_CUS, "gp_ensemble_create_values", values->x, values->w, (int64_t)P,
                           0, &sink);
        values_stage_free(stage);
        if (rc) return rc;
        a.x0 = x0;
        a.w0 = w0;
    }
    a.mu = e->mean;
    a.idx = e->d_idx;
    a.G = Geom{};
    a.G.P = (uint32_t)e->P;
    a.G.T = (uint32_t)e->T;
    a.G.g = (uint32_t)e->g;
    a.G.g2 = (uint32_t)(e->g * e->g);
    a.G.div_g = make_fastdiv(a.G.g);
    a.G.div_g2 = make_fastdiv(a.G.g2);
    a.nwords = e->nwords;
    a.max_rounds = e->cfg.max_rounds;
    e->rec.assign(n, gp_member{});
    e->running.resize(n);
    for (size_t m = 0; m < n; ++m) {
        e->rec[m].seed = seeds[m];
        e->rec[m].status = GP_STATUS_RUNNING;
        e->running[m] = (uint32_t)m;
    }
    HIP_TRY(hipMemcpyAsync(a.rec, e->rec.data(), n * sizeof(gp_member), hipMemcpyHostToDevice, e->stream));
    return launch(e, 0, true);
}

}  // namespace

extern "C" {

// The caps are a function of the LDS layout (ens_max_nodes: a few thousand integer steps on the host).
int64_t gp_ensemble_max_nodes(int32_t topology, int32_t algorithm) {
    return pair_ok(topology, algorithm) ? ens_max_nodes(topology, algorithm, EnsVariant{false, false}) : GP_EINVAL;
}

// gp_ensemble_create_faults' checks of the failure model.
static int faults_ok(const char* who, const gp_faults* faults) {
    // (the negated comparisons also refuse NaN)
    if (!(faults->node_fail >= 0.0 && faults->node_fail <= 1.0)) {
        set_err("%s: node_fail must be in [0, 1] (got %g)", who, faults->node_fail);
        return GP_EINVAL;
    }
    if (!(faults->msg_drop >= 0.0 && faults->msg_drop <= 1.0)) {
        set_err("%s: msg_drop must be in [0, 1] (got %g)", who, faults->msg_drop);
        return GP_EINVAL;
    }
    if (faults->fail_round < 0) {
        set_err("%s: fail_round must be >= 0 (got %lld)", who, (long long)faults->fail_round);
        return GP_EINVAL;
    }
    if (faults->reserved != 0) {
        set_err("%s: reserved must be 0 (got %lld)", who, (long long)faults->reserved);
        return GP_EINVAL;
    }
    return GP_OK;
}

// gp_ensemble_create_traced's checks of the trace configuration.
static int trace_ok(const char* who, const gp_trace_cfg* trace) {
    if (trace->stride < 1) {
        set_err("%s: stride must be >= 1 (got %lld)", who, (long long)trace->stride);
        return GP_EINVAL;
    }
    if (trace->capacity < 0) {
        set_err("%s: capacity must be >= 0 (got %lld)", who, (long long)trace->capacity);
        return GP_EINVAL;
    }
    if (trace->reserved[0] != 0 || trace->reserved[1] != 0) {
        set_err("%s: reserved must be 0 (got %lld, %lld)", who, (long long)trace->reserved[0],
                (long long)trace->reserved[1]);
        return GP_EINVAL;
    }
    return GP_OK;
}

// gp_ensemble_create, gp_ensemble_create_faults (faults != null) and gp_ensemble_create_traced
// (trace != null), their own arguments already checked.
// values != null: gp_ensemble_create_values, its own fields but count already checked.
// graph != null: gp_ensemble_create_graph, cfg->topology == GP_GRAPH already checked; the graph is checked here.
static int ensemble_create(const gp_config* cfg, const gp_values* values, const gp_faults* faults,
                           const gp_trace_cfg* trace, const uint64_t* seeds, int64_t nseeds, gp_ensemble** out,
                           const gp_graph* graph = nullptr) {
    if (!seeds) {
        set_err("gp_ensemble_create: seeds is null");
        return GP_EINVAL;
    }
    if (nseeds <= 0 || nseeds > 0x7FFFFFFFll) {
        set_err("gp_ensemble_create: nseeds must be in [1, 2^31) (got %lld)", (long long)nseeds);
        return GP_EINVAL;
    }
    if (cfg->num_gpus != 1 || (cfg->flags & GP_FLAG_VIRTUAL_RANKS)) {
        set_err("gp_ensemble_create: an ensemble runs on one GPU (num_gpus = %d, flags = %d)", cfg->num_gpus, cfg->flags);
        return GP_EINVAL;
    }
    if (cfg->max_rounds <= 0) {
        set_err("gp_ensemble_create: max_rounds must be > 0 (an ensemble needs an explicit cap)");
        return GP_EINVAL;
    }
    if (!pair_ok(graph ? GP_LINE : cfg->topology, cfg->algorithm)) return GP_EINVAL;
    const EnsVariant v{faults != nullptr, trace != nullptr};
    int64_t P = 0, T = 0, g = 0;
    int64_t graph_lds = 0;
    if (graph) {  // SRS v1-G: P = T = the graph's nodes, no extra actor
        graph_lds = graph_image(graph, cfg->algorithm, v);
        if (graph_lds < 0) return GP_EINVAL;
        if (cfg->num_nodes != graph->num_nodes) {
            set_err("gp_ensemble_create_graph: cfg.num_nodes %lld is not the graph's num_nodes %lld",
                    (long long)cfg->num_nodes, (long long)graph->num_nodes);
            return GP_EINVAL;
        }
        P = T = graph->num_nodes;
    } else if (gp_resolve(cfg->num_nodes, cfg->topology, &P, &T, &g)) {
        return GP_EINVAL;
    }
    if (P < 2) {
        set_err("gp_ensemble_create: a population of %lld has no edge", (long long)P);
        return GP_EINVAL;
    }
    if (values && values->count != P) {
        set_err("gp_ensemble_create_values: count %lld is not the population %lld", (long long)values->count, (long long)P);
        return GP_EINVAL;
    }
    const int64_t cap = graph ? (int64_t)ENS_GRAPH_POP_MAX : ens_max_nodes(cfg->topology, cfg->algorithm, v);
    if (cfg->num_nodes > cap) {
        set_err("gp_ensemble_create: num_nodes %lld exceeds the ensemble cap %lld of this pair (one workgroup's LDS%s%s); "
                "use gp_create", (long long)cfg->num_nodes, (long long)cap, faults ? ", failure layout" : "",
                trace ? ", trace layout" : "");
        return GP_EINVAL;
    }
    int64_t capacity = 0;
    if (trace) {
        capacity = trace->capacity ? trace->capacity : cfg->max_rounds / trace->stride;
        const int64_t rows_max = ENS_TRACE_BYTES_MAX / (int64_t)sizeof(gp_trace_row) / nseeds;
        if (capacity > rows_max) {
            // floor(max_rounds / stride) <= rows_max  <=>  stride >= floor(max_rounds / (rows_max + 1)) + 1
            set_err("gp_ensemble_create_traced: %lld members x %lld rows x %zu bytes exceed the trace buffer's 1 GiB; "
                    "at most %lld rows per member fit: the smallest stride that records every row (capacity 0) is %lld",
                    (long long)nseeds, (long long)capacity, sizeof(gp_trace_row), (long long)rows_max,
                    (long long)(cfg->max_rounds / (rows_max + 1) + 1));
            return GP_EINVAL;
        }
    }
    const int rc_dev = check_device(cfg->device);
    if (rc_dev) return rc_dev;

    gp_ensemble* e = new (std::nothrow) gp_ensemble();
    if (!e) {
        set_err("out of host memory");
        return GP_ENOMEM;
    }
    e->cfg = *cfg;
    e->P = P;
    e->T = T;
    e->g = g;
    e->nseeds = nseeds;
    e->nwords = (uint32_t)((T + 31) / 32);
    e->v = v;
    e->mean = values ? values->mean : (double)(P - 1) * 0.5;
    if (graph) {
        graph_build(graph, &e->csr);
        e->graph_lds = (uint32_t)graph_lds;
    }
    if (faults) {
        e->args.f.q_node = fault_threshold(faults->node_fail);
        e->args.f.q_drop = fault_threshold(faults->msg_drop);
        e->args.f.fail_round = faults->fail_round;
    }
    if (trace) {
        e->args.t.stride = trace->stride;
        e->args.t.capacity = capacity;
    }
    const int rc = create(e, seeds, values);
    if (rc) {
        gp_ensemble_destroy(e);  // (hipFree does not touch the error message)
        return rc;
    }
    *out = e;
    return GP_OK;
}

int gp_ensemble_create(const gp_config* cfg, const uint64_t* seeds, int64_t nseeds, gp_ensemble** out) {
    if (!cfg || !out) {
        set_err("gp_ensemble_create: null argument");
        return GP_EINVAL;
    }
    *out = nullptr;
    return ensemble_create(cfg, nullptr, nullptr, nullptr, seeds, nseeds, out);
}

int64_t gp_ensemble_faults_max_nodes(int32_t topology, int32_t algorithm) {
    return pair_ok(topology, algorithm) ? ens_max_nodes(topology, algorithm, EnsVariant{true, false}) : GP_EINVAL;
}

int gp_ensemble_create_faults(const gp_config* cfg, const gp_faults* faults, const uint64_t* seeds, int64_t nseeds,
                              gp_ensemble** out) {
    if (!cfg || !out) {
        set_err("gp_ensemble_create_faults: null argument");
        return GP_EINVAL;
    }
    *out = nullptr;
    if (!faults) {
        set_err("gp_ensemble_create_faults: faults is null");
        return GP_EINVAL;
    }
    if (faults_ok("gp_ensemble_create_faults", faults)) return GP_EINVAL;
    return ensemble_create(cfg, nullptr, faults, nullptr, seeds, nseeds, out);
}

int64_t gp_ensemble_trace_max_nodes(int32_t topology, int32_t algorithm, int32_t faults) {
    return pair_ok(topology, algorithm) ? ens_max_nodes(topology, algorithm, EnsVariant{faults != 0, true}) : GP_EINVAL;
}

int gp_ensemble_create_traced(const gp_config* cfg, const gp_faults* faults, const gp_trace_cfg* trace,
                              const uint64_t* seeds, int64_t nseeds, gp_ensemble** out) {
    if (!cfg || !out) {
        set_err("gp_ensemble_create_traced: null argument");
        return GP_EINVAL;
    }
    *out = nullptr;
    if (!trace) {
        set_err("gp_ensemble_create_traced: trace is null");
        return GP_EINVAL;
    }
    if (trace_ok("gp_ensemble_create_traced", trace)) return GP_EINVAL;
    if (faults && faults_ok("gp_ensemble_create_traced", faults)) return GP_EINVAL;
    return ensemble_create(cfg, nullptr, faults, trace, seeds, nseeds, out);
}

// gp_ensemble_create_values' checks of the values' own fields (count and entries are checked later).
static int values_ok(const char* who, const gp_config* cfg, const gp_values* values) {
    if (!values->x) {
        set_err("%s: values.x is null", who);
        return GP_EINVAL;
    }
    if (values->reserved != 0) {
        set_err("%s: reserved must be 0 (got %lld)", who, (long long)values->reserved);
        return GP_EINVAL;
    }
    if (!mean_ok(values->mean)) {
        set_err("%s: mean must be finite, >= 0 and < 2^32 (got %g)", who, values->mean);
        return GP_EINVAL;
    }
    if (cfg->algorithm == GP_GOSSIP) {
        set_err("%s: gossip has no values (cfg.algorithm is gossip)", who);
        return GP_EINVAL;
    }
    return GP_OK;
}

int gp_ensemble_create_values(const gp_config* cfg, const gp_values* values, const gp_faults* faults,
                              const gp_trace_cfg* trace, const uint64_t* seeds, int64_t nseeds, gp_ensemble** out) {
    const char* who = "gp_ensemble_create_values";
    if (!cfg || !out) {
        set_err("%s: null argument", who);
        return GP_EINVAL;
    }
    *out = nullptr;
    if (!values) {
        set_err("%s: values is null", who);
        return GP_EINVAL;
    }
    if (values_ok(who, cfg, values)) return GP_EINVAL;
    if (trace && trace_ok(who, trace)) return GP_EINVAL;
    if (faults && faults_ok(who, faults)) return GP_EINVAL;
    return ensemble_create(cfg, values, faults, trace, seeds, nseeds, out);
}

int64_t gp_ensemble_graph_lds_bytes(const gp_graph* graph, int32_t algorithm, int32_t faults, int32_t trace) {
    if (!pair_ok(GP_LINE, algorithm)) return GP_EINVAL;
    const int64_t bytes = graph_image(graph, algorithm, EnsVariant{faults != 0, trace != 0});
    return bytes < 0 ? GP_EINVAL : bytes;
}

int gp_ensemble_create_graph(const gp_config* cfg, const gp_graph* graph, const gp_values* values,
                             const gp_faults* faults, const gp_trace_cfg* trace, const uint64_t* seeds, int64_t nseeds,
                             gp_ensemble** out) {
    const char* who = "gp_ensemble_create_graph";
    if (!cfg || !out) {
        set_err("%s: null argument", who);
        return GP_EINVAL;
    }
    *out = nullptr;
    if (!graph) {
        set_err("%s: graph is null", who);
        return GP_EINVAL;
    }
    if (cfg->topology != GP_GRAPH) {
        set_err("%s: cfg.topology must be GP_GRAPH (got %d)", who, cfg->topology);
        return GP_EINVAL;
    }
    if (values && values_ok(who, cfg, values)) return GP_EINVAL;
    if (trace && trace_ok(who, trace)) return GP_EINVAL;
    if (faults && faults_ok(who, faults)) return GP_EINVAL;
    return ensemble_create(cfg, values, faults, trace, seeds, nseeds, out, graph);
}

// Rows member m has recorded: a pure function of its record, no counter lives on the device.
static int64_t trace_rows_of(const gp_ensemble* e, size_t m) {
    return std::min(e->args.t.capacity, e->rec[m].rounds / e->args.t.stride);
}

int gp_ensemble_trace_rows(gp_ensemble* e, int64_t* rows_out) {
    if (!e || !rows_out) {
        set_err("gp_ensemble_trace_rows: null argument");
        return GP_EINVAL;
    }
    if (!e->v.trace) {
        set_err("gp_ensemble_trace_rows: the ensemble records no trace (gp_ensemble_create_traced does)");
        return GP_ESTATE;
    }
    for (int64_t m = 0; m < e->nseeds; ++m) rows_out[m] = trace_rows_of(e, (size_t)m);
    return GP_OK;
}

int gp_ensemble_trace_read(gp_ensemble* e, int64_t member, int64_t first, int64_t count, gp_trace_row* out) {
    if (!e) {
        set_err("gp_ensemble_trace_read: null handle");
        return GP_EINVAL;
    }
    if (!e->v.trace) {
        set_err("gp_ensemble_trace_read: the ensemble records no trace (gp_ensemble_create_traced does)");
        return GP_ESTATE;
    }
    if (member < 0 || member >= e->nseeds) {
        set_err("gp_ensemble_trace_read: member %lld outside %lld members", (long long)member, (long long)e->nseeds);
        return GP_EINVAL;
    }
    const int64_t have = trace_rows_of(e, (size_t)member);
    if (first < 0 || count < 0 || first > have || count > have - first) {
        set_err("gp_ensemble_trace_read: rows [%lld, +%lld) outside the %lld rows member %lld has recorded",
                (long long)first, (long long)count, (long long)have, (long long)member);
        return GP_EINVAL;
    }
    if (count == 0) return GP_OK;
    if (!out) {
        set_err("gp_ensemble_trace_read: out is null");
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    const gp_trace_row* src = e->args.t.rows + ((size_t)member * (size_t)e->args.t.capacity + (size_t)first);
    HIP_TRY(hipMemcpyAsync(out, src, (size_t)count * sizeof(gp_trace_row), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return GP_OK;
}

int gp_ensemble_fault_stats(gp_ensemble* e, gp_fault_stats* out) {
    if (!e || !out) {
        set_err("gp_ensemble_fault_stats: null argument");
        return GP_EINVAL;
    }
    for (int64_t m = 0; m < e->nseeds; ++m) {
        gp_fault_stats& o = out[m];
        o = gp_fault_stats{0, 0, e->T, 0};
        if (!e->v.faults) continue;
        const EnsFaultRec& f = e->frec[(size_t)m];
        o.doomed = f.doomed;
        o.down = e->rec[(size_t)m].rounds >= e->args.f.fail_round ? f.doomed : 0;
        o.threshold = std::max<int64_t>(1, e->T - f.doomed);
        o.lost = f.lost;
    }
    return GP_OK;
}

int64_t gp_ensemble_step(gp_ensemble* e, int64_t nrounds) {
    if (!e || nrounds < 0) {
        set_err("gp_ensemble_step: bad argument");
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    while (nrounds > 0 && !e->running.empty()) {
        const int64_t chunk = std::min(nrounds, launch_rounds(e->running.size()));
        const int rc = launch(e, chunk, false);
        if (rc) return rc;
        nrounds -= chunk;
    }
    return (int64_t)e->running.size();
}

int gp_ensemble_members(gp_ensemble* e, gp_member* out) {
    if (!e || !out) {
        set_err("gp_ensemble_members: null argument");
        return GP_EINVAL;
    }
    for (int64_t m = 0; m < e->nseeds; ++m) {
        out[m] = e->rec[(size_t)m];
        out[m].reserved = 0;
    }
    return GP_OK;
}

int gp_ensemble_run(gp_ensemble* e, gp_member* out) {
    if (!e) {
        set_err("gp_ensemble_run: null handle");
        return GP_EINVAL;
    }
    // every member stops at max_rounds (> 0) at the latest
    while (!e->running.empty()) {
        const int64_t left = gp_ensemble_step(e, ENS_LAUNCH_ROUNDS);
        if (left < 0) return (int)left;
    }
    return out ? gp_ensemble_members(e, out) : GP_OK;
}

int gp_ensemble_read_state(gp_ensemble* e, int64_t member, int64_t first, int64_t count, int32_t* c, double* s,
                           double* w, uint8_t* flags) {
    if (!e) {
        set_err("gp_ensemble_read_state: null handle");
        return GP_EINVAL;
    }
    if (member < 0 || member >= e->nseeds || first < 0 || count < 0 || first + count > e->P) {
        set_err("gp_ensemble_read_state: member %lld range [%lld, %lld) outside %lld members of %lld nodes",
                (long long)member, (long long)first, (long long)(first + count), (long long)e->nseeds, (long long)e->P);
        return GP_EINVAL;
    }
    if (count == 0) return GP_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t at = (size_t)member * (size_t)e->P + (size_t)first, n = (size_t)count;
    // Failure ensembles: is node first + q down at the member's round count?  D is a pure
    // function of the seed, recomputed here with the kernels' own draw.
    const gp_member& mr = e->rec[(size_t)member];
    const bool any_down = e->v.faults && mr.rounds >= e->args.f.fail_round;
    auto down = [&](size_t q) {
        return any_down && ens_doomed((uint32_t)mr.seed, (uint32_t)(mr.seed >> 32), (uint32_t)(first + (int64_t)q),
                                      (uint32_t)mr.seed_node, e->args.f.q_node);
    };
    if (e->cfg.algorithm == GP_GOSSIP) {
        std::vector<int32_t> hc(n);
        HIP_TRY(hipMemcpyAsync(hc.data(), e->args.c + at, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const int64_t seed_node = e->rec[(size_t)member].seed_node;
        for (size_t q = 0; q < n; ++q) {
            const int32_t ci = hc[q];
            if (c) c[q] = ci;
            if (s) s[q] = 0.0;
            if (w) w[q] = 0.0;
            if (flags) {
                const int act = ((int64_t)(first + (int64_t)q) == seed_node || ci >= 1) && ci <= 10;
                flags[q] = (uint8_t)(act | ((ci >= (int32_t)GOSSIP_DONE) << 1));
                if (down(q)) flags[q] = (uint8_t)((flags[q] & ~1u) | GP_STATE_DOWN);  // a down node is not active
            }
        }
    } else {
        if (s) HIP_TRY(hipMemcpyAsync(s, e->args.s + at, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (w) HIP_TRY(hipMemcpyAsync(w, e->args.w + at, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (flags) HIP_TRY(hipMemcpyAsync(flags, e->args.fl + at, n, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (flags && any_down)
            for (size_t q = 0; q < n; ++q)
                if (down(q)) flags[q] |= GP_STATE_DOWN;  // (its active bit stays frozen as it was)
        if (c) std::fill(c, c + n, 0);
    }
    return GP_OK;
}

int gp_ensemble_summary(gp_ensemble* e, double tol, gp_summary* out) {
    if (!e || !out) {
        set_err("gp_ensemble_summary: null argument");
        return GP_EINVAL;
    }
    if (!(tol >= 0.0) || !std::isfinite(tol)) {
        set_err("gp_ensemble_summary: tol must be finite and >= 0 (got %g)", tol);
        return GP_EINVAL;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t n = (size_t)e->nseeds;
    if (!e->d_sum) {
        const int rc = ens_alloc(e, &e->d_sum, n);
        if (rc) return rc;
    }
    // the members' stored state (every launch leaves it in HBM), one workgroup per member
    SumEnsArgs a{};
    a.c = e->args.c;
    a.s = e->args.s;
    a.w = e->args.w;
    a.fl = e->args.fl;
    a.rec = e->args.rec;
    a.P = (uint32_t)e->P;
    a.mu = e->mean;
    a.tol = tol;
    a.out = e->d_sum;
    const int alg = e->cfg.algorithm == GP_PUSHSUM ? PUSHSUM : GOSSIP;
    HIP_TRY(summary_ens_launch(alg, a, (uint32_t)n, e->stream));
    std::vector<SumAcc> h(n);
    HIP_TRY(hipMemcpyAsync(h.data(), e->d_sum, n * sizeof(SumAcc), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t m = 0; m < n; ++m) summary_from_acc(h[m], alg, 0, e->P, e->P, e->rec[m].rounds, tol, &out[m]);
    return GP_OK;
}

void gp_ensemble_destroy(gp_ensemble* e) {
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
}

}  // extern "C"
