/*
 * gossip_hip.h -- C-ABI of libgossip_hip.so, the MI355X-native replacement for
 * the gossip / push-sum hot path of sharwarimarathe/GossipProtocol.
 *
 * The reference has no plugin or operator API: its only caller of the path is
 * `main` in /root/reference/Project2/Program.fs (cited below as Program.fs:N),
 * driven by the CLI `dotnet run <num_nodes> <topology> <algorithm>`
 * (README.md:1, argv parse Program.fs:32-34).  Each entry point below names the
 * block of Program.fs it replaces; a front-end keeps the argv/stdout contract
 * and binds these symbols (F# P/Invoke stub: INTEGRATION.md).
 *
 * Conventions: plain C types and blittable structs only (no torch or HIP
 * types), return 0 on success or a negative GP_E* code; gp_last_error() holds
 * the message for the calling thread.  The library owns all device memory and
 * streams; the caller owns cfg/out/readback buffers.  A gp_sim is not
 * reentrant: one caller thread per handle.
 *
 * Semantics: the synchronous-round specification SRS v1 (SURVEY.md Appendix
 * B).  Randomness is Philox4x32-10 keyed by cfg.seed, so runs are
 * reproducible and bit-identical to the CPU oracle.
 */
#ifndef GOSSIP_HIP_H
#define GOSSIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_VERSION 10100 /* 1.1.0 */
/* Largest population (node ids are 32-bit; tiles of 1024 ids must not wrap). */
#define GP_MAX_POPULATION 0xFFFFF000u

/* topology strings "line" | "full" | "3D" | "Imp3D" (Program.fs:180,209,238,258) */
enum { GP_LINE = 0, GP_FULL = 1, GP_3D = 2, GP_IMP3D = 3,
       GP_GRAPH = 4 /* a caller-supplied graph: gp_ensemble_create_graph only; every other entry point
                       that takes a topology refuses it like an unknown value, and it has no string */ };
/* algorithm strings "gossip" | "push-sum" (Program.fs:196,202) */
enum { GP_GOSSIP = 0, GP_PUSHSUM = 1 };
/* gp_result.status */
enum { GP_STATUS_CONVERGED = 0, GP_STATUS_MAX_ROUNDS = 1, GP_STATUS_RUNNING = 2 };
/* error codes */
enum {
    GP_OK = 0,
    GP_EINVAL = -1,    /* bad argument / unknown topology or algorithm */
    GP_ENOMEM = -2,    /* host or device allocation failed */
    GP_EHIP = -3,      /* HIP runtime error */
    GP_ENCCL = -4,     /* RCCL error */
    GP_ESTATE = -5,    /* call not valid in the handle's state */
    GP_ENODEV = -6     /* no usable gfx950 device */
};
/* gp_config.flags */
enum {
    GP_FLAG_KERNEL_TIMING = 1, /* bracket every round kernel with HIP events (gp_kernel_stats) */
    GP_FLAG_VIRTUAL_RANKS = 2  /* num_gpus > 1 slabs in this process on `device` (the multi-GPU
                                  exchange with device copies instead of RCCL; for testing) */
};

typedef struct gp_sim gp_sim;

/* Replaces Program.fs:32-34 (argv) plus the constants the reference hard-codes. */
typedef struct gp_config {
    int64_t num_nodes;   /* argv[0]: `nodes` (Program.fs:32) */
    int32_t topology;    /* GP_LINE .. GP_IMP3D (argv[1], Program.fs:33) */
    int32_t algorithm;   /* GP_GOSSIP | GP_PUSHSUM (argv[2], Program.fs:34) */
    uint64_t seed;       /* Philox key; replaces `new Random()` (Program.fs:86 et al.) */
    int32_t num_gpus;    /* 1; multi-GPU runs one process per GPU (gp_create_rank; launchers:
                            `gossip --gpus N` / GOSSIP_GPUS, bench.py --gpus N), or num_gpus
                            in-process slabs with GP_FLAG_VIRTUAL_RANKS */
    int32_t device;      /* HIP device ordinal for num_gpus == 1 */
    int64_t max_rounds;  /* cap; <= 0 means unlimited (the reference blocks forever, Program.fs:282) */
    int32_t flags;       /* GP_FLAG_* */
    int32_t reserved;
} gp_config;

/* What the scheduler actor reports (Program.fs:53-55) plus throughput. */
typedef struct gp_result {
    int64_t rounds;             /* rounds executed by this handle so far */
    int64_t converged;          /* cumulative alerts (scheduler `counter`, Program.fs:52) */
    int64_t population;         /* P: nodes simulated */
    int64_t threshold;          /* T: alerts needed (Program.fs:53) */
    double elapsed_ms;          /* round-loop wall time of this call (Stopwatch, Program.fs:35,194,54) */
    double node_updates_per_s;  /* P * rounds / elapsed */
    double hbm_bytes_alg;       /* algorithmic HBM bytes of the rounds run */
    int32_t status;             /* GP_STATUS_* */
    int32_t reserved;
} gp_result;

typedef struct gp_info {
    int64_t population, threshold, grid;  /* P, T, g (g = 0 for line/full) */
    int64_t seed_node;                    /* `choice` (Program.fs:193,221,263) */
    int64_t rounds, alerts_total, active; /* progress */
    int32_t topology, algorithm;
    int32_t device, num_gpus;             /* num_gpus = ranks sharing the population */
    int64_t slab_first, slab_count;       /* node ids owned by this handle */
} gp_info;

/* Library version (GP_VERSION). */
int gp_version(void);
/* Message for the last failing call on this thread ("" if none). */
const char* gp_last_error(void);

/* CLI helpers: parse the reference's case-sensitive strings (Program.fs:178-279);
 * "imp3D" is accepted as an alias of "Imp3D".  Return the enum or GP_EINVAL. */
int gp_parse_topology(const char* s);
int gp_parse_algorithm(const char* s);
/* Resolve P (population), T (alert threshold) and g (grid edge) for n nodes:
 * line/full P = n+1, T = n (Program.fs:170-171,53); 3D/Imp3D g = ceil(cbrt n)
 * exactly, P = T = g^3 (Program.fs:239-240). */
int gp_resolve(int64_t num_nodes, int32_t topology, int64_t* P, int64_t* T, int64_t* g);

/* Replaces Program.fs:36-39,63,65-176 and the topology blocks 180-191 / 209-216 /
 * 238-261: allocates the SoA node state on the device, builds the implicit
 * topology (Imp3D: random edges + receiver-sorted in-lists), initialises
 * s = id, w = 1, count = 1, rumours = 0, and picks the seed node. */
int gp_create(const gp_config* cfg, gp_sim** out);

/* Multi-GPU: one process per GPU.  `unique_id` is the 128-byte RCCL id from
 * gp_get_unique_id() on rank 0, broadcast by the caller.  Nodes are split into
 * contiguous id slabs (plane-aligned for 3D/Imp3D). */
int gp_get_unique_id(uint8_t unique_id[128]);
int gp_create_rank(const gp_config* cfg, int32_t rank, int32_t world, const uint8_t unique_id[128],
                   gp_sim** out);

/* Launcher rendezvous without a host framework (gossip --gpus N, bench.py
 * --gpus N, the F# front-end): the launcher starts one process per GPU before
 * any of them touches a GPU and hands all of them one fresh file path.  Rank 0
 * calls gp_get_unique_id and publishes the 128 bytes at `path` (written under a
 * private name, then renamed, so a reader never sees a partial id); every other
 * rank waits for the file (at most timeout_ms; < 0 waits forever) and reads it.
 * Then every rank calls gp_create_rank with the same id.  The launcher removes
 * the file afterwards.  The path must be fresh: rank 0 fails with GP_ESTATE when
 * a file is already there.  If GOSSIP_RDV_NONCE is set in the environment (the
 * launchers set one value per launch), rank 0 appends it to the id and readers
 * accept only a file carrying the same nonce, so a file left at a reused path by
 * a crashed run is never taken for this run's id. */
int gp_rendezvous_id(int32_t rank, const char* path, int32_t timeout_ms, uint8_t unique_id[128]);

/* Replaces the message loop Program.fs:84-131,141-163 plus the scheduler
 * Program.fs:41-61: runs synchronous rounds until the cumulative alert count
 * reaches T (then status = GP_STATUS_CONVERGED) or max_rounds is hit. */
int gp_run(gp_sim* sim, gp_result* out);

/* Runs at most `nrounds` rounds (stops after the converging round).  Writes the
 * per-round alert counts of the executed rounds to alerts_per_round_out (may be
 * NULL).  Returns the number of rounds executed (>= 0) or a GP_E* code. */
int64_t gp_step(gp_sim* sim, int64_t nrounds, int64_t* alerts_per_round_out);

/* Copies node state [first, first+count) to caller buffers; null pointers are
 * skipped.  c: gossip rumour counters (push-sum: 0).  s, w: push-sum sum and
 * weight (gossip: 0).  flags: bit0 active, bit1 converged, bits2-3 push-sum
 * stability count.  In multi-GPU mode the range must lie in this rank's slab. */
int gp_read_state(gp_sim* sim, int64_t first, int64_t count, int32_t* c, double* s, double* w,
                  uint8_t* flags);

/* Neighbour list of node i in the reference's slot order (Program.fs:182-191,
 * 211-216, 246-260).  Writes min(deg, cap) ids; returns deg or a GP_E* code. */
int gp_neighbors(gp_sim* sim, int64_t node, int64_t* out, int64_t cap);

int gp_get_info(gp_sim* sim, gp_info* out);
/* Blocks until all work queued by the handle has finished. */
int gp_sync(gp_sim* sim);
/* Round-kernel timing (GP_FLAG_KERNEL_TIMING): sum of HIP-event durations of the
 * dominant per-round kernel and the number of launches measured since the last
 * reset; `name` receives the kernel's name (may be NULL). */
int gp_kernel_stats(gp_sim* sim, double* total_ms, int64_t* launches, char* name, int32_t name_cap,
                    int32_t reset);
/* Algorithmic HBM bytes per node-round of the dominant kernel for the current
 * state. */
double gp_alg_bytes_per_node(gp_sim* sim);

void gp_destroy(gp_sim* sim);

/* ---- Ensembles: many small networks per launch ----------------
 * The reference was run at 100..1000 nodes (README.md, Report.pdf), where what
 * is wanted is statistics over many seeds.  An ensemble simulates one network
 * per seed, each by one workgroup with its whole state in LDS, all seeds
 * concurrently; every member is bit-identical to a gp_create / gp_run of the
 * same (num_nodes, topology, algorithm, seed). */
typedef struct gp_ensemble gp_ensemble;
typedef struct gp_member {      /* one per seed, blittable */
    uint64_t seed;
    int64_t rounds;             /* rounds this member executed */
    int64_t converged;          /* cumulative alerts */
    int64_t seed_node;          /* `choice` (Program.fs:193,221,263) */
    int32_t status;             /* GP_STATUS_* */
    int32_t reserved;
} gp_member;

/* Largest num_nodes an ensemble accepts for the pair (host only, no GPU), or GP_EINVAL. */
int64_t gp_ensemble_max_nodes(int32_t topology, int32_t algorithm);
/* One member per seed, in the order of `seeds` (duplicates allowed).  cfg->seed is
 * ignored; cfg->device and cfg->max_rounds are honoured, and max_rounds must be > 0.
 * num_gpus must be 1 and num_nodes <= gp_ensemble_max_nodes(). */
int gp_ensemble_create(const gp_config* cfg, const uint64_t* seeds, int64_t nseeds, gp_ensemble** out);
/* Every unfinished member runs up to nrounds more rounds (stops after its converging
 * round or at max_rounds).  Returns the members still running, or a GP_E* code. */
int64_t gp_ensemble_step(gp_ensemble* e, int64_t nrounds);
/* Runs until every member has converged or hit max_rounds; out (nseeds, may be NULL). */
int gp_ensemble_run(gp_ensemble* e, gp_member* out);
/* Copies the nseeds member records to out. */
int gp_ensemble_members(gp_ensemble* e, gp_member* out);
/* gp_read_state of one member. */
int gp_ensemble_read_state(gp_ensemble* e, int64_t member, int64_t first, int64_t count, int32_t* c,
                           double* s, double* w, uint8_t* flags);
void gp_ensemble_destroy(gp_ensemble* e);

/* ---- Ensembles with a failure model: SRS v1-F ------
 * The question the reference never reached: every actor there lives for ever and
 * every `<!` is delivered.  A failure ensemble fixes, per member, a doomed set D
 * (node i != seed node is in D with probability node_fail; one Philox draw per
 * node, stream 5) whose nodes go down from round fail_round on -- they neither send
 * nor receive, their state is frozen -- and loses every node-to-node message with
 * probability msg_drop (one draw per sender and round, stream 6; the gossip
 * injector's messages are never dropped).  Only alerts of nodes outside D count, and
 * a member converges at T_f = max(1, T - |D|) of them.  A probability p acts as the
 * threshold q = floor(p * 2^32): an event happens iff the draw's first 32-bit word
 * is < q, so p = 1 means always and no floating-point comparison decides a fault.
 * With node_fail = msg_drop = 0 every member is bit-identical to gp_ensemble_create. */
typedef struct gp_faults {      /* blittable */
    double node_fail, msg_drop; /* probabilities in [0, 1] */
    int64_t fail_round;         /* >= 0: the first round in which the doomed nodes are down */
    int64_t reserved;           /* 0 */
} gp_faults;
typedef struct gp_fault_stats { /* one per member, blittable */
    int64_t doomed;             /* |D| */
    int64_t down;               /* |D| once the member's rounds >= fail_round, 0 before */
    int64_t threshold;          /* T_f */
    int64_t lost;               /* messages a node sent that nobody received: dropped, or addressed
                                   to a down node (a converged gossip target suppresses, not loses) */
} gp_fault_stats;
/* gp_ensemble_read_state flag bit 4: the node is down at the member's current round count
 * (failure ensembles only; a down gossip node never shows bit 0). */
enum { GP_STATE_DOWN = 0x10 };

/* gp_ensemble_max_nodes for a failure ensemble (host only): the doomed bitmap takes LDS,
 * so a cap may be lower than the plain one. */
int64_t gp_ensemble_faults_max_nodes(int32_t topology, int32_t algorithm);
/* gp_ensemble_create with a failure model.  Every check of gp_ensemble_create applies
 * (against gp_ensemble_faults_max_nodes); in addition faults must be non-null, both
 * probabilities in [0, 1] (NaN refused), fail_round >= 0 and reserved 0, else GP_EINVAL.
 * The handle works with every gp_ensemble_* call.  gp_member.converged holds the counted
 * alerts.  gp_ensemble_summary is unchanged: it reduces all P nodes, frozen ones included. */
int gp_ensemble_create_faults(const gp_config* cfg, const gp_faults* faults, const uint64_t* seeds,
                              int64_t nseeds, gp_ensemble** out);
/* nseeds records to out.  On a plain ensemble doomed = down = lost = 0 and threshold = T. */
int gp_ensemble_fault_stats(gp_ensemble* e, gp_fault_stats* out);

/* ---- Ensemble traces: SRS v1-T -------------------------------------
 * How a member got to its end: the S-curve of nodes reached, the messages spent, the
 * decay of push-sum's worst estimate error, recorded inside the kernel.  A member that
 * has just completed round R (R = 1, 2, ..., as gp_member.rounds counts) records a row
 * iff R % stride == 0 and k = R / stride - 1 < capacity; row k is the state after R
 * rounds, the one gp_ensemble_read_state would return if the member stopped there.  A
 * member has recorded min(capacity, rounds / stride) rows; the initial state has none,
 * nor has a final state whose round is no multiple of stride.  Tracing observes only:
 * a traced member is bit-identical to the untraced one. */
typedef struct gp_trace_row {   /* 32 bytes, blittable */
    int64_t  round;    /* R: rounds completed when the row was taken */
    uint32_t reached;  /* gossip: nodes that know the rumour: c >= 1, or the seed node;
                          push-sum: nodes with flag bit0 (active), down ones included */
    uint32_t alerts;   /* cumulative counted alerts (gp_member.converged at round R) */
    uint64_t sent;     /* cumulative node-to-node messages sent in rounds 1..R: one per (node, round) in
                          which the node drew a target, i.e. gossip: (seed node or c >= 1) and c <= 10 at
                          round start; push-sum: active at round start; under the failure model: and not
                          down in that round.  Suppressed, dropped and lost messages count (they were sent);
                          the gossip injector's picks do not. */
    double   err_max;  /* push-sum: max over all P nodes of |fl(fl(s/w) - mu)|, mu = the handle's mean,
                          (P - 1) / 2 unless values were set, exactly as
                          gp_summary.err_max defines the term, taken as the largest 64-bit pattern with the
                          sign bit cleared; a pattern above +inf's reads as the quiet NaN 0x7FF8000000000000.
                          gossip: 0.0 */
} gp_trace_row;
typedef struct gp_trace_cfg {   /* blittable */
    int64_t stride;             /* >= 1 */
    int64_t capacity;           /* rows per member, >= 0; 0: floor(max_rounds / stride), i.e. every row */
    int64_t reserved[2];        /* 0 */
} gp_trace_cfg;

/* gp_ensemble_max_nodes for a traced ensemble (host only); faults != 0: with a failure model. */
int64_t gp_ensemble_trace_max_nodes(int32_t topology, int32_t algorithm, int32_t faults);
/* gp_ensemble_create / _create_faults (faults may be NULL) with tracing.  Every check of those
 * applies (against gp_ensemble_trace_max_nodes); in addition trace must be non-null, stride >= 1,
 * capacity >= 0, reserved 0 and nseeds x capacity x 32 bytes at most 1 GiB, else GP_EINVAL.
 * The handle works with every gp_ensemble_* call. */
int gp_ensemble_create_traced(const gp_config* cfg, const gp_faults* faults, const gp_trace_cfg* trace,
                              const uint64_t* seeds, int64_t nseeds, gp_ensemble** out);
/* Rows recorded so far per member: nseeds values.  GP_ESTATE on an untraced ensemble. */
int gp_ensemble_trace_rows(gp_ensemble* e, int64_t* rows_out);
/* Rows [first, first+count) of one member; the range must lie within its recorded rows. */
int gp_ensemble_trace_read(gp_ensemble* e, int64_t member, int64_t first, int64_t count, gp_trace_row* out);

/* ---- State summary: what a run computed, reduced on the device ---
 * The reference never printed s/w, yet that ratio is the whole
 * output of push-sum.  gp_summary_take reduces the node state where it lives, in
 * one pass (17 B per push-sum node, 4 B per gossip node), instead of copying it
 * to the host with gp_read_state.  Every field is a pure function of the state:
 * two calls on the same handle and state return identical bytes. */
enum { GP_SCOPE_LOCAL = 0, GP_SCOPE_GLOBAL = 1 };
typedef struct gp_summary {      /* blittable, fixed layout (304 bytes) */
    int64_t first, count;        /* node ids covered: [first, first + count) */
    int64_t population, rounds;  /* P of the whole network; rounds executed when the summary was taken */
    int32_t algorithm, reserved; /* GP_GOSSIP | GP_PUSHSUM; 0 */
    int64_t active, converged;   /* nodes with flag bit0 / bit1 set, as gp_read_state defines them */
    /* gossip (all zero for push-sum) */
    int64_t c_hist[12];          /* nodes whose rumour counter c is 0..10, and (last) c >= 11 */
    int32_t c_max, reserved2;    /* largest rumour counter; 0 */
    /* push-sum (all zero for gossip) */
    int64_t cnt_hist[4];         /* nodes whose stability count (flag bits 2-3) is 0..3 */
    double  est_min, est_max;    /* min / max over the nodes of the estimate fl(s / w) */
    double  w_min, w_max;        /* min / max weight */
    double  err_max;             /* max |e|, e = fl(fl(s / w) - mu), mu = the handle's mean, (P - 1) / 2 unless
                                    values were set */
    int64_t err_max_node;        /* lowest node id attaining err_max */
    int64_t within_tol;          /* nodes with |e| <= tol */
    double  tol;                 /* the tolerance the summary was taken with */
    double  sum_s[2], sum_w[2];  /* sum of s / of w as a double-double (hi, lo): the conserved mass */
    double  sum_sqerr[2];        /* sum of fl(e * e), double-double (hi, lo) */
} gp_summary;

/* Summary of the node ids `scope` covers.  GP_SCOPE_LOCAL: the ids this handle owns
 * (a single-GPU or virtual-rank handle owns all P; a gp_create_rank handle its slab).
 * GP_SCOPE_GLOBAL on a gp_create_rank handle is collective -- every rank calls it, the
 * ranks' local summaries are gathered over the handle's communicator and merged in rank
 * order, and every rank receives the whole network's summary; on any other handle it
 * equals LOCAL.  tol must be finite and >= 0.  Synchronises the handle's stream, reads
 * the state gp_read_state would read, and leaves the run untouched. */
int gp_summary_take(gp_sim* sim, double tol, int32_t scope, gp_summary* out);
/* out = a joined with b (host only, no GPU).  a and b must be adjacent
 * (a.first + a.count == b.first) and agree in population, rounds, algorithm and tol,
 * else GP_EINVAL.  Counts and histograms add, min / max combine, err_max_node ties go
 * to the lower id, the double-double sums add as double-doubles.  out may alias a or b. */
int gp_summary_merge(const gp_summary* a, const gp_summary* b, gp_summary* out);
/* One summary per ensemble member into out (nseeds records, each with first = 0 and
 * count = P, rounds = the member's), in one launch. */
int gp_ensemble_summary(gp_ensemble* e, double tol, gp_summary* out);

/* ---- Push-sum over caller-supplied values and weights: SRS v1-V ---
 * Push-sum aggregates data that lives on the nodes; without these calls every run averages
 * s_i = i, w_i = 1.  SRS v1-V is SRS v1 with the push-sum initial state s_i = x_i, w_i = omega_i
 * (count = 1, only the seed node active); the stop rule, the Philox streams, the fold order and
 * the ratio test are v1's.  Gossip has no values: these calls refuse a gossip configuration with
 * GP_EINVAL.  A handle that never sets values, and an ensemble made by the other entry points,
 * is bit-identical to what it was.
 *
 * Admissible input -- every entry is checked (on the device), and a call with an inadmissible
 * one returns GP_EINVAL, changes nothing, and names the lowest offending node id and its rule in
 * gp_last_error():
 *   - x_i and omega_i are finite with the sign bit clear (-0.0 is refused);
 *   - omega_i in [2^-32, 2^32]; a null weight pointer means all weights are 1;
 *   - x_i = 0, or x_i >= 2^-64;
 *   - x_i * 2^-32 < omega_i, so that every ratio s / w a run forms stays below 2^32.
 * Negative data is out of scope: the caller shifts it.
 *
 * mu, the value err_max, err_max_node, within_tol and sum_sqerr of the summaries and err_max of
 * the trace rows are measured against, is an input of a value run, not something the library
 * derives: finite, >= 0 and < 2^32. */
typedef struct gp_values {      /* blittable */
    const double* x;            /* count values */
    const double* w;            /* count weights, or NULL: all 1 */
    int64_t count;
    double mean;                /* mu */
    int64_t reserved;           /* 0 */
} gp_values;

/* Overwrites the initial (s, w) of node ids [first, first + count).  Push-sum handles only
 * (else GP_EINVAL), and only while the handle has run no round (else GP_ESTATE).  The range must
 * lie inside the ids the handle owns: all P for a single-GPU or virtual-rank handle, the slab
 * for a gp_create_rank handle.  May be called any number of times, so a large network can be
 * loaded in chunks (the arrays are streamed through a bounded pinned buffer; a call of at most
 * 2^20 nodes is uploaded once, a longer one twice); each call is all or nothing.  Flags, count,
 * active bit and seed node stay as they are.  On gp_create_rank handles, if any rank sets values
 * every rank calls gp_set_values at least once (count 0 will do) before the first gp_step. */
int gp_set_values(gp_sim* sim, int64_t first, int64_t count, const double* x, const double* w);
/* Sets mu (any round).  On gp_create_rank handles every rank sets the same value:
 * gp_summary_merge cannot check it, the 304-byte record does not carry mu. */
int gp_set_mean(gp_sim* sim, double mean);

/* gp_ensemble_create / _create_faults / _create_traced (faults and trace may be NULL) where every
 * member starts from the same P values.  Every check of those applies, against the same
 * gp_ensemble_*_max_nodes; in addition values must be non-null with x non-null, count == P,
 * reserved == 0, an admissible mean and admissible entries, and cfg must be push-sum. */
int gp_ensemble_create_values(const gp_config* cfg, const gp_values* values, const gp_faults* faults,
                              const gp_trace_cfg* trace, const uint64_t* seeds, int64_t nseeds,
                              gp_ensemble** out);

/* ---- Ensembles over a caller-supplied graph: SRS v1-G ---------
 * The four topologies above are the reference's; this is yours.  A directed graph in CSR form:
 * the neighbours of node i are indices[indptr[i] .. indptr[i + 1]) in the caller's order (the
 * reference's NeighbourRef array).  Self-loops are allowed, duplicates are allowed and weight the
 * pick, an undirected network lists every edge both ways.  P = T = num_nodes, no extra actor; the
 * seed node is U_START(T).  Gossip: an active node delivers to nb(i)[U_GOSSIP(deg i)], the
 * injector runs over {0..T-1} as for line / 3D, so a run ends whatever the graph.  Push-sum: an
 * active node halves itself and sends to nb(i)[U_PUSHSUM(deg i)]; a receiver folds its own half
 * first, then every message by ascending sender id.  Everything else is SRS v1 with the same
 * streams, and the failure model, the trace and the values compose as with the built-in topologies.
 *
 * Admissible graphs -- checked on the host, all or nothing; gp_last_error() names the lowest
 * offending node and the first rule it breaks:
 *   - 2 <= num_nodes <= 8192 (one workgroup's node slots), reserved == 0;
 *   - indptr[0] == 0, indptr non-decreasing, indptr[num_nodes] == num_edges;
 *   - every node has degree >= 1;
 *   - every index < num_nodes;
 *   - the member's LDS image, adjacency included, fits (gp_ensemble_graph_lds_bytes; the error
 *     names the bytes it would need).
 * A graph that is not strongly connected is admissible: push-sum on it ends at max_rounds. */
typedef struct gp_graph {       /* blittable */
    const int64_t* indptr;      /* num_nodes + 1 entries */
    const uint32_t* indices;    /* num_edges entries */
    int64_t num_nodes;
    int64_t num_edges;
    int64_t reserved;           /* 0 */
} gp_graph;

/* The LDS image in bytes of one member on this graph (host only, no GPU): validates the graph and
 * returns the size, or GP_EINVAL for an inadmissible graph or pair -- one whose image exceeds the
 * 150 KiB a member may take included.  faults / trace != 0: with a failure model / a trace. */
int64_t gp_ensemble_graph_lds_bytes(const gp_graph* graph, int32_t algorithm, int32_t faults, int32_t trace);
/* An ensemble on the graph: cfg->topology must be GP_GRAPH and cfg->num_nodes == graph->num_nodes.
 * values (push-sum only), faults and trace may be NULL; every check of gp_ensemble_create,
 * _create_faults, _create_traced and _create_values applies to what is given.  The arrays are
 * copied: the caller may free them after the call.  The handle works with every gp_ensemble_* call;
 * the summaries' default mean is (P - 1) / 2. */
int gp_ensemble_create_graph(const gp_config* cfg, const gp_graph* graph, const gp_values* values,
                             const gp_faults* faults, const gp_trace_cfg* trace, const uint64_t* seeds,
                             int64_t nseeds, gp_ensemble** out);

#ifdef __cplusplus
}
#endif
#endif /* GOSSIP_HIP_H */
