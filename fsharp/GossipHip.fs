/// P/Invoke binding of libgossip_hip.so (include/gossip_hip.h).
/// Blittable structs only, Cdecl, no marshalling code needed.
/// UNVERIFIED in this repository's CI: no .NET SDK exists in the build image.
module GossipHip

open System
open System.Runtime.InteropServices

[<Literal>]
let Lib = "gossip_hip"

[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpConfig =
    val mutable NumNodes: int64
    val mutable Topology: int32
    val mutable Algorithm: int32
    val mutable Seed: uint64
    val mutable NumGpus: int32
    val mutable Device: int32
    val mutable MaxRounds: int64
    val mutable Flags: int32
    val mutable Reserved: int32

[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpResult =
    val mutable Rounds: int64
    val mutable Converged: int64
    val mutable Population: int64
    val mutable Threshold: int64
    val mutable ElapsedMs: double
    val mutable NodeUpdatesPerS: double
    val mutable HbmBytesAlg: double
    val mutable Status: int32
    val mutable Reserved: int32

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_parse_topology(string s)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_parse_algorithm(string s)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_create(GpConfig& cfg, nativeint& sim)

/// Multi-GPU, one process per GPU: rank 0 publishes its RCCL id at `path`, the
/// other ranks read it (include/gossip_hip.h gp_rendezvous_id); then every rank
/// joins with gp_create_rank.
[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_rendezvous_id(int rank, string path, int timeoutMs, byte[] uniqueId)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_create_rank(GpConfig& cfg, int rank, int world, byte[] uniqueId, nativeint& sim)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_run(nativeint sim, GpResult& result)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int64 gp_step(nativeint sim, int64 nrounds, int64[] alertsPerRound)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_read_state(nativeint sim, int64 first, int64 count, int32[] c, double[] s, double[] w, byte[] flags)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern void gp_destroy(nativeint sim)

// Ensembles: one network per seed, all seeds at once (INTEGRATION.md §2.2)
[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpMember =
    val mutable Seed: uint64
    val mutable Rounds: int64
    val mutable Converged: int64
    val mutable SeedNode: int64
    val mutable Status: int32
    val mutable Reserved: int32

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int64 gp_ensemble_max_nodes(int topology, int algorithm)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_create(GpConfig& cfg, uint64[] seeds, int64 nseeds, nativeint& ensemble)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int64 gp_ensemble_step(nativeint ensemble, int64 nrounds)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_run(nativeint ensemble, [<Out>] GpMember[] members)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_members(nativeint ensemble, [<Out>] GpMember[] members)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_read_state(nativeint ensemble, int64 ``member``, int64 first, int64 count, int32[] c, double[] s, double[] w, byte[] flags)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern void gp_ensemble_destroy(nativeint ensemble)

// Ensembles with a failure model: crashed nodes and lost messages (SRS v1-F, DESIGN.md §11)
[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpFaults =
    val mutable NodeFail: double
    val mutable MsgDrop: double
    val mutable FailRound: int64
    val mutable Reserved: int64

[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpFaultStats =
    val mutable Doomed: int64
    val mutable Down: int64
    val mutable Threshold: int64
    val mutable Lost: int64

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int64 gp_ensemble_faults_max_nodes(int topology, int algorithm)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_create_faults(GpConfig& cfg, GpFaults& faults, uint64[] seeds, int64 nseeds, nativeint& ensemble)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_fault_stats(nativeint ensemble, [<Out>] GpFaultStats[] stats)

// State summary: what a run computed, reduced on the device (INTEGRATION.md §2.3).
// gp_summary is 304 bytes; the fixed arrays are spelled out field by field to stay blittable.
[<Struct; StructLayout(LayoutKind.Sequential)>]
type GpSummary =
    val mutable First: int64
    val mutable Count: int64
    val mutable Population: int64
    val mutable Rounds: int64
    val mutable Algorithm: int32
    val mutable Reserved: int32
    val mutable Active: int64
    val mutable Converged: int64
    val mutable CHist0: int64
    val mutable CHist1: int64
    val mutable CHist2: int64
    val mutable CHist3: int64
    val mutable CHist4: int64
    val mutable CHist5: int64
    val mutable CHist6: int64
    val mutable CHist7: int64
    val mutable CHist8: int64
    val mutable CHist9: int64
    val mutable CHist10: int64
    val mutable CHist11Plus: int64
    val mutable CMax: int32
    val mutable Reserved2: int32
    val mutable CntHist0: int64
    val mutable CntHist1: int64
    val mutable CntHist2: int64
    val mutable CntHist3: int64
    val mutable EstMin: double
    val mutable EstMax: double
    val mutable WMin: double
    val mutable WMax: double
    val mutable ErrMax: double
    val mutable ErrMaxNode: int64
    val mutable WithinTol: int64
    val mutable Tol: double
    val mutable SumSHi: double
    val mutable SumSLo: double
    val mutable SumWHi: double
    val mutable SumWLo: double
    val mutable SumSqErrHi: double
    val mutable SumSqErrLo: double

[<Literal>]
let GP_SCOPE_LOCAL = 0

[<Literal>]
let GP_SCOPE_GLOBAL = 1

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_summary_take(nativeint sim, double tol, int scope, GpSummary& result)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_summary_merge(GpSummary& a, GpSummary& b, GpSummary& result)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern int gp_ensemble_summary(nativeint ensemble, double tol, [<Out>] GpSummary[] summaries)

[<DllImport(Lib, CallingConvention = CallingConvention.Cdecl)>]
extern nativeint gp_last_error()

let lastError () = Marshal.PtrToStringAnsi(gp_last_error ())
