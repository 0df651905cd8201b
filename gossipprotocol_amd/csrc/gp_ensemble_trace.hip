// gp_ensemble_trace.hip -- ensemble kernels that record a trace: the TRACE = true
// instantiations of gp_ensemble_kernels.hpp for both values of FAULTS (SRS v1-T: a
// 32-byte row per `stride` rounds with the nodes reached, the counted alerts, the
// messages sent and push-sum's worst estimate error, taken from LDS and registers
// inside the round loop) and their launch interface.  DESIGN.md §12.  Kept apart from
// gp_ensemble.hip and gp_ensemble_faults.hip so that their objects stay what they are.
#include "gp_ensemble_kernels.hpp"

namespace gp {

hipError_t ens_trace_setup(int topo, int alg, uint32_t P, bool faults) {
    return faults ? ens_setup_t<true, true>(topo, alg, P) : ens_setup_t<false, true>(topo, alg, P);
}

hipError_t ens_trace_launch(int topo, int alg, const EnsTraceArgs& a, uint32_t nblocks, hipStream_t st) {
    return ens_launch_t<false, true>(topo, alg, a, nblocks, st);
}

hipError_t ens_trace_launch(int topo, int alg, const EnsTraceFaultArgs& a, uint32_t nblocks, hipStream_t st) {
    return ens_launch_t<true, true>(topo, alg, a, nblocks, st);
}

}  // namespace gp
