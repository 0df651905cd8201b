// gp_ensemble_trace.hip -- ensemble kernels that record a trace: the TRACE = true
// instantiations of gp_ensemble_kernels.hpp for both values of FAULTS (SRS v1-T: a
// 32-byte row per `stride` rounds with the nodes reached, the counted alerts, the
// messages sent and push-sum's worst estimate error, taken from LDS and registers
// inside the round loop).  DESIGN.md §12.  Kept apart from gp_ensemble.hip and
// gp_ensemble_faults.hip so that their objects stay what they are.
#include "gp_ensemble_kernels.hpp"

namespace gp {

template hipError_t ens_setup_t<false, true>(int, int, uint32_t, uint32_t);
template hipError_t ens_launch_t<false, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);
template hipError_t ens_setup_t<true, true>(int, int, uint32_t, uint32_t);
template hipError_t ens_launch_t<true, true>(int, int, const EnsArgs&, uint32_t, hipStream_t);

}  // namespace gp
