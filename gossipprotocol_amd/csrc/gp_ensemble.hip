// gp_ensemble.hip -- the plain ensemble kernels: the <FAULTS, TRACE> = <false, false>
// instantiation of gp_ensemble_kernels.hpp (SRS v1, every node lives for ever and
// every message arrives).  DESIGN.md §9; the failure and the traced kernels are
// translation units of their own, gp_ensemble_faults.hip and gp_ensemble_trace.hip.
#include "gp_ensemble_kernels.hpp"

namespace gp {

template hipError_t ens_setup_t<false, false>(int, int, uint32_t, uint32_t);
template hipError_t ens_launch_t<false, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);

}  // namespace gp
