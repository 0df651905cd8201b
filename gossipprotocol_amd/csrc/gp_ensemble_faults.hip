// gp_ensemble_faults.hip -- ensemble kernels with a failure model: the <FAULTS, TRACE> =
// <true, false> instantiation of gp_ensemble_kernels.hpp (SRS v1-F, SURVEY.md Appendix
// B.5: doomed nodes that go down at fail_round, messages dropped with a probability).
// DESIGN.md §11.  Kept apart from gp_ensemble.hip so that the plain kernels' object
// stays what it is.
#include "gp_ensemble_kernels.hpp"

namespace gp {

template hipError_t ens_setup_t<true, false>(int, int, uint32_t, uint32_t);
template hipError_t ens_launch_t<true, false>(int, int, const EnsArgs&, uint32_t, hipStream_t);

}  // namespace gp
