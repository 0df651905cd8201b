// gp_ensemble_faults.hip -- ensemble kernels with a failure model: the FAULTS = true
// instantiations of gp_ensemble_kernels.hpp (SRS v1-F, SURVEY.md Appendix B.5:
// doomed nodes that go down at fail_round, messages dropped with a probability)
// and their launch interface.  DESIGN.md §11.  Kept apart from gp_ensemble.hip so
// that the plain kernels' object stays what it is.
#include "gp_ensemble_kernels.hpp"

namespace gp {

hipError_t ens_faults_setup(int topo, int alg, uint32_t P) { return ens_setup_t<true>(topo, alg, P); }

hipError_t ens_faults_launch(int topo, int alg, const EnsFaultArgs& a, uint32_t nblocks, hipStream_t st) {
    return ens_launch_t<true>(topo, alg, a, nblocks, st);
}

}  // namespace gp
