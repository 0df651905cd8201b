// gp_ensemble.hip -- the plain ensemble kernels: the FAULTS = false instantiations
// of gp_ensemble_kernels.hpp (SRS v1, every node lives for ever and every message
// arrives) and their launch interface.  DESIGN.md §9; the failure kernels are a
// translation unit of their own, gp_ensemble_faults.hip.
#include "gp_ensemble_kernels.hpp"

namespace gp {

hipError_t ens_setup(int topo, int alg, uint32_t P) { return ens_setup_t<false>(topo, alg, P); }

hipError_t ens_launch(int topo, int alg, const EnsArgs& a, uint32_t nblocks, hipStream_t st) {
    return ens_launch_t<false>(topo, alg, a, nblocks, st);
}

}  // namespace gp
