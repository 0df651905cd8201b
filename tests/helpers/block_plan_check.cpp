// Host-side print of the LDS-resident push-sum kernel's box grid (gp_block_plan.hpp is
// host-only): one line per (cus, g),
//   "P cus g nbx nby nbz vmax fmax lds"   or   "P cus g none"
// followed by the constants the plan is bounded by.
// Built by tests/test_block_plan.py with the host compiler; runs on the CPU.
#include <cstdio>

#include "../../gossipprotocol_amd/csrc/gp_block_plan.hpp"

int main() {
    const int cus[] = {8, 64, 256, 304};
    for (int c : cus)
        for (uint32_t g = 2; g <= 130; ++g) {
            gp::BlockPlan p{};
            if (gp::block_plan(g, c, p))
                std::printf("P %d %u %u %u %u %u %u %u\n", c, g, p.nbx, p.nby, p.nbz, p.vmax, p.fmax, p.lds);
            else
                std::printf("P %d %u none\n", c, g);
        }
    std::printf("K %d %d %u\n", gp::BK_THREADS, gp::BK_NPT, gp::BK_LDS_MAX);
    return 0;
}
