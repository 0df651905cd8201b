// Host-side evaluation of the ensemble launch shape (gp_ensemble_shape.hpp is host-clean): reads one
// query per line from standard input and prints one line per query, the results as integers.
// Built by tests/test_ensemble_shape.py with the host compiler; runs on the CPU.
//   K                               -> ENS_THREADS ENS_NPT_MAX ENS_LDS_MAX ENS_LDS_HDR ENS_LDS_TRACE
//   shape topo alg P faults trace   -> npt threads lds_bytes     (npt of push-sum; 1 for gossip)
//   range alg P0 P1                 -> npt threads of every P in [P0, P1], in order
//   cap topo alg faults trace       -> max_population max_nodes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../gossipprotocol_amd/csrc/gp_ensemble_shape.hpp"

using namespace gp;

int main() {
    std::string line, q;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> q)) continue;
        std::printf("%s", q.c_str());
        if (q == "K") {
            std::printf(" %d %d %u %u %u", ENS_THREADS, ENS_NPT_MAX, ENS_LDS_MAX, ENS_LDS_HDR, ENS_LDS_TRACE);
        } else if (q == "shape") {
            int topo, alg, faults, trace;
            uint32_t P;
            in >> topo >> alg >> P >> faults >> trace;
            std::printf(" %d %u %u", alg == GP_PUSHSUM ? ens_npt(P) : 1, ens_threads(alg, P),
                        ens_lds_bytes(topo, alg, P, EnsVariant{faults != 0, trace != 0}));
        } else if (q == "range") {
            int alg;
            uint32_t P0, P1;
            in >> alg >> P0 >> P1;
            for (uint32_t P = P0; P <= P1 && P >= P0; ++P)
                std::printf(" %d %u", alg == GP_PUSHSUM ? ens_npt(P) : 1, ens_threads(alg, P));
        } else if (q == "cap") {
            int topo, alg, faults, trace;
            in >> topo >> alg >> faults >> trace;
            const EnsVariant v{faults != 0, trace != 0};
            std::printf(" %u %lld", ens_max_population(topo, alg, v), (long long)ens_max_nodes(topo, alg, v));
        } else {
            std::printf(" ?");
        }
        std::printf("\n");
    }
    return 0;
}
