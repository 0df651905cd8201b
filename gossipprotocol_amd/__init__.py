"""gossipprotocol_amd -- MI355X-native synchronous gossip / push-sum simulator.

Drop-in for the hot path of sharwarimarathe/GossipProtocol
(`dotnet run num_nodes topology algorithm`, Program.fs:31-283): the per-round
message delivery of gossip and push-sum on line / full / 3D / Imp3D
topologies plus the convergence check, as HIP kernels for gfx950 behind the
C-ABI in include/gossip_hip.h.  See DESIGN.md.
"""
from .graph import Graph  # noqa: F401
from .sim import (ALGORITHMS, TOPOLOGIES, Ensemble, Faults, Simulation, Trace, Values,  # noqa: F401
                  default_mean, ensemble_graph_lds_bytes, ensemble_max_nodes, parse_algorithm, parse_topology,
                  resolve, run)

__version__ = "1.0.0"
