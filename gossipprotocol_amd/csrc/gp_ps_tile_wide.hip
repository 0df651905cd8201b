// gp_ps_tile_wide.hip -- the push-sum tile kernel of gp_ps_tile.hip compiled a second
// time as the small-population size class: 1024 threads per 1024-node tile, one
// node per thread, 8 waves per SIMD (gp::wide::launch_ps_tile).  Line and 3D only:
// the Imp3D in-edge pass spills at 8 waves and measured slower at every size
// (profiles/r04/tile_size_class.txt), so gp_ps_tile.hip builds no Imp3D kernel here.
//
// A tile then costs one dependent memory round trip in its node phase instead of
// four (gp_ps_tile.hip's 256 threads x 4 nodes), which is what bounds a round when
// the network has only a few tiles per resident block: C2 (3D push-sum, P = 10^6,
// 977 tiles) measured 26.4 -> 21.0 us per round (profiles/r04/c2_tile_shape.txt).
// At 10^9 nodes the 4-nodes-per-thread kernel is faster (more waves' worth of
// memory-level parallelism per VGPR), so gp_setup.hip's choose_kernel picks by size.
#define GP_TILE_WIDE 1
#define GP_TPB 1024
#define GP_NPT 1
#define GP_MINB 8
#include "gp_ps_tile.hip"
