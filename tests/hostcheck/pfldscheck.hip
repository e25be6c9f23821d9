// TEST SUPPORT: the LDS footprint of the pre-filter scoring block (prefilter_lds.hpp), host-compiled for
// tests/test_register_budget.py.  The block's shared memory is dynamic -- the code object says 0 -- so the number comes from the
// very header launch_score_prefilter sizes its launches with.
#include "../../cuda-sfm_amd/csrc/prefilter_lds.hpp"

extern "C" {

// points per tile of a launch over `ld` correspondences
int pfcheck_tile_points(int ld) { return sfm::pf_tile_points(ld, sfm::kPfTileMax); }

// dynamic LDS bytes of one scoring block of the band rules (per-tile and per-hypothesis forms share the map) for that tile
int pfcheck_lds_bytes(int tile) { return sfm::PfLds<sfm::kPfRuleBand>(tile).bytes; }

// wavefronts of one scoring block
int pfcheck_block_waves(void) { return sfm::kPfWaves; }

}
