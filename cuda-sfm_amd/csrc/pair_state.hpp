// pair_state.hpp -- which of a pair's results describe its current points: the seven stages as one value, one named
// transition per kind of producing call, and the text of each stage's SFM_E_STATE.  Nothing else assigns a stage.  No HIP header:
// a host compiler builds this file alone (tests/hostcheck/pairstatecheck.cpp).
#pragma once
#include <stdint.h>

namespace sfm {

enum PairStage : uint32_t {
    kPoints = 1,        // X / U hold correspondences (fillXU, set_points)
    kE = 2,             // d_E, d_mask, d_best: a finalized hypothesis
    kP = 4,             // the four pose candidates
    kPose = 8,          // the chosen candidate and the inverses
    kPoints3d = 16,     // linear_triangulation ran for the current pose
    kRefined = 32,      // a refinement ran since the last fillXU / set_points / reset
    kView = 64          // a registration ran since the last fillXU / set_points / reset
};

struct PairState {
    uint32_t have = 0;
    // what was derived from the points (read by ransac*.hip)
    bool unit_z = false;               // every X z-coordinate is exactly 1 (fillXU with K^-1 last row (0 0 1))
    bool have_pts4 = false;            // d_pts4 describes the current points (fillXU with the unit-z layout)
    bool have_bound = false;           // d_bound describes the current points (fillXU)
    bool key_clean = false;            // slot[0].key is known to be zero (pair creation, fillXU): the next score launch needs no memset
    uint32_t last_count = 0;           // hyp_count of the last score call

    bool has(uint32_t stages) const { return (have & stages) == stages; }
    uint32_t missing(uint32_t stages) const { return stages & ~have; }

    // the three ways the points change: everything computed from the old ones is stale
    void reset() { have = 0; last_count = 0; }                          // sfm_pair_reset: no points either
    void points_filled(bool z_is_one)                                   // sfm_fill_xu: fill_xu_kernel zeroes slot[0].key, writes the 16-byte
    {                                                                   // records (they stand for the points when every z is 1) and the bound
        have = kPoints; last_count = 0;
        key_clean = true; unit_z = z_is_one; have_pts4 = z_is_one; have_bound = true;
    }
    void points_set()                                                   // sfm_set_points: generic z, no records, no bound
    {
        have = kPoints; last_count = 0;
        unit_z = have_pts4 = have_bound = false;
    }
    // a new E makes the poses stale, NOT the refinement or the registration (they are stale only after new points)
    void E_finalized() { have = (have & ~(kP | kPose | kPoints3d)) | kE; }
    void candidates_done() { have = (have & ~(kPose | kPoints3d)) | kP; }
    void pose_chosen() { have = (have & ~kPoints3d) | kPose; }
    void triangulated() { have |= kPoints3d; }
    void chain_done() { have |= kP | kPose | kPoints3d; }              // sfm_pose_chain, REFERENCE mode: the three above in one launch
    void refined() { have |= kRefined; }
    void view_registered() { have |= kView; }
    void view_dropped() { have &= ~(uint32_t)kView; }                   // its per-hypothesis buffers are about to be regrown
};

// What is missing and which call provides it: the SFM_E_STATE text of the first missing stage.
inline const char *pair_stage_hint(uint32_t missing)
{
    if (missing & kPoints) return "no points yet: fillXU / set_points has not run";
    if (missing & kE) return "no E yet: estimateE (or a ransac_finalize) has not run";
    if (missing & kP) return "no pose candidates yet: computePosecandidates has not run";
    if (missing & kPose) return "choosePose has not run";
    if (missing & kPoints3d) return "linear_triangulation has not run";
    if (missing & kRefined) return "no refinement since the last fillXU / set_points / reset";
    if (missing & kView) return "no registration since the last fillXU / set_points / reset";
    return "";
}

} // namespace sfm
