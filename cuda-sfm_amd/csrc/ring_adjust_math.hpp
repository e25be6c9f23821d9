// ring_adjust_math.hpp -- arithmetic of sfm_adjust_ring (ring_adjust.hip): one bundle adjustment over a CLOSED ring as
// sfm_fuse_ring leaves it, one camera per view, view 0 fixed, the seam tracks used.
//
// Everything per observation and per track is chain_adjust_math.hpp's, unchanged.  What differs is which camera an observation
// belongs to and how the head pairs' partial bands add up:
//   views    an observation with obs_cam = c is of view ((c >> 1) + (c & 1)) mod k.  View 0 is the fixed [I|0] whichever pair
//            observes it; view v >= 1 is block v - 1 (k - 1 blocks), block 0 with kChainRoot's 5 degrees of freedom.
//   partial  a track headed in pair h has its local view v at ring view (h + v) mod k, chain tracks and seam tracks alike, so all
//            tracks of one head pair share one map from local to global blocks and chain_part_* holds their sums as it is.  Only
//            view 0 can occur twice in a track (h = 0, the full-cycle track: local 0 and local k); it has no block.
//   reduce   block (P, Q) of the reduced system is the sum over the head pairs h, ascending, of the local block
//            ((P + 1 - h) mod k, (Q + 1 - h) mod k) where both are < W -- transposed where the local indices come in the other
//            order.  On rings with k - 1 < W a block pair is reached both ways round; the sum over all h takes both.
//   fold     the reduced system is cyclic-banded (a band and two corners).  Positions 0, 1, 2, 3, ... hold the blocks 0, k - 2, 1,
//            k - 3, ...: two blocks fewer than W views apart round the ring lie at most 2 W - 1 positions apart, so the folded
//            system is block-banded with min(2 W, k - 1) block diagonals and chain_band_* factor and solve it as they are.  Block
//            0 stays at position 0: the unit row of the 5-dof block stays scalar row 5.
// Compiled as HIP host code by tests/hostcheck/ringadjustcheck.hip.
#pragma once
#include "chain_adjust_math.hpp"

namespace sfm {

constexpr int kRingCounts = 4 + kChainMaxViews;       // per head pair: used tracks, their observations, over-long tracks, used seam
                                                      // tracks, then the used observations of its local views 0 .. W - 1

SFM_HD int ring_view(int obs_cam, int k) { return ((obs_cam >> 1) + (obs_cam & 1)) % k; }
// the block of a view (-1: the fixed one) and what its camera is
SFM_HD int ring_block(int obs_cam, int k) { return ring_view(obs_cam, k) - 1; }
SFM_HD int ring_local_block(int h, int v, int k) { return (h + v) % k - 1; }
SFM_HD int ring_kind(int block) { return block < 0 ? kChainFixed : (block == 0 ? kChainRoot : kChainFree); }
// chain_used's flag test widened to the seam tracks
SFM_HD int ring_flag(int flag) { return flag == SFM_FUSE_SEAM_REFINED ? SFM_FUSE_REFINED : flag; }

// the fold: nb = k - 1 blocks
SFM_HD int ring_band_width(int W, int nb) { return 2 * W < nb ? 2 * W : nb; }
SFM_HD int ring_fold_block(int pos, int nb) { return (pos & 1) ? nb - 1 - (pos >> 1) : (pos >> 1); }
SFM_HD int ring_fold_pos(int block, int nb) { return block <= (nb - 1) / 2 ? 2 * block : 2 * (nb - 1 - block) + 1; }

// the head pair whose local view a is block P's view (a < k), and that pair's local index of block Q's view
SFM_HD int ring_head_of(int P, int a, int k) { const int h = P + 1 - a; return h < 0 ? h + k : h; }
SFM_HD int ring_local_of(int Q, int h, int k) { const int b = Q + 1 - h; return b < 0 ? b + k : b; }

// Element e = 6 i + j of block (P, Q), any order of P and Q: the head pairs in ascending order.  h = P + 1 - a for a <= P + 1
// (a descending: h ascending from P + 1 - a), then h = P + 1 - a + k for the larger a (again a descending), all of which are > P + 1.
SFM_HD double ring_reduce_block(const double *part, int W, int k, int P, int Q, int e)
{
    const size_t stride = (size_t)chain_part_values(W);
    const int top = (W < k ? W : k) - 1, et = 6 * (e % 6) + e / 6;
    double s = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        const int hi = pass == 0 ? (P + 1 < top ? P + 1 : top) : top, lo = pass == 0 ? 0 : P + 2;
        for (int a = hi; a >= lo; --a) {
            const int h = ring_head_of(P, a, k), b = ring_local_of(Q, h, k);
            if (b >= W) continue;
            s += a <= b ? part[stride * h + chain_part_block(W, a, b) + e] : part[stride * h + chain_part_block(W, b, a) + et];
        }
    }
    return s;
}
// value i of block P's rows of b (diag_u: of diag U), the head pairs in the same order
SFM_HD double ring_reduce_row(const double *part, int W, int k, int P, int i, bool diag_u)
{
    const size_t stride = (size_t)chain_part_values(W);
    const int top = (W < k ? W : k) - 1, at = diag_u ? chain_part_u(W) : chain_part_b(W);
    double s = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        const int hi = pass == 0 ? (P + 1 < top ? P + 1 : top) : top, lo = pass == 0 ? 0 : P + 2;
        for (int a = hi; a >= lo; --a) s += part[stride * ring_head_of(P, a, k) + at + 6 * a + i];
    }
    return s;
}
// block P's used observations from the head pairs' counts (kRingCounts ints per pair)
SFM_HD int ring_block_obs(const int *hcnt, int W, int k, int P)
{
    const int top = (W < k ? W : k) - 1;
    int n = 0;
    for (int a = 0; a <= top; ++a) n += hcnt[(size_t)kRingCounts * ring_head_of(P, a, k) + 4 + a];
    return n;
}

// the ring's one record between the launches
struct RingSeg {
    ChainSeg s;                           // (end is not used: the ring is one segment of k - 1 blocks)
    int seam;                             // used seam tracks
    SFM_HD RingSeg() : s(), seam(0) {}
};

} // namespace sfm
