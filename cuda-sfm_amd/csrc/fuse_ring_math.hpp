// fuse_ring_math.hpp -- arithmetic of sfm_fuse_ring (fuse_ring.hip): sfm_fuse_chain's fusion over a closed ring, the tracks that
// cross the seam joined.
//
// Pairs 0 .. k - 1 of a ring, pair i = (view i, view i + 1 mod k), and k links; link k - 1 carries pair k - 1 into pair 0.  The
// chain part (fuse_math.hpp over the first k - 1 links) gives the frames and the chain tracks.  The closure D = F_{k-1} o
// L_{k-1}^-1 is taken from the STORED fp32 frame of pair k - 1 (what the points below are carried by) and goes through
// sfm_close_ring's ring_drift with this call's own gates; only a CLOSED ring is joined.
// The seam: record j of pair k - 1 proposes (0, index[j]) under fuse_edge.  A = the chain track that ends in (k - 1, j), headed in
// pair h_A; B = the chain track headed by (0, m) over len(B) pairs.  The proposal is eligible when len(B) < h_A: the joined track
// then sees views h_A .. k - 1, view 0 and views 1 .. len(B), every view once.  Among the eligible proposers of one target the
// smallest fuse_key wins; the winner's track goes on into B.  h_A >= 2 follows, so a track crosses the seam at most once, has at
// most k pairs, and no walk cycles; a feature followed round the whole ring to its own record has h_A = 0 and stays a chain track.
//
// Every walk here is a counted loop bounded by k.  The host build (tests/hostcheck/fuseringcheck.hip) runs the same functions.
#pragma once
#include "fuse_math.hpp"
#include "ring_math.hpp"

namespace sfm {

// what the seam kernels keep per record of pair k - 1: the global id of its chain track's head, or -1 where it proposes nothing
// eligible
constexpr int kFuseRingNoHead = -1;

// the first invalid link of the ring, or k: link i is pair i's (pair k - 1 holds the closing one)
SFM_HD int fuse_ring_first_invalid(const FusePair *pairs, int k, int from, int step)
{
    for (int i = from; i < k; i += step)
        if (!fuse_link_ok(pairs[i])) return i;
    return k;
}

// The closure of a ring whose k links are valid: D = frame o link^-1 in fp64 from the rounded frame of pair k - 1 and the closing
// link; closure: ln s, the rotation angle and |t| of D; returns SFM_RING_CLOSED or SFM_RING_REJECTED by ring_drift's two gates.
SFM_HD int fuse_ring_closure(const float frame[kFuseSim], const float link[kFuseSim], float max_rotation_rad, float max_log_scale,
                             float closure[3])
{
    double F[kFuseSim], inv[kFuseSim], D[kFuseSim];
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) F[q] = (double)frame[q];
    fuse_invert(link, inv);
    fuse_compose(F, inv, D);
    RingHead h;
    ring_drift(D, max_rotation_rad, max_log_scale, h, closure);
    return h.status;
}

// The head of the chain track through live node (pair, rec): backwards along the winning keys, whose low 32 bits are the
// predecessor's record.  Counted by the pair index: at most `pair` steps.  Returns the head's global id; head_pair: its pair.
SFM_HD int fuse_ring_head(const FusePair *pairs, const unsigned long long *keys, int pair, int rec, int &head_pair)
{
    int q = pair;
    for (; q > 0; --q) {
        const unsigned long long key = keys[(size_t)pairs[q].offset + rec];
        if (key == kFuseNoKey) break;
        rec = (int)(uint32_t)key;
    }
    head_pair = q;
    return pairs[q].offset + rec;
}

// len(B) < h_A: the two sides share no view
SFM_HD bool fuse_ring_eligible(int len_b, int head_pair) { return len_b < head_pair; }

// Record j of pair k - 1 (`last`) at the seam: the target in pair 0 (`first`, whose offset is 0) or -1 where there is no edge;
// where there is one, key is its key, head the head of its own chain track, and eligible the join rule's answer.  len: the chain
// tracks' lengths.
SFM_HD int fuse_ring_proposal(const FusePair *pairs, int k, const FusePair &last, const FusePair &first, bool link_ok,
                              const unsigned long long *keys, const int *len, int j, unsigned long long &key, int &head, bool &eligible)
{
    head = kFuseRingNoHead; eligible = false;
    const int m = fuse_edge(last, first, link_ok, j, key);
    if (m < 0) return -1;
    int hp;
    head = fuse_ring_head(pairs, keys, k - 1, j, hp);
    eligible = fuse_ring_eligible(len[(size_t)first.offset + m], hp);
    return m;
}

// the pair behind `pair` on a path of the ring
SFM_HD int fuse_ring_next(int pair, int k) { return pair + 1 == k ? 0 : pair + 1; }

// a track crosses the seam when its first observation's pair is larger than its last's; its flag is the chain's + 2
SFM_HD uint8_t fuse_ring_flag(uint8_t flag, int first_cam, int last_cam)
{
    return (first_cam >> 1) > (last_cam >> 1) ? (uint8_t)(flag + (SFM_FUSE_SEAM_REFINED - SFM_FUSE_REFINED)) : flag;
}

} // namespace sfm
