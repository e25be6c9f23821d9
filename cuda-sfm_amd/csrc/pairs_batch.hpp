// pairs_batch.hpp -- one entry per view pair of a batched sfm_process_pairs call (BASELINE configs[4]): everything the three
// many-pairs kernels need to know about the pair (fill_xu_pairs, ransac_fused_pairs, finalize_pose_pairs; grid.y = pair).
// src/main.cpp:282-307 runs MatchSiftData -> fillXU -> estimateE -> poses -> triangulation once per pair; the per-pair
// kernels of that chain are a few wavefronts each, and 630 pairs x 5 launches are bound by the launch rate of the host
// (~7 us per launch), not by the GPU.  Batched, the matcher remains one launch per pair (it fills the chip) and the rest
// of the chain is three launches for ALL pairs.
#pragma once
#include "common.hpp"
#include <vector>

namespace sfm {

struct PairJob {
    const sfm_sift_point *s1, *s2;      // the two views' records (positions are read, nothing is written)
    const int *m_idx;                   // matcher output of this pair: index of the best match in s2 per point of s1 (-1: none)
    int n, ld;                          // correspondences (= points of the first view), padded row length
    uint32_t H, seed;                   // hypotheses (ids 0 .. H - 1), sampler seed
    float thr;
    float *X0, *X1;                     // 3 x ld each (K^-1 [x; y; 1]), NaN beyond n
    int *counts;                        // H
    float *Ecand;                       // 9 H
    unsigned long long *key;            // arg-max key of the pair
    uint8_t *mask;                      // n
    float *points;                      // 4 x n
    float *record;                      // SFM_RECORD_FLOATS: E | chosen pose | index, inliers, hypothesis | singular flag
    float *chosen;                      // 9 + 16 + 1: the winner's E, the chosen (inverted) candidate and whether a hypothesis won, from choose_pose_pairs to triangulate_pairs
};

// The arrays of one job inside the call's workspace -- THE layout: run over a null base it yields the bytes a job takes, run
// over the workspace its pointers (n, ld and H are set).  Every array starts at a multiple of 256 bytes, and so does the next job.
constexpr size_t kPairJobAlign = 256;
inline size_t carve_pair_job(Carver &c, PairJob &j)
{
    const size_t n = (size_t)j.n, ld = (size_t)j.ld, H = j.H, a = kPairJobAlign;
    j.m_idx = c.take<int>(n, a);
    j.X0 = c.take<float>(3 * ld, a);
    j.X1 = c.take<float>(3 * ld, a);
    j.counts = c.take<int>(H, a);
    j.Ecand = c.take<float>(9 * H, a);
    j.key = c.take<unsigned long long>(2, a);
    j.mask = c.take<uint8_t>(n, a);
    j.points = c.take<float>(4 * n, a);
    j.chosen = c.take<float>(9 + 16 + 1, a);
    (void)c.take<char>(0, a);
    return c.used;
}

// MatchSiftData of a batch: the jobs [begin, end) go through ONE matcher launch (launch_match_jobs, grid.z = pair) when there
// are two or more of them, a single job through the matcher rule of sfm_match.  Job end - 1 writes the first view's record fields.
struct MatchRun { size_t begin, end; int kernel; };
// A run is made of consecutive jobs that share their first view and its n (the all-pairs list of configs[4] has 35, 34, ... of
// them in a row) and run the same kernel -- pick(n1, n2) says which; the four-kernel pre-filter is never part of a run.
// db_rows: the rows of every job's second view that the matcher visits.
template <typename Pick>
inline std::vector<MatchRun> plan_match_runs(const PairJob *jobs, const int *db_rows, size_t njobs, Pick pick)
{
    std::vector<MatchRun> runs;
    for (size_t k = 0; k < njobs; ) {
        size_t k1 = k;
        int kernel = -1;                                    // one kernel per launch: what pick says for the first pair
        while (k1 < njobs && jobs[k1].s1 == jobs[k].s1 && jobs[k1].n == jobs[k].n) {
            const int p = db_rows[k1] < 1 ? SFM_MATCH_PREFILTER : pick(jobs[k].n, db_rows[k1]);
            if (p == SFM_MATCH_PREFILTER || (kernel >= 0 && p != kernel)) break;
            kernel = p;
            ++k1;
        }
        if (k1 < k + 2) { k1 = k + 1; kernel = -1; }         // no run: this pair alone
        runs.push_back({ k, k1, kernel });
        k = k1;
    }
    return runs;
}

int launch_fill_xu_pairs(sfm_ctx *ctx, const PairJob *d_jobs, int njobs, int max_ld, const float h_Kinv[9]);
int launch_fused_pairs(sfm_ctx *ctx, const PairJob *d_jobs, int njobs, int blocks_per_pair, uint32_t max_H);
int launch_finalize_pose_pairs(sfm_ctx *ctx, const PairJob *d_jobs, int njobs, int max_n);      // two launches: one wavefront per pair, then the points

} // namespace sfm
