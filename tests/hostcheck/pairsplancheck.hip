// TEST SUPPORT: the host arithmetic of a batched sfm_process_pairs call (pairs_batch.hpp) -- the layout of a job's arrays in the
// workspace and the grouping of jobs into matcher launches -- host-compiled for tests/test_pairs_plan_host.py.
#include "../../cuda-sfm_amd/csrc/pairs_batch.hpp"

extern "C" {

// `count` jobs of (n[k], H[k]) carved back to back from `base` (0: the sizing pass).  out: per job the addresses of m_idx, X0, X1,
// counts, Ecand, key, mask, points, chosen and the bytes used after it.
void ppcheck_carve(uint64_t base, int count, const int *n, const uint32_t *H, uint64_t *out)
{
    sfm::Carver c(reinterpret_cast<void *>(base));
    for (int k = 0; k < count; ++k) {
        sfm::PairJob j{};
        j.n = n[k]; j.ld = sfm::round_up(n[k], 128); j.H = H[k];
        const size_t used = sfm::carve_pair_job(c, j);
        const void *arrays[9] = { j.m_idx, j.X0, j.X1, j.counts, j.Ecand, j.key, j.mask, j.points, j.chosen };
        for (int a = 0; a < 9; ++a) out[10 * k + a] = reinterpret_cast<uint64_t>(arrays[a]);
        out[10 * k + 9] = used;
    }
}

int ppcheck_align(void) { return (int)sfm::kPairJobAlign; }
int ppcheck_prefilter_id(void) { return SFM_MATCH_PREFILTER; }

// jobs k with first view view[k] (any distinct non-zero numbers), n[k] points and db_rows[k] database rows; pick[k]: what the
// kernel choice says for job k (the callback finds k by its db_rows, which the caller keeps distinct).  Returns the number of
// runs; per run begin, end, kernel.
int ppcheck_runs(int count, const uint64_t *view, const int *n, const int *db_rows, const int *pick, int *begin, int *end, int *kernel)
{
    std::vector<sfm::PairJob> jobs((size_t)count);
    for (int k = 0; k < count; ++k) { jobs[k].s1 = reinterpret_cast<const sfm_sift_point *>(view[k]); jobs[k].n = n[k]; }
    const std::vector<sfm::MatchRun> runs = sfm::plan_match_runs(jobs.data(), db_rows, (size_t)count, [&](int, int n2) {
        for (int k = 0; k < count; ++k) if (db_rows[k] == n2) return pick[k];
        return -1;
    });
    for (size_t r = 0; r < runs.size(); ++r) { begin[r] = (int)runs[r].begin; end[r] = (int)runs[r].end; kernel[r] = runs[r].kernel; }
    return (int)runs.size();
}

}
