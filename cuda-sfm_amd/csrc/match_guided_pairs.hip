// match_guided_pairs.hip -- sfm_match_guided_pairs: the guided match (match_guided.hip) of many (view 1, view 2, F) jobs in at most
// two launches.
//
// A caller that refined 630 pairs in one call and took their 630 F matrices in one launch (pair_fundamentals.hip) looped over 630
// launches of match_guided_kernel, each sized for ONE small match: 2155 x 2170 is 9 query blocks x 14 splits, 126 blocks on 256
// CUs, half prologue and epilogue (the comment above match_mfma_jobs_kernel, match.hip).  Here every (job, query block, split) is
// one unit of a 1-D grid; the jobs of one configuration -- (1,4) up to 4500 queries, (1,8) above -- share a launch, and the splits
// come from ONE budget over all jobs of the launch (match_guided_plan.hpp), so many jobs mean few splits each: fewer prologues, fewer
// partials, a full chip.
//
// A block finds its job by a binary search of blockIdx.x over the first-unit fields of the launch's job table (a uniform address:
// scalar loads), derives (split, query block) inside the job and runs match_guided_body.inc, the schedule of the one-match kernel,
// on the job's own tickets and partials: the same scores in the same order, so job k's records are the single call's bytes
// whatever its split count.  A job's units are split-major (unit = first + split * qblocks + qblock): neighbours in the grid are
// the query blocks of one split, the order of the one-match launch's 2-D grid.  Nobody measured the other order (the splits of one
// query block next to each other, which would bring a query block's ticket draws closer together).
//
// No block waits for another, there is no polled merge, and the host waits only where a buffer grows or the staging buffer's
// previous upload is still in flight.  The workspace is ctx->match_jobs_ws, shared with launch_match_jobs: every user is ordered
// by the context's stream, and the tickets are zeroed on that stream before the launches.
//
// A translation unit of its own: build/match_guided.usage.txt keeps exactly the three kernels of match_guided.hip.
#include <new>
#include <vector>
#include "common.hpp"
#include "buffer_ranges.hpp"
#include "match_guided_plan.hpp"
#include "match_guided_device.hpp"

namespace sfm {

struct GuidedJob {                      // one entry of a launch's device table, in the order of the caller's list
    sfm_sift_point *sift1;
    const sfm_sift_point *sift2;
    const float *F;
    float *partials;                    // best[nsplit * n1], second[nsplit * n1], idx[nsplit * n1]
    unsigned int *tickets;              // one per query block
    int n1, n2, rows_per_split, nsplit, qblocks;
    unsigned int first_unit;            // strictly increasing over the table, table[0].first_unit == 0
};

template <int W>
__global__ __launch_bounds__(W * 64)
void match_guided_jobs_kernel(const GuidedJob *__restrict__ jobs, int njobs, float band)
{
    constexpr int CT = 1;
    // the last job whose first unit is not beyond this block's
    const unsigned int unit = blockIdx.x;
    int lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].first_unit <= unit) lo = mid; else hi = mid;
    }
    const GuidedJob &j = jobs[lo];
    sfm_sift_point *__restrict__ sift1 = j.sift1;
    const sfm_sift_point *__restrict__ sift2 = j.sift2;
    const float *__restrict__ d_F = j.F;
    const int nq = j.n1, ndb = j.n2, rows_per_split = j.rows_per_split, nsplit = j.nsplit;
    const int u = (int)(unit - j.first_unit);
    const int split = u / j.qblocks, qblock = u - split * j.qblocks;
    if (split >= nsplit) return;                                     // (never: the grid is the plan's unit count)
    float *__restrict__ ws_best = j.partials;
    float *__restrict__ ws_second = ws_best + (size_t)nsplit * nq;
    int *__restrict__ ws_idx = reinterpret_cast<int *>(ws_second + (size_t)nsplit * nq);
    unsigned int *__restrict__ tickets = j.tickets;
#include "match_guided_body.inc"
}

// jobs: checked (sizes >= 0, no null pointer in a job that runs, no overlap across jobs); jp, plan: match_guided_pairs_plan's
static int launch_match_guided_pairs(sfm_ctx *ctx, const sfm_match_guided_job *jobs, int num_jobs, const GuidedJobPlan *jp,
                                     const GuidedPairsPlan &plan, float band_px)
{
    if (!plan.launch[0].jobs && !plan.launch[1].jobs) return SFM_OK;
    // the tables: staged in pinned memory in the workspace's own layout, one copy
    const size_t table_bytes = plan.tickets_off;
    const size_t records = (table_bytes + sizeof(GuidedJob) - 1) / sizeof(GuidedJob);
    JobArray &ja = ctx->guided_jobs;
    int rc = job_array_reserve(ja, records, sizeof(GuidedJob), ctx->stream);
    if (rc != SFM_OK) return rc;
    rc = grow(&ctx->match_jobs_ws, &ctx->match_jobs_ws_bytes, plan.workspace_bytes, ctx->stream);
    if (rc != SFM_OK) return rc;
    char *base = static_cast<char *>(ctx->match_jobs_ws);
    char *stage = static_cast<char *>(ja.pinned);
    for (int k = 0; k < num_jobs; ++k) {
        const GuidedJobPlan &p = jp[k];
        if (p.launch < 0) continue;
        GuidedJob &g = reinterpret_cast<GuidedJob *>(stage + plan.launch[p.launch].table_off)[p.slot];
        g.sift1 = jobs[k].d_sift1; g.sift2 = jobs[k].d_sift2; g.F = jobs[k].d_F;
        g.partials = reinterpret_cast<float *>(base + p.partials_off);
        g.tickets = reinterpret_cast<unsigned int *>(base + p.tickets_off);
        g.n1 = jobs[k].n1; g.n2 = jobs[k].n2; g.rows_per_split = p.rows_per_split; g.nsplit = p.nsplit;
        g.qblocks = (int)p.qblocks;                                  // (<= 2^31 / 128)
        g.first_unit = (unsigned int)p.first_unit;                   // (< 2^31: the plan refuses more)
    }
    SFM_HIP_TRY(hipMemsetAsync(base + plan.tickets_off, 0, plan.tickets_bytes, ctx->stream));     // (the workspace is shared between calls of different shapes)
    SFM_HIP_TRY(hipMemcpyAsync(base, stage, table_bytes, hipMemcpyHostToDevice, ctx->stream));
    SFM_HIP_TRY(hipEventRecord(ja.ev, ctx->stream));
    for (int c = 0; c < 2; ++c) {
        const GuidedLaunchPlan &l = plan.launch[c];
        if (!l.jobs) continue;
        const GuidedJob *table = reinterpret_cast<const GuidedJob *>(base + l.table_off);
        const dim3 grid((unsigned int)l.units);
        if (l.wv == 8) hipLaunchKernelGGL((match_guided_jobs_kernel<8>), grid, dim3(512), 0, ctx->stream, table, (int)l.jobs, band_px);
        else hipLaunchKernelGGL((match_guided_jobs_kernel<4>), grid, dim3(256), 0, ctx->stream, table, (int)l.jobs, band_px);
        SFM_HIP_TRY(hipGetLastError());
    }
    return SFM_OK;
}

// everything that needs no device, in the order the header lists it
static int match_guided_pairs_checked(sfm_ctx *ctx, const sfm_match_guided_job *jobs, int num_jobs, const sfm_match_guided_params *p)
{
    SFM_REQUIRE(ctx && jobs && p, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(num_jobs >= 0, SFM_E_INVALID, "negative job count");
    SFM_REQUIRE(p->band_px > 0.0f && p->band_px < __builtin_inff(), SFM_E_INVALID, "sfm_match_guided_params.band_px must be finite and > 0");
    for (int i = 0; i < 4; ++i) SFM_REQUIRE(p->reserved[i] == 0, SFM_E_INVALID, "sfm_match_guided_params.reserved[%d] must be zero", i);
    if (num_jobs == 0) return SFM_OK;
    for (int k = 0; k < num_jobs; ++k) {
        const sfm_match_guided_job &j = jobs[k];
        SFM_REQUIRE(j.n1 >= 0 && j.n2 >= 0, SFM_E_INVALID, "jobs[%d]: negative point count", k);
        SFM_REQUIRE(!(j.n1 > 0 && j.n2 > 0) || (j.d_sift1 && j.d_sift2 && j.d_F), SFM_E_INVALID, "jobs[%d]: null pointer", k);
    }
    // no job's records to update on another job's records, second view or F (buffer_ranges.hpp); inside one job the single call's
    // rules hold: nothing is asked.  Empty jobs touch nothing and take no part.
    std::vector<BufferRange> ranges;
    ranges.reserve((size_t)3 * (size_t)num_jobs);
    for (int k = 0; k < num_jobs; ++k) {
        const sfm_match_guided_job &j = jobs[k];
        if (j.n1 <= 0 || j.n2 <= 0) continue;
        ranges.push_back(BufferRange{ j.d_sift1, (size_t)j.n1 * sizeof(sfm_sift_point), true, k, "d_sift1" });
        ranges.push_back(BufferRange{ j.d_sift2, (size_t)j.n2 * sizeof(sfm_sift_point), false, k, "d_sift2" });
        ranges.push_back(BufferRange{ j.d_F, 9 * sizeof(float), false, k, "d_F" });
    }
    const RangeConflict hit = first_conflict_across_overlapping_owners(ranges);
    SFM_REQUIRE(!hit, SFM_E_INVALID, "jobs[%d].%s overlaps jobs[%d].%s: a job's d_sift1 is written while the other job runs (two pairs that share a view need a copy of its records each)",
                hit.a->owner, hit.a->name, hit.b->owner, hit.b->name);
    GuidedJobPlan *jp = new (std::nothrow) GuidedJobPlan[(size_t)num_jobs];
    SFM_REQUIRE(jp, SFM_E_NOMEM, "host allocation failed");
    GuidedPairsPlan plan;
    const char *what = "";
    int rc = match_guided_pairs_plan(ctx->num_cus, jobs, num_jobs, sizeof(GuidedJob), jp, &plan, &what);
    if (rc != SFM_OK) set_error("sfm_match_guided_pairs: %s", what);
    else if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice failed"); rc = SFM_E_HIP; }
    else rc = launch_match_guided_pairs(ctx, jobs, num_jobs, jp, plan, p->band_px);
    delete[] jp;
    return rc;
}

} // namespace sfm

extern "C" {

int sfm_match_guided_pairs(sfm_ctx *ctx, const sfm_match_guided_job *jobs, int num_jobs, const sfm_match_guided_params *p)
{
    try {
        return sfm::match_guided_pairs_checked(ctx, jobs, num_jobs, p);
    } catch (const std::bad_alloc &) {
        sfm::set_error("host allocation failed");
        return SFM_E_NOMEM;
    } catch (...) {
        sfm::set_error("sfm_match_guided_pairs: unexpected host failure");
        return SFM_E_NOMEM;
    }
}

} // extern "C"
