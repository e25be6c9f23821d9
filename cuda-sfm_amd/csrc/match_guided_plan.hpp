// match_guided_plan.hpp -- the launch plan of sfm_match_guided_pairs: a pure function from (the CU count, the jobs' sizes) to each
// job's configuration, split, first unit and workspace offsets, and each launch's unit count.  No HIP header: a host compiler
// builds this file alone (tests/hostcheck/matchguidedplancheck.cpp).
//
// The planner allocates nothing: its only arrays are the caller's, one entry per job.  Every count and every product is 64-bit
// or size_t, every sum that can leave its type is checked, and a plan that cannot be launched or addressed is REFUSED
// (SFM_E_INVALID) -- a job of 2^31 - 1 queries is a plan like any other (8.4 million query blocks), a list whose unit total
// passes 2^31 - 1 (the grid's x limit) is a refusal.  A workspace that merely does not fit the device is not the planner's
// business: the allocation fails with SFM_E_NOMEM.
//
// Configuration: (1,4) up to 4500 queries, (1,8) above -- exact_match_plan(..., max_ct = 1) of match_mfma.hpp; at most two
// launches, one per configuration.  Split: one budget per launch over all its jobs, about two rounds of blocks over the CUs in
// total (match_jobs_workspace, match.hip): want = ceil(2 CUs / total query blocks), job k takes min(want, ceil(n2 / 64)), its
// rows per split are rounded up to a multiple of 32 and the split count recomputed from them, as exact_match_plan does (a split's
// last stage may hold one row tile).  A unit is one (job, query block, split); a job's units are consecutive, split-major:
// unit = first_unit + split * qblocks + qblock, the order of the one-match launch's 2-D grid.
//
// Workspace: [table of launch 0][table of launch 1][tickets of every job][partials of every job].  Job k has one ticket (4 bytes)
// per query block and 12 bytes per (split, query) -- best, second, index as three arrays of nsplit * n1 words; the merge indexes
// them split * n1 + p1.  Every piece starts on a multiple of 256 bytes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/sfm_amd.h"

namespace sfm {

constexpr int64_t kGuidedMaxUnits = 2147483647;        // blocks of a 1-D grid
constexpr size_t kGuidedAlign = 256;

struct GuidedJobPlan {
    int launch;                    // 0: (1,4), 1: (1,8), -1: an empty job (n1 == 0 or n2 == 0), which takes part in nothing
    int32_t nsplit, rows_per_split;
    int64_t qblocks;
    int64_t first_unit;            // in its launch's grid
    int64_t slot;                  // its entry in its launch's table
    size_t tickets_off, partials_off;       // bytes from the workspace's base
};

struct GuidedLaunchPlan {
    int wv;                        // wavefronts per block: 4 or 8
    int64_t jobs, qblocks, units;
    int64_t want;                  // the split count the budget gives a job whose rows allow it
    size_t table_off;              // bytes from the workspace's base
};

struct GuidedPairsPlan {
    GuidedLaunchPlan launch[2];
    size_t tickets_off, tickets_bytes;      // the area zeroed before the launches
    size_t workspace_bytes;
};

inline int guided_wv(int32_t n1) { return n1 > 4500 ? 8 : 4; }

// a + b into *out, false when it does not fit size_t
inline bool guided_add(size_t a, size_t b, size_t *out)
{
    if (b > SIZE_MAX - a) return false;
    *out = a + b;
    return true;
}

// v rounded up to kGuidedAlign, false when it does not fit
inline bool guided_align(size_t v, size_t *out)
{
    if (!guided_add(v, kGuidedAlign - 1, out)) return false;
    *out &= ~(kGuidedAlign - 1);
    return true;
}

// jobs[k].n1, .n2 >= 0 (the caller has checked); out: num_jobs entries; job_record_bytes: the size of one entry of a launch's
// device table.  SFM_OK, or SFM_E_INVALID with *what naming the limit.
inline int match_guided_pairs_plan(int num_cus, const sfm_match_guided_job *jobs, int num_jobs, size_t job_record_bytes,
                                   GuidedJobPlan *out, GuidedPairsPlan *plan, const char **what)
{
    *what = "";
    for (int c = 0; c < 2; ++c) plan->launch[c] = GuidedLaunchPlan{ c ? 8 : 4, 0, 0, 0, 1, 0 };
    plan->tickets_off = plan->tickets_bytes = plan->workspace_bytes = 0;
    if (num_cus < 1) num_cus = 1;
    // 1: configurations and query blocks
    for (int k = 0; k < num_jobs; ++k) {
        GuidedJobPlan &j = out[k];
        j = GuidedJobPlan{ -1, 0, 0, 0, 0, 0, 0, 0 };
        const int64_t n1 = jobs[k].n1, n2 = jobs[k].n2;
        if (n1 <= 0 || n2 <= 0) continue;
        const int wv = guided_wv(jobs[k].n1);
        const int64_t qper = 32 * wv;
        j.launch = wv == 8 ? 1 : 0;
        j.qblocks = (n1 + qper - 1) / qper;
        GuidedLaunchPlan &l = plan->launch[j.launch];
        j.slot = l.jobs++;
        l.qblocks += j.qblocks;                         // (< 2^31 jobs of < 2^24 blocks each)
    }
    // 2: one split budget per launch, the units
    for (int c = 0; c < 2; ++c) {
        GuidedLaunchPlan &l = plan->launch[c];
        if (!l.jobs) continue;
        const int64_t want = (2 * (int64_t)num_cus + l.qblocks - 1) / l.qblocks;
        l.want = want < 1 ? 1 : want;                   // (<= 2 CUs)
    }
    for (int k = 0; k < num_jobs; ++k) {
        GuidedJobPlan &j = out[k];
        if (j.launch < 0) continue;
        GuidedLaunchPlan &l = plan->launch[j.launch];
        const int64_t n2 = jobs[k].n2;
        int64_t nsplit = l.want;
        const int64_t most = (n2 + 63) / 64;
        if (nsplit > most) nsplit = most;
        if (nsplit < 1) nsplit = 1;
        int64_t rps = (n2 + nsplit - 1) / nsplit;
        rps = (rps + 31) / 32 * 32;                     // (<= 2^31 + 30: 64-bit until it is known to fit)
        nsplit = (n2 + rps - 1) / rps;
        if (rps > INT32_MAX) { *what = "a job's rows per split do not fit 32 bits"; return SFM_E_INVALID; }
        j.rows_per_split = (int32_t)rps;
        j.nsplit = (int32_t)nsplit;
        j.first_unit = l.units;
        l.units += j.qblocks * nsplit;                  // (< 2^24 x 2^25 per job, checked against the limit before the next is added)
        if (l.units > kGuidedMaxUnits) { *what = "a launch of more than 2^31 - 1 (job, query block, split) units"; return SFM_E_INVALID; }
    }
    // 3: the workspace
    size_t used = 0;
    for (int c = 0; c < 2; ++c) {
        plan->launch[c].table_off = used;
        const uint64_t bytes = (uint64_t)plan->launch[c].jobs * (uint64_t)job_record_bytes;      // (< 2^31 x a record)
        if (bytes > SIZE_MAX || !guided_add(used, (size_t)bytes, &used) || !guided_align(used, &used)) { *what = "the job tables do not fit size_t"; return SFM_E_INVALID; }
    }
    plan->tickets_off = used;
    for (int k = 0; k < num_jobs; ++k) {
        GuidedJobPlan &j = out[k];
        if (j.launch < 0) continue;
        j.tickets_off = used;
        if (!guided_add(used, (size_t)j.qblocks * 4, &used) || !guided_align(used, &used)) { *what = "the tickets do not fit size_t"; return SFM_E_INVALID; }
    }
    plan->tickets_bytes = used - plan->tickets_off;
    for (int k = 0; k < num_jobs; ++k) {
        GuidedJobPlan &j = out[k];
        if (j.launch < 0) continue;
        j.partials_off = used;
        const uint64_t words = (uint64_t)j.nsplit * (uint64_t)jobs[k].n1;                        // (< 2^25 x 2^31)
        const uint64_t bytes = words * 12;
        if (bytes > SIZE_MAX || !guided_add(used, (size_t)bytes, &used) || !guided_align(used, &used)) { *what = "the partials do not fit size_t"; return SFM_E_INVALID; }
    }
    plan->workspace_bytes = used;
    return SFM_OK;
}

} // namespace sfm
