// tests/hostcheck/matchguidedplancheck.cpp -- TEST HARNESS ONLY.
// Drives the real launch planner of sfm_match_guided_pairs (cuda-sfm_amd/csrc/match_guided_plan.hpp) and the buffer rule it is
// called behind (cuda-sfm_amd/csrc/buffer_ranges.hpp: first_conflict_across_overlapping_owners) from
// tests/test_match_guided_pairs_host.py.  Built by the plain host compiler: neither header includes a HIP header.  Its only
// allocations have num_jobs entries.  Nothing in the product loads this library.
#include <new>
#include <stdlib.h>
#include "../../cuda-sfm_amd/csrc/match_guided_plan.hpp"
#include "../../cuda-sfm_amd/csrc/buffer_ranges.hpp"

using namespace sfm;

// every allocation this library makes through operator new is seen here (linked -Bsymbolic-functions: the library's own calls
// bind to these definitions): the largest request since mgp_reset_largest_allocation tells whether anything scaled with n1
static size_t g_largest = 0;
static void *counted(size_t bytes) { if (bytes > g_largest) g_largest = bytes; return malloc(bytes ? bytes : 1); }
void *operator new(size_t bytes) { void *p = counted(bytes); if (!p) throw std::bad_alloc(); return p; }
void *operator new[](size_t bytes) { void *p = counted(bytes); if (!p) throw std::bad_alloc(); return p; }
void *operator new(size_t bytes, const std::nothrow_t &) noexcept { return counted(bytes); }
void *operator new[](size_t bytes, const std::nothrow_t &) noexcept { return counted(bytes); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

extern "C" {

void mgp_reset_largest_allocation(void) { g_largest = 0; }
uint64_t mgp_largest_allocation(void) { return (uint64_t)g_largest; }

// per_job: 8 int64 per job (launch, nsplit, rows_per_split, qblocks, first_unit, slot, tickets_off, partials_off);
// per_launch: 2 x 6 int64 (wv, jobs, qblocks, units, want, table_off); totals: tickets_off, tickets_bytes, workspace_bytes.
// Returns the planner's code, or -1000 when the probe's own arrays could not be allocated.
int mgp_plan(int num_cus, const int32_t *n1, const int32_t *n2, int num_jobs, uint64_t record_bytes,
             int64_t *per_job, int64_t *per_launch, uint64_t *totals, char *what, int what_bytes)
{
    sfm_match_guided_job *jobs = new (std::nothrow) sfm_match_guided_job[(size_t)num_jobs + 1];
    GuidedJobPlan *jp = new (std::nothrow) GuidedJobPlan[(size_t)num_jobs + 1];
    if (!jobs || !jp) { delete[] jobs; delete[] jp; return -1000; }
    for (int k = 0; k < num_jobs; ++k) jobs[k] = sfm_match_guided_job{ nullptr, n1[k], nullptr, n2[k], nullptr };
    GuidedPairsPlan plan;
    const char *w = "";
    const int rc = match_guided_pairs_plan(num_cus, jobs, num_jobs, (size_t)record_bytes, jp, &plan, &w);
    int i = 0;
    for (; w[i] && i + 1 < what_bytes; ++i) what[i] = w[i];
    if (what_bytes > 0) what[i] = 0;
    if (rc == SFM_OK) {
        for (int k = 0; k < num_jobs; ++k) {
            int64_t *o = per_job + 8 * (size_t)k;
            o[0] = jp[k].launch; o[1] = jp[k].nsplit; o[2] = jp[k].rows_per_split; o[3] = jp[k].qblocks; o[4] = jp[k].first_unit;
            o[5] = jp[k].slot; o[6] = (int64_t)jp[k].tickets_off; o[7] = (int64_t)jp[k].partials_off;
        }
        for (int c = 0; c < 2; ++c) {
            int64_t *o = per_launch + 6 * c;
            const GuidedLaunchPlan &l = plan.launch[c];
            o[0] = l.wv; o[1] = l.jobs; o[2] = l.qblocks; o[3] = l.units; o[4] = l.want; o[5] = (int64_t)l.table_off;
        }
        totals[0] = plan.tickets_off; totals[1] = plan.tickets_bytes; totals[2] = plan.workspace_bytes;
    }
    delete[] jobs;
    delete[] jp;
    return rc;
}

// 1 and the owners of the two ranges, or 0
int mgp_first_across_owners(const uint64_t *addr, const uint64_t *bytes, const int *out, const int *owner, int n, int *a, int *b)
{
    std::vector<BufferRange> r((size_t)n);
    for (int i = 0; i < n; ++i) r[(size_t)i] = { reinterpret_cast<const void *>((uintptr_t)addr[i]), (size_t)bytes[i], out[i] != 0, owner[i], "" };
    const RangeConflict c = first_conflict_across_overlapping_owners(r);
    if (!c) return 0;
    *a = c.a->owner; *b = c.b->owner;
    return 1;
}

}
