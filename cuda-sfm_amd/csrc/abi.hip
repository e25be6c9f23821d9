// abi.hip -- implementation of the C ABI declared in include/sfm_amd.h (its two host-side drivers: views.hip, pairs.hip).
#include "common.hpp"
#include "buffer_ranges.hpp"
#include "device_math.hpp"
#include "fuse_math.hpp"
#include "chain_adjust_math.hpp"
#include "ring_math.hpp"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <atomic>
#include <vector>
#include <algorithm>
#include <initializer_list>

namespace sfm {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

template <typename T>
static int dev_alloc(T **p, size_t count)
{
    SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
    return SFM_OK;
}

static int resolve_shard(const sfm_pair *pair, const sfm_ransac_params *p, uint32_t *h0, uint32_t *count)
{
    SFM_REQUIRE(pair && p, SFM_E_INVALID, "null pair/params");
    SFM_NEED(pair, kPoints);
    SFM_REQUIRE(pair->n >= 8, SFM_E_INVALID, "the 8-point solver needs at least 8 correspondences (have %d)", pair->n);
    SFM_REQUIRE(p->num_hypotheses > 0, SFM_E_INVALID, "num_hypotheses must be > 0");
    SFM_REQUIRE(p->hyp_begin <= p->num_hypotheses, SFM_E_INVALID, "hyp_begin %u beyond num_hypotheses %u", p->hyp_begin, p->num_hypotheses);
    SFM_REQUIRE(p->jacobi_sweeps >= 0 && p->jacobi_sweeps <= 64, SFM_E_INVALID, "jacobi_sweeps out of range (0 = Householder solver)");
    SFM_REQUIRE(p->kernel >= SFM_KERNEL_AUTO && p->kernel <= SFM_KERNEL_PREFILTER, SFM_E_INVALID, "unknown kernel id %d", p->kernel);
#if !SFM_AB
    SFM_REQUIRE(p->kernel != 3, SFM_E_INVALID, "kernel id 3 (f32 matrix-core scoring, a recorded A/B variant) exists only in libsfm_amd_ab.so");
    SFM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0 && p->reserved[3] == 0, SFM_E_INVALID,
                "sfm_ransac_params.reserved[] must be zero (the A/B switches exist only in libsfm_amd_ab.so, include/sfm_amd_ab.h)");
#endif
    uint32_t c = p->hyp_count ? p->hyp_count : p->num_hypotheses - p->hyp_begin;
    SFM_REQUIRE((uint64_t)p->hyp_begin + c <= p->num_hypotheses, SFM_E_INVALID, "shard [%u, %u) exceeds num_hypotheses %u",
                p->hyp_begin, p->hyp_begin + c, p->num_hypotheses);
    *h0 = p->hyp_begin;
    *count = c;
    return SFM_OK;
}

// buffers that are allocated together on first use: all of them or none
struct BufSpec { void **ptr; size_t bytes; };
static int alloc_group(std::initializer_list<BufSpec> bufs)
{
    int rc = SFM_OK;
    for (const BufSpec &b : bufs) if (rc == SFM_OK) rc = dev_alloc(reinterpret_cast<char **>(b.ptr), b.bytes);
    if (rc != SFM_OK) for (const BufSpec &b : bufs) { if (*b.ptr) (void)hipFree(*b.ptr); *b.ptr = nullptr; }
    return rc;
}

// d_rreproj / d_vreproj: one float error per point, then one uint8 flag per point (used / inlier)
static size_t reproj_bytes(size_t points) { return points * 5; }
static const uint8_t *reproj_flags(const sfm_pair *pair, const float *reproj) { return reinterpret_cast<const uint8_t *>(reproj + pair->n); }

// the Levenberg-Marquardt fields every params struct of a solver shares; most: the largest max_iterations the call takes
template <typename Params>
static int check_lm_params(const Params &p, const char *name, int most = 200)
{
    SFM_REQUIRE(p.reserved[0] == 0 && p.reserved[1] == 0 && p.reserved[2] == 0 && p.reserved[3] == 0, SFM_E_INVALID, "%s.reserved[] must be zero", name);
    SFM_REQUIRE(p.max_iterations >= 0 && p.max_iterations <= most, SFM_E_INVALID, "max_iterations %d outside 0..%d", p.max_iterations, most);
    SFM_REQUIRE(p.huber_px >= 0.0f && isfinite(p.huber_px), SFM_E_INVALID, "huber_px must be finite and >= 0");
    SFM_REQUIRE(isfinite(p.min_rel_decrease) && p.min_rel_decrease >= 0.0f, SFM_E_INVALID, "min_rel_decrease must be finite and >= 0");
    SFM_REQUIRE(isfinite(p.initial_lambda) && p.initial_lambda >= 0.0f, SFM_E_INVALID, "initial_lambda must be finite and >= 0");
    return SFM_OK;
}

static int copy_out(sfm_pair *pair, void *h_dst, const void *d_src, size_t bytes)
{
    SFM_FLUSH(pair);
    SFM_HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, pair->ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(pair->ctx->stream));
    return SFM_OK;
}

// ---- the pair list of a batched call: ONE gate for sfm_refine_pairs, sfm_register_views, sfm_triangulate_views, sfm_adjust_views,
// sfm_align_pairs (two lists, its entries are links[i]) and sfm_fuse_chain.  Two phases that every caller keeps apart:
// list_entries_present looks at the list alone and goes with the checks that read no pair; the three below it read the pairs and
// come after all of those.  The messages that differ between the calls are arguments: a format that takes the entry's index.
static int list_entries_present(sfm_pair *const *pairs, int count, const char *null_fmt)
{
    for (int i = 0; i < count; ++i) SFM_REQUIRE(pairs[i], SFM_E_INVALID, null_fmt, i);
    return SFM_OK;
}

// one context and -- with `why`, what would go wrong, given -- no handle twice: the later of the two entries is named.
// label: "pairs" / "links", as: "" / " as a".
static int list_one_context_each_once(sfm_pair *const *pairs, int count, const sfm_ctx *ctx, const char *other_fmt, const char *label,
                                      const char *as, const char *why)
{
    for (int i = 0; i < count; ++i) SFM_REQUIRE(pairs[i]->ctx == ctx, SFM_E_INVALID, other_fmt, i);
    std::vector<std::pair<const sfm_pair *, int>> sorted((size_t)(why ? count : 0));
    for (size_t i = 0; i < sorted.size(); ++i) sorted[i] = { pairs[i], (int)i };
    std::sort(sorted.begin(), sorted.end());
    for (size_t k = 1; k < sorted.size(); ++k)
        SFM_REQUIRE(sorted[k].first != sorted[k - 1].first, SFM_E_INVALID, "%s[%d]: the pair is listed twice%s (%s)", label, sorted[k].second, as, why);
    return SFM_OK;
}

static int list_flush(sfm_pair *const *pairs, int count)
{
    for (int i = 0; i < count; ++i) SFM_FLUSH(pairs[i]);
    return SFM_OK;
}

// every entry has the stages need(i); role: "" / "a: " / "b: "
template <typename Need>
static int list_stages(sfm_pair *const *pairs, int count, const char *label, const char *role, Need need)
{
    for (int i = 0; i < count; ++i) {
        const uint32_t stages = need(i);
        SFM_REQUIRE(pairs[i]->state.has(stages), SFM_E_STATE, "%s[%d]: %s%s", label, i, role, pair_stage_hint(pairs[i]->state.missing(stages)));
    }
    return SFM_OK;
}

// ---- no output on an input or on another output (buffer_ranges.hpp), as SFM_E_INVALID with the two names -----------------------
// inside one set; who: "" or "pairs[i]: " / "links[i]: "
static int check_ranges_in_set(const BufferRange *r, size_t count, const char *who)
{
    const RangeConflict c = first_conflict_in_set(r, count);
    SFM_REQUIRE(!c, SFM_E_INVALID, "%s%s overlaps %s", who, c.a->name, c.b->name);
    return SFM_OK;
}

// The entries of a batched call with the arrays' real lengths; table(i, r) writes entry i's per_entry ranges, owner i.  Inside
// every entry first, then across them: the blocks of different entries run at the same time, so no output may lie on an output
// or an input of another entry either (inputs may be shared).  This order is first_conflict_across_owners' precondition.
template <typename Table>
static int check_ranges_of_entries(int count, int per_entry, const char *label, Table table)
{
    std::vector<BufferRange> all((size_t)count * per_entry);
    char who[32];
    for (int i = 0; i < count; ++i) {
        BufferRange *r = &all[(size_t)i * per_entry];
        table(i, r);
        snprintf(who, sizeof(who), "%s[%d]: ", label, i);
        const int rc = check_ranges_in_set(r, (size_t)per_entry, who);
        if (rc != SFM_OK) return rc;
    }
    const RangeConflict c = first_conflict_across_owners(all);
    SFM_REQUIRE(!c, SFM_E_INVALID, "%s[%d]: a buffer overlaps a buffer of %s[%d], and one of the two is an output", label,
                std::max(c.a->owner, c.b->owner), label, std::min(c.a->owner, c.b->owner));
    return SFM_OK;
}

// rows of the second view that MatchSiftData visits (matching.cu:325: under SFM_QUIRK_MATCH_TAIL the tile loop stops 32 points short)
int match_db_rows(const sfm_ctx *ctx, int n2) { return (ctx->quirks & SFM_QUIRK_MATCH_TAIL) ? n2 - n2 % 32 : n2; }

// THE matcher rule for SiftPoint records (sfm_match, and every pair of sfm_process_pairs that is not part of a many-matches launch)
int match_records(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2, int *out_idx)
{
    n2 = match_db_rows(ctx, n2);
    if (n2 == 0) {                                                      // nothing left to match against: index -1 everywhere
        const int rc = launch_match_none(ctx, n1, d_sift1);
        if (rc == SFM_OK && out_idx) SFM_HIP_TRY(hipMemsetAsync(out_idx, 0xFF, (size_t)n1 * 4, ctx->stream));
        return rc;
    }
    const int ld = (int)(sizeof(sfm_sift_point) / sizeof(float));
    const int rc = launch_match(ctx, d_sift1->data, n1, ld, d_sift2->data, n2, ld, nullptr, nullptr, out_idx, d_sift1, d_sift2);
    if (rc != SFM_OK || !(ctx->quirks & SFM_QUIRK_MATCH_AMBIGUITY)) return rc;
    return launch_match_ambiguity_quirk(ctx, d_sift1->data, n1, ld, d_sift2->data, n2, ld, d_sift1, nullptr);      // matching.cu:378-396
}

// poses, triangulation and (d_record given) the pair's record on the device: one launch in SFM_POSE_REFERENCE, four otherwise
int pose_chain(sfm_pair *pair, int mode, float *d_record)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_FLUSH(pair);
    SFM_REQUIRE(mode == SFM_POSE_REFERENCE || mode == SFM_POSE_CORRECT, SFM_E_INVALID, "unknown pose mode %d", mode);
    SFM_NEED(pair, kE);
    if (mode == SFM_POSE_CORRECT) {               // the majority vote needs every point before the choice: three launches
        int rc = sfm_pose_candidates(pair, mode);
        if (rc == SFM_OK) rc = sfm_choose_pose(pair, mode);
        if (rc == SFM_OK) rc = sfm_triangulate(pair, mode);
        if (rc == SFM_OK && d_record) rc = launch_pair_record(pair, mode, d_record);
        return rc;
    }
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    const int rc = launch_pose_chain(pair, d_record);
    if (rc == SFM_OK) { pair->state.chain_done(); pair->pose_mode = mode; }
    return rc;
}

} // namespace sfm

using namespace sfm;

extern "C" {

int sfm_abi_version(void) { return SFM_ABI_VERSION; }
const char *sfm_last_error(void) { return g_err; }

int sfm_ctx_create(int device_id, sfm_ctx **out)
{
    SFM_REQUIRE(out, SFM_E_INVALID, "null out pointer");
    *out = nullptr;
    int ndev = 0;
    SFM_HIP_TRY(hipGetDeviceCount(&ndev));
    SFM_REQUIRE(device_id >= 0 && device_id < ndev, SFM_E_INVALID, "device %d not present (%d HIP devices)", device_id, ndev);
    SFM_HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    SFM_HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    sfm_ctx *c = new (std::nothrow) sfm_ctx();
    SFM_REQUIRE(c, SFM_E_NOMEM, "host allocation failed");
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) { delete c; set_error("hipEventCreate failed: %s", hipGetErrorString(e)); return SFM_E_HIP; }
    *out = c;
    return SFM_OK;
}

int sfm_ctx_retain(sfm_ctx *ctx)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    ctx->refs.fetch_add(1, std::memory_order_relaxed);
    return SFM_OK;
}

static int ctx_destroy_now(sfm_ctx *ctx);

// one reference less (a pair or a communicator went away); the last one destroys a context whose owner has already let go of it
static void ctx_release(sfm_ctx *ctx)
{
    if (!ctx) return;
    // whoever takes the count to zero destroys a context its owner has already let go of (fetch_sub decides: two threads releasing
    // at once cannot both see zero, nor both miss it)
    const int before = ctx->refs.fetch_sub(1, std::memory_order_acq_rel);
    if (before <= 0) { ctx->refs.fetch_add(1, std::memory_order_relaxed); return; }      // (release without a retain: ignored)
    if (before == 1 && ctx->destroy_requested.load(std::memory_order_acquire)) (void)ctx_destroy_now(ctx);
}

int sfm_ctx_release(sfm_ctx *ctx)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    ctx_release(ctx);
    return SFM_OK;
}

int sfm_ctx_destroy(sfm_ctx *ctx)
{
    if (!ctx) return SFM_OK;
    // The owner's handle counts as one reference from here on: taken, the request flagged, given back -- so that "the last one
    // destroys" is decided by ONE fetch_sub whether the last pair goes before, after or during this call.
    ctx->refs.fetch_add(1, std::memory_order_relaxed);
    ctx->destroy_requested.store(true, std::memory_order_release);
    if (ctx->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) return ctx_destroy_now(ctx);
    return SFM_OK;                               // pairs / communicators still point here: the last of them destroys the context
}

static int ctx_destroy_now(sfm_ctx *ctx)
{
    (void)hipSetDevice(ctx->device);
    // a borrowed stream (sfm_ctx_set_stream: e.g. a torch stream) may already have been destroyed by its owner when a deferred
    // destruction gets here: wait for the device instead of touching it
    if (ctx->own_stream || !ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    else (void)hipDeviceSynchronize();
    if (ctx->match_poll_flag) (void)hipHostFree(ctx->match_poll_flag);
    if (ctx->match_ws) (void)hipFree(ctx->match_ws);
    if (ctx->match_poll_ws) (void)hipFree(ctx->match_poll_ws);
    if (ctx->match_jobs_ws) (void)hipFree(ctx->match_jobs_ws);
    if (ctx->match_pf_ws) (void)hipFree(ctx->match_pf_ws);
    if (ctx->homo_ws) (void)hipFree(ctx->homo_ws);
    if (ctx->sift_temp) (void)hipFree(ctx->sift_temp);
    if (ctx->sift_ws) (void)hipFree(ctx->sift_ws);
    if (ctx->pool_pair) (void)sfm_pair_destroy(ctx->pool_pair);
    for (sfm_ctx *l : ctx->lane) if (l) (void)sfm_ctx_destroy(l);
    for (hipEvent_t e : ctx->lane_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->pool_records) (void)hipFree(ctx->pool_records);
    if (ctx->batch_ws) (void)hipFree(ctx->batch_ws);
    if (ctx->views_pinned) (void)hipHostFree(ctx->views_pinned);
    if (ctx->views_image) (void)hipFree(ctx->views_image);
    if (ctx->views_ev) (void)hipEventDestroy(ctx->views_ev);
    sift_job_free(ctx);
    job_array_free(ctx->refine_jobs);
    job_array_free(ctx->register_jobs);
    job_array_free(ctx->view_points_jobs);
    job_array_free(ctx->adjust_jobs);
    job_array_free(ctx->align_jobs);
    job_array_free(ctx->fuse_jobs);
    if (ctx->fuse_ws) (void)hipFree(ctx->fuse_ws);
    job_array_free(ctx->chain_jobs);
    if (ctx->chain_ws) (void)hipFree(ctx->chain_ws);
    job_array_free(ctx->ring_jobs);
    job_array_free(ctx->fundamental_jobs);
    job_array_free(ctx->guided_jobs);
    if (ctx->ring_ws) (void)hipFree(ctx->ring_ws);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (auto &t : ctx->tev) for (hipEvent_t e : t) if (e) (void)hipEventDestroy(e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    delete ctx;
    return SFM_OK;
}

int sfm_ctx_set_stream(sfm_ctx *ctx, void *hip_stream)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    if (ctx->own_stream && ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return SFM_OK;
}

int sfm_ctx_set_quirks(sfm_ctx *ctx, unsigned int flags)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_REQUIRE((flags & ~(SFM_QUIRK_MATCH_TAIL | SFM_QUIRK_MATCH_AMBIGUITY)) == 0, SFM_E_INVALID, "unknown quirk flags 0x%x", flags);
    ctx->quirks = flags;
    for (sfm_ctx *l : ctx->lane) if (l) l->quirks = flags;          // the lane contexts of sfm_process_pairs / sfm_extract_views
    return SFM_OK;
}

int sfm_ctx_set_match_kernel(sfm_ctx *ctx, int kernel)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_REQUIRE(kernel == SFM_MATCH_AUTO || kernel == SFM_MATCH_EXACT || kernel == SFM_MATCH_PREFILTER || kernel == SFM_MATCH_FUSED, SFM_E_INVALID, "unknown matcher %d", kernel);
    ctx->match_kernel = kernel;
    for (sfm_ctx *l : ctx->lane) if (l) l->match_kernel = kernel;
    return SFM_OK;
}

int sfm_ctx_last_match_kernel(sfm_ctx *ctx, int *kernel)
{
    SFM_REQUIRE(ctx && kernel, SFM_E_INVALID, "null argument");
    *kernel = ctx->last_match_kernel;
    return SFM_OK;
}

int sfm_ctx_own_stream(sfm_ctx *ctx)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    if (ctx->own_stream) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    hipStream_t st = nullptr;
    SFM_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    ctx->stream = st;
    ctx->own_stream = true;
    return SFM_OK;
}

int sfm_ctx_synchronize(sfm_ctx *ctx)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return match_poll_check(ctx);
}

int sfm_ctx_get_stream(sfm_ctx *ctx, void **hip_stream)
{
    SFM_REQUIRE(ctx && hip_stream, SFM_E_INVALID, "null argument");
    *hip_stream = static_cast<void *>(ctx->stream);
    return SFM_OK;
}

int sfm_ctx_get_device(sfm_ctx *ctx, int *device_id)
{
    SFM_REQUIRE(ctx && device_id, SFM_E_INVALID, "null argument");
    *device_id = ctx->device;
    return SFM_OK;
}

int sfm_ctx_timer_start(sfm_ctx *ctx)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return SFM_OK;
}

int sfm_ctx_timer_stop(sfm_ctx *ctx, float *elapsed_ms)
{
    SFM_REQUIRE(ctx && elapsed_ms, SFM_E_INVALID, "null argument");
    SFM_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    SFM_HIP_TRY(hipEventSynchronize(ctx->ev1));
    SFM_HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return SFM_OK;
}

int sfm_ctx_kernel_timing(sfm_ctx *ctx, int enable)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    if (enable && !ctx->tev[0][0]) {
        for (auto &t : ctx->tev) for (hipEvent_t &e : t) SFM_HIP_TRY(hipEventCreate(&e));
    }
    ctx->timing = enable != 0;
    ctx->tcount = 0;
    return SFM_OK;
}

int sfm_ctx_kernel_timing_read(sfm_ctx *ctx, float *solve_ms, float *score_ms, int *calls)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    float a = 0.f, b = 0.f;
    for (int i = 0; i < ctx->tcount; ++i) {
        float t = 0.f;
        SFM_HIP_TRY(hipEventElapsedTime(&t, ctx->tev[i][0], ctx->tev[i][1])); a += t;
        SFM_HIP_TRY(hipEventElapsedTime(&t, ctx->tev[i][1], ctx->tev[i][2])); b += t;
    }
    if (solve_ms) *solve_ms = a;
    if (score_ms) *score_ms = b;
    if (calls) *calls = ctx->tcount;
    ctx->tcount = 0;
    return SFM_OK;
}

int sfm_device_alloc(sfm_ctx *ctx, size_t bytes, void **d_ptr)
{
    SFM_REQUIRE(ctx && d_ptr, SFM_E_INVALID, "null argument");
    *d_ptr = nullptr;
    if (bytes == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipMalloc(d_ptr, bytes));
    return SFM_OK;
}

int sfm_device_free(sfm_ctx *ctx, void *d_ptr)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    if (!d_ptr) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    SFM_HIP_TRY(hipFree(d_ptr));
    return SFM_OK;
}

int sfm_copy_to_device(sfm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    SFM_REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), SFM_E_INVALID, "null argument");
    if (bytes == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SFM_OK;
}

int sfm_copy_to_host(sfm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    SFM_REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), SFM_E_INVALID, "null argument");
    if (bytes == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SFM_OK;
}

int sfm_copy_to_host_2d(sfm_ctx *ctx, void *h_dst, size_t dst_pitch, const void *d_src, size_t src_pitch,
                        size_t width_bytes, size_t height)
{
    SFM_REQUIRE(ctx && h_dst && d_src, SFM_E_INVALID, "null argument");
    if (width_bytes == 0 || height == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipMemcpy2DAsync(h_dst, dst_pitch, d_src, src_pitch, width_bytes, height, hipMemcpyDeviceToHost, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SFM_OK;
}

int sfm_copy_to_device_2d(sfm_ctx *ctx, void *d_dst, size_t dst_pitch, const void *h_src, size_t src_pitch,
                          size_t width_bytes, size_t height)
{
    SFM_REQUIRE(ctx && d_dst && h_src, SFM_E_INVALID, "null argument");
    if (width_bytes == 0 || height == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    SFM_HIP_TRY(hipMemcpy2DAsync(d_dst, dst_pitch, h_src, src_pitch, width_bytes, height, hipMemcpyHostToDevice, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SFM_OK;
}

// ---- match ------------------------------------------------------------------------------------
int sfm_match(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_REQUIRE(n1 >= 0 && n2 >= 0, SFM_E_INVALID, "negative point count");
    if (n1 == 0 || n2 == 0 || !d_sift1 || !d_sift2) return SFM_OK;      // matching.cu:1095-1102
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return match_records(ctx, d_sift1, n1, d_sift2, n2, nullptr);
}

int sfm_match_soa(sfm_ctx *ctx, const float *d_desc1, int n1, int ld1, const float *d_desc2, int n2, int ld2,
                  float *d_best, float *d_second, int32_t *d_index)
{
    SFM_REQUIRE(ctx, SFM_E_INVALID, "null context");
    SFM_REQUIRE(n1 >= 0 && n2 >= 0, SFM_E_INVALID, "negative point count");
    if (n1 == 0 || n2 == 0) return SFM_OK;
    SFM_REQUIRE(d_desc1 && d_desc2, SFM_E_INVALID, "null descriptor pointer");
    SFM_REQUIRE(ld1 >= 128 && ld2 >= 128 && ld1 % 4 == 0 && ld2 % 4 == 0, SFM_E_INVALID, "row strides must be >= 128 and multiples of 4 floats");
    SFM_REQUIRE(((uintptr_t)d_desc1 & 15) == 0 && ((uintptr_t)d_desc2 & 15) == 0, SFM_E_INVALID, "descriptor rows must be 16-byte aligned");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    const int rc = launch_match(ctx, d_desc1, n1, ld1, d_desc2, n2, ld2, d_best, d_second, d_index, nullptr, nullptr);
    if (rc != SFM_OK || !(ctx->quirks & SFM_QUIRK_MATCH_AMBIGUITY) || !d_second) return rc;
    return launch_match_ambiguity_quirk(ctx, d_desc1, n1, ld1, d_desc2, n2, ld2, nullptr, d_second);
}

// ---- guided match (match_guided.hip) ---------------------------------------------------------------
void sfm_match_guided_default_params(sfm_match_guided_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->band_px = 4.0f;
}

int sfm_match_guided(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2,
                     const float *d_F, const sfm_match_guided_params *p)
{
    SFM_REQUIRE(ctx && d_sift1 && d_sift2 && d_F && p, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(n1 >= 0 && n2 >= 0, SFM_E_INVALID, "negative point count");
    SFM_REQUIRE(p->band_px > 0.0f && p->band_px < __builtin_inff(), SFM_E_INVALID, "sfm_match_guided_params.band_px must be finite and > 0");
    for (int i = 0; i < 4; ++i) SFM_REQUIRE(p->reserved[i] == 0, SFM_E_INVALID, "sfm_match_guided_params.reserved[%d] must be zero", i);
    if (n1 == 0 || n2 == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_match_guided(ctx, d_sift1, n1, d_sift2, n2, d_F, p->band_px);
}

int sfm_pair_fundamental(sfm_pair *pair, int refined, float *d_F)
{
    SFM_REQUIRE(pair && d_F, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(refined == 0 || refined == 1, SFM_E_INVALID, "refined must be 0 or 1");
    SFM_FLUSH(pair);
    if (refined) SFM_NEED(pair, kRefined); else SFM_NEED(pair, kE);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    return launch_pair_fundamental(pair, refined, d_F);
}

int sfm_pair_fundamentals(sfm_pair *const *pairs, int num_pairs, int refined, float *d_F)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(pairs && d_F, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(num_pairs >= 0, SFM_E_INVALID, "negative pair count");
    SFM_REQUIRE(refined == 0 || refined == 1, SFM_E_INVALID, "refined must be 0 or 1");
    if (num_pairs == 0) return SFM_OK;
    int rc = list_entries_present(pairs, num_pairs, "pairs[%d] is null");
    if (rc != SFM_OK) return rc;
    sfm_ctx *ctx = pairs[0]->ctx;
    rc = list_one_context_each_once(pairs, num_pairs, ctx, "pairs[%d] belongs to another context than pairs[0]", "pairs", "", "a pair has one F");
    if (rc == SFM_OK) rc = list_flush(pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(pairs, num_pairs, "pairs", "", [refined](int) { return (uint32_t)(refined ? kRefined : kE); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_pair_fundamentals(ctx, pairs, num_pairs, refined, d_F);
}

// ---- ExtractSift ---------------------------------------------------------------------------------
int sfm_sift_temp_layout(int width, int height, int num_octaves, int scale_up, sfm_sift_layout *layout)
{
    SFM_REQUIRE(layout, SFM_E_INVALID, "null layout");
    SFM_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384, SFM_E_INVALID, "image size %d x %d", width, height);
    SFM_REQUIRE(num_octaves >= 1 && num_octaves <= 7, SFM_E_INVALID, "num_octaves %d outside 1..7", num_octaves);
    sift_layout(width, height, num_octaves, scale_up, layout);
    return SFM_OK;
}

int sfm_extract_sift(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height,
                     int pitch, int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up,
                     float *d_temp, int *num_pts, int *num_stored)
{
    SFM_REQUIRE(ctx && d_sift && d_image && num_pts, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384 && pitch >= width, SFM_E_INVALID,
                "image %d x %d pitch %d", width, height, pitch);
    SFM_REQUIRE(num_octaves >= 1 && num_octaves <= 7, SFM_E_INVALID, "num_octaves %d outside 1..7", num_octaves);
    SFM_REQUIRE(max_pts > 0, SFM_E_INVALID, "max_pts %d", max_pts);
    *num_pts = 0;
    if (num_stored) *num_stored = 0;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_extract_sift(ctx, d_sift, max_pts, d_image, width, height, pitch, num_octaves, init_blur, thresh, lowest_scale,
                               scale_up ? 1 : 0, d_temp, num_pts, num_stored);
}

int sfm_extract_sift_begin(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height,
                           int pitch, int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up, float *d_temp)
{
    SFM_REQUIRE(ctx && d_sift && d_image, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384 && pitch >= width, SFM_E_INVALID,
                "image %d x %d pitch %d", width, height, pitch);
    SFM_REQUIRE(num_octaves >= 1 && num_octaves <= 7, SFM_E_INVALID, "num_octaves %d outside 1..7", num_octaves);
    SFM_REQUIRE(max_pts > 0, SFM_E_INVALID, "max_pts %d", max_pts);
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_extract_sift_begin(ctx, d_sift, max_pts, d_image, width, height, pitch, num_octaves, init_blur, thresh, lowest_scale,
                                     scale_up ? 1 : 0, d_temp);
}

int sfm_extract_sift_end(sfm_ctx *ctx, int *num_pts, int *num_stored)
{
    SFM_REQUIRE(ctx && num_pts, SFM_E_INVALID, "null argument");
    *num_pts = 0;
    if (num_stored) *num_stored = 0;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_extract_sift_end(ctx, num_pts, num_stored);
}

// ---- FindHomography ------------------------------------------------------------------------------
int sfm_find_homography(sfm_ctx *ctx, const sfm_sift_point *d_sift, int num_pts, float h_H[9], int *num_matches,
                        int num_loops, float min_score, float max_ambiguity, float thresh, uint32_t seed,
                        const int32_t *h_pts, int32_t *h_counts, float *h_homo)
{
    SFM_REQUIRE(ctx && h_H && num_matches, SFM_E_INVALID, "null argument");
    *num_matches = 0;
    for (int i = 0; i < 9; ++i) h_H[i] = (i % 4 == 0) ? 1.0f : 0.0f;           // matching.cu:1002-1005
    if (!d_sift || num_pts < 8 || num_loops <= 0) return SFM_OK;                // matching.cu:1010-1018
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    const int L = round_up(num_loops, 16);                                      // matching.cu:1015
    if (h_pts) {
        for (size_t i = 0; i < (size_t)4 * L; ++i)
            SFM_REQUIRE(h_pts[i] >= 0 && h_pts[i] < num_pts, SFM_E_INVALID, "sample index %d out of range", h_pts[i]);
    }
    // without an explicit sample the score / ambiguity gate (matching.cu:1030-1036) and the seeded sampler run on the device
    int num_valid = 0;
    return launch_homography(ctx, d_sift, num_pts, h_pts, L, thresh, min_score, max_ambiguity, seed, &num_valid, h_H, num_matches, h_counts, h_homo);
}

// ---- Image_pair ---------------------------------------------------------------------------------
int sfm_pair_create(sfm_ctx *ctx, const float h_K[9], const float h_Kinv[9], int image_count, int num_points, sfm_pair **out)
{
    SFM_REQUIRE(out, SFM_E_INVALID, "null out pointer");
    *out = nullptr;
    SFM_REQUIRE(ctx && h_K && h_Kinv, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(image_count == 2, SFM_E_INVALID, "image_count must be 2 (the reference only ever uses two views, sfm.h:31)");
    SFM_REQUIRE(num_points > 0, SFM_E_INVALID, "num_points must be positive");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    sfm_pair *p = new (std::nothrow) sfm_pair();
    SFM_REQUIRE(p, SFM_E_NOMEM, "host allocation failed");
    p->ctx = ctx;
    p->holds_ctx_ref = true; ctx->refs++;
    p->image_count = image_count;
    p->n = num_points;
    p->cap_points = num_points;
    p->ld = round_up(num_points, 128);
    memcpy(p->h_Kinv, h_Kinv, sizeof(p->h_Kinv));
    int rc = SFM_OK;
    auto A = [&](auto **ptr, size_t count) { if (rc == SFM_OK) rc = dev_alloc(ptr, count); };
    A(&p->d_K, 9); A(&p->d_Kinv, 9);
    for (int i = 0; i < 2; ++i) { A(&p->d_U[i], (size_t)3 * p->ld); A(&p->d_X[i], (size_t)3 * p->ld); }
    A(&p->d_pts4, (size_t)p->ld);
    A(&p->d_E, 9); A(&p->d_P, 64); A(&p->d_Pinv, 64); A(&p->d_Pind, 8);
    A(&p->d_points, (size_t)4 * num_points);
    A(&p->d_mask, (size_t)num_points);
    A(&p->slot[0].key, 2); A(&p->d_best, 2); A(&p->d_clk, kClkWords); A(&p->d_bound, 10);      // [0] bound (fill_xu_kernel), [2..9] the coordinate boxes (pf_cells_build_kernel)
    if (rc != SFM_OK) { sfm_pair_destroy(p); return rc; }
    hipError_t e = hipMemcpyAsync(p->d_K, h_K, 9 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_Kinv, h_Kinv, 9 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->slot[0].key, 0, 2 * sizeof(unsigned long long), ctx->stream);
    p->state.key_clean = true;
    if (e == hipSuccess) e = hipMemsetAsync(p->d_best, 0, 2 * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_bound, 0, 10 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_clk, 0, kClkWords * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_Pind, 0, 8 * sizeof(int), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);       // host K arrays may go out of scope
    if (e != hipSuccess) { sfm_pair_destroy(p); set_error("pair init failed: %s", hipGetErrorString(e)); return SFM_E_HIP; }
    *out = p;
    return SFM_OK;
}

int sfm_pair_reset(sfm_pair *pair, int num_points)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_FLUSH(pair);
    SFM_REQUIRE(num_points > 0 && num_points <= pair->cap_points, SFM_E_INVALID,
                "num_points %d outside (0, %d] (the size the pair was created with)", num_points, pair->cap_points);
    pair->n = num_points;
    pair->ld = round_up(num_points, 128);
    pair->state.reset();
    return SFM_OK;
}

int sfm_pair_destroy(sfm_pair *p)
{
    if (!p) return SFM_OK;
    if (p->ctx) { (void)hipSetDevice(p->ctx->device); (void)hipStreamSynchronize(p->ctx->stream); }
    void *bufs[] = { p->d_K, p->d_Kinv, p->d_U[0], p->d_U[1], p->d_X[0], p->d_X[1], p->d_pts4, p->d_E, p->d_P, p->d_Pinv, p->d_Pind,
                     p->d_points, p->d_mask, p->d_best, p->d_clk, p->d_bound, p->d_cells, p->d_pts4s, p->d_tile_boxes, p->d_buckets,
                     p->d_rstate, p->d_rpoints, p->d_rreproj, p->d_rwork, p->d_vstate, p->d_vreproj, p->d_vwork, p->d_vhyp, p->d_vcounts, p->d_awork,
                     p->d_lwork, p->d_lhyp };
    for (void *b : bufs) if (b) (void)hipFree(b);
    for (ShardSlot &s : p->slot) shard_slot_free(s);
    if (p->pipe_stream) { (void)hipStreamSynchronize(p->pipe_stream); (void)hipStreamDestroy(p->pipe_stream); }
    for (hipEvent_t e : p->pipe_final) if (e) (void)hipEventDestroy(e);
    if (p->pipe_call) (void)hipEventDestroy(p->pipe_call);
    if (p->cells_ev) (void)hipEventDestroy(p->cells_ev);
    if (p->pipe_keys) (void)hipFree(p->pipe_keys);
    sfm_ctx *owner = p->holds_ctx_ref ? p->ctx : nullptr;
    delete p;
    ctx_release(owner);
    return SFM_OK;
}

int sfm_fill_xu(sfm_pair *pair, const sfm_sift_point *d_data)
{
    SFM_REQUIRE(pair && d_data, SFM_E_INVALID, "null argument");
    SFM_FLUSH(pair);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    const int rc = launch_fill_xu(pair, d_data);
    // X_z = fma(Kinv[8], 1, fma(Kinv[7], y, Kinv[6] * x)) is exactly 1 for finite pixel coordinates when
    // the last row of K^-1 is (0 0 1): the scoring kernel may then drop z (ransac_device.hpp)
    if (rc == SFM_OK) pair->state.points_filled(unit_z_Kinv(pair->h_Kinv));
    return rc;
}

int sfm_set_points(sfm_pair *pair, const float *d_X0, const float *d_X1)
{
    SFM_REQUIRE(pair && d_X0 && d_X1, SFM_E_INVALID, "null argument");
    SFM_FLUSH(pair);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    const int rc = launch_set_points(pair, d_X0, d_X1);
    if (rc == SFM_OK) pair->state.points_set();
    return rc;
}

void sfm_ransac_default_params(sfm_ransac_params *p, int num_points)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->num_hypotheses = num_points >= 8 ? (uint32_t)(num_points / 8) : 1u;     // sfm.cu:95
    p->seed = 0x5EED5F3Du;
    p->threshold = 1e-6f;                                                        // sfm.cu:220
    p->jacobi_sweeps = 0;                                                        // Householder null-vector solver
    p->kernel = SFM_KERNEL_AUTO;
}

int sfm_ransac_permutation_indices(sfm_ctx *ctx, int num_points, uint32_t seed, int32_t *d_indices)
{
    SFM_REQUIRE(ctx && d_indices, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(num_points >= 8, SFM_E_INVALID, "need at least 8 points");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_permutation_indices(ctx, num_points, seed, d_indices);
}

// the three plain scoring calls: the shard on the context's stream, behind a pending burst
static int score_shard(sfm_pair *pair, const sfm_ransac_params *p, uint64_t *d_key_out, const float *d_E)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_FLUSH(pair);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    return launch_ransac_score(pair, pair->slot[0], pair->ctx->stream, *p, h0, count, reinterpret_cast<unsigned long long *>(d_key_out), d_E);
}

int sfm_ransac_score(sfm_pair *pair, const sfm_ransac_params *p) { return score_shard(pair, p, nullptr, nullptr); }

int sfm_ransac_score_candidates(sfm_pair *pair, const sfm_ransac_params *p, const float *d_E)
{
    SFM_REQUIRE(d_E, SFM_E_INVALID, "null candidate pointer");
    return score_shard(pair, p, nullptr, d_E);
}

int sfm_ransac_score_into(sfm_pair *pair, const sfm_ransac_params *p, uint64_t *d_key_out)
{
    SFM_REQUIRE(d_key_out, SFM_E_INVALID, "null key pointer");
    return score_shard(pair, p, d_key_out, nullptr);
}

int sfm_ransac_score_into_slot(sfm_pair *pair, const sfm_ransac_params *p, uint64_t *d_key_out, int slot, void *hip_stream)
{
    SFM_REQUIRE(d_key_out, SFM_E_INVALID, "null key pointer");
    SFM_REQUIRE(slot == 0 || slot == 1, SFM_E_INVALID, "slot must be 0 or 1");
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : pair->ctx->stream;
    if (slot == 1 && !pair->slot[1].key) {
        SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pair->slot[1].key), 2 * sizeof(unsigned long long)));
        // cleared on the stream the launches below go to.  (Until round 6 this was a plain hipMemset: it runs on the NULL stream, which a
        // non-blocking stream does not wait for -- queued behind slot 0's kernels when the context works on the null stream, it cleared slot
        // 1's key while or after slot 1's first fused-kernel launch wrote it: the first pipelined call of a pair on slot 1 could finalize a
        // partial or empty key.  Found by the fuzz's stateful round; profiles/pipelined_burst_case.py.)
        SFM_HIP_TRY(hipMemsetAsync(pair->slot[1].key, 0, 2 * sizeof(unsigned long long), stream));
    }
    if (slot == 1) pair->state.key_clean = false;      // (the flag describes slot[0]'s key: a launch on slot 1 clears its key itself)
    return launch_ransac_score(pair, pair->slot[slot], stream, *p, h0, count, reinterpret_cast<unsigned long long *>(d_key_out), nullptr, /* serial */ false);
}

// Image_pair::estimateE for a STREAM of calls: step k runs on slot k % 2 (its own stream and per-shard buffers), so that
// consecutive calls overlap -- the next call's lane-solve kernel and launch gaps fill what this call's scoring kernel
// leaves idle.  Results (E, mask, best) are those of the last call once sfm_pair_flush has run.
int sfm_estimate_E_pipelined(sfm_pair *pair, const sfm_ransac_params *p)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(count > 0, SFM_E_INVALID, "empty hypothesis range");
    sfm_ctx *ctx = pair->ctx;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    if (!pair->pipe_stream) {
        SFM_HIP_TRY(hipStreamCreateWithFlags(&pair->pipe_stream, hipStreamNonBlocking));
        for (hipEvent_t &e : pair->pipe_final) SFM_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        SFM_HIP_TRY(hipEventCreateWithFlags(&pair->pipe_call, hipEventDisableTiming));
        SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pair->pipe_keys), 2 * sizeof(uint64_t)));
    }
    const int slot = (int)(pair->pipe_step & 1ull);
    hipStream_t st = slot ? pair->pipe_stream : ctx->stream;
    // What the caller enqueued on the context stream BEFORE this burst of pipelined calls (the points) must come first on
    // the second stream too -- marked once, when the burst starts: an event recorded later would sit behind the previous
    // step's kernels and serialise the two slots.
    if (!pair->pipe_pending) SFM_HIP_TRY(hipEventRecord(pair->pipe_call, ctx->stream));
    if (slot) SFM_HIP_TRY(hipStreamWaitEvent(st, pair->pipe_call, 0));
    rc = sfm_ransac_score_into_slot(pair, p, pair->pipe_keys + slot, slot, st);
    if (rc != SFM_OK) return rc;
    // E, mask and best exist once: the finalizes of consecutive steps keep their order across the two streams
    if (pair->pipe_step >= 1) SFM_HIP_TRY(hipStreamWaitEvent(st, pair->pipe_final[slot ^ 1], 0));
    rc = launch_ransac_finalize(pair, *p, reinterpret_cast<const unsigned long long *>(pair->pipe_keys + slot), 0, true, st, true);
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipEventRecord(pair->pipe_final[slot], st));
    pair->pipe_step++;
    pair->pipe_pending = true;
    pair->state.E_finalized();
    return SFM_OK;
}

int sfm_pair_flush(sfm_pair *pair)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    if (!pair->pipe_pending) return SFM_OK;
    const int last = (int)((pair->pipe_step - 1) & 1ull);
    SFM_HIP_TRY(hipStreamWaitEvent(pair->ctx->stream, pair->pipe_final[last], 0));     // the finalizes are ordered: the last one covers all
    pair->pipe_pending = false;
    return SFM_OK;
}

int sfm_ransac_finalize(sfm_pair *pair, const sfm_ransac_params *p, uint32_t hyp)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_FLUSH(pair);
    SFM_REQUIRE(hyp < p->num_hypotheses, SFM_E_INVALID, "hypothesis id %u out of range", hyp);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = launch_ransac_finalize(pair, *p, nullptr, hyp, false);
    if (rc == SFM_OK) pair->state.E_finalized();
    return rc;
}

int sfm_ransac_export_key(sfm_pair *pair, uint64_t *d_key_out)
{
    SFM_REQUIRE(pair && d_key_out, SFM_E_INVALID, "null argument");
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    SFM_HIP_TRY(hipMemcpyAsync(d_key_out, pair->slot[0].key, sizeof(uint64_t), hipMemcpyDeviceToDevice, pair->ctx->stream));
    return SFM_OK;
}

int sfm_ransac_finalize_key(sfm_pair *pair, const sfm_ransac_params *p, const uint64_t *d_key)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_FLUSH(pair);
    SFM_REQUIRE(d_key, SFM_E_INVALID, "null key pointer");
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = launch_ransac_finalize(pair, *p, reinterpret_cast<const unsigned long long *>(d_key), 0, true);
    if (rc == SFM_OK) pair->state.E_finalized();
    return rc;
}

int sfm_ransac_finalize_key_on(sfm_pair *pair, const sfm_ransac_params *p, const uint64_t *d_key, void *hip_stream)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(d_key, SFM_E_INVALID, "null key pointer");
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = launch_ransac_finalize(pair, *p, reinterpret_cast<const unsigned long long *>(d_key), 0, true,
                                static_cast<hipStream_t>(hip_stream), true);
    if (rc == SFM_OK) pair->state.E_finalized();
    return rc;
}

int sfm_estimate_E(sfm_pair *pair, const sfm_ransac_params *p)
{
    uint32_t h0, count;
    int rc = resolve_shard(pair, p, &h0, &count);
    if (rc != SFM_OK) return rc;
    SFM_FLUSH(pair);
    SFM_REQUIRE(count > 0, SFM_E_INVALID, "empty hypothesis range");
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = launch_ransac_score(pair, pair->slot[0], pair->ctx->stream, *p, h0, count);
    if (rc != SFM_OK) return rc;
    rc = launch_ransac_finalize(pair, *p, pair->slot[0].key, 0, true);     // arg-max stays on the device
    if (rc == SFM_OK) pair->state.E_finalized();
    return rc;
}

int sfm_pose_candidates(sfm_pair *pair, int mode)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_FLUSH(pair);
    SFM_REQUIRE(mode == SFM_POSE_REFERENCE || mode == SFM_POSE_CORRECT, SFM_E_INVALID, "unknown pose mode %d", mode);
    SFM_NEED(pair, kE);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    int rc = launch_pose_candidates(pair, mode);
    if (rc == SFM_OK) { pair->state.candidates_done(); pair->pose_mode = mode; }
    return rc;
}

int sfm_choose_pose(sfm_pair *pair, int mode)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_REQUIRE(mode == SFM_POSE_REFERENCE || mode == SFM_POSE_CORRECT, SFM_E_INVALID, "unknown pose mode %d", mode);
    SFM_NEED(pair, kP);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    int rc = launch_choose_pose(pair, mode);
    if (rc == SFM_OK) pair->state.pose_chosen();
    return rc;
}

int sfm_triangulate(sfm_pair *pair, int mode)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_REQUIRE(mode == SFM_POSE_REFERENCE || mode == SFM_POSE_CORRECT, SFM_E_INVALID, "unknown pose mode %d", mode);
    SFM_NEED(pair, kPose);
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    int rc = launch_triangulate(pair, mode);
    if (rc == SFM_OK) pair->state.triangulated();
    return rc;
}

int sfm_pose_chain(sfm_pair *pair, int mode) { return pose_chain(pair, mode, nullptr); }

// ---- two-view bundle adjustment (refine.hip) ------------------------------------------------------
void sfm_refine_default_params(sfm_refine_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 20;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// the refinement's per-pair buffers, allocated at the first call and sized to the creation-time count: sfm_pair_reset needs no reallocation
static int refine_buffers(sfm_pair *pair)
{
    if (pair->d_rstate) return SFM_OK;
    const size_t cap = (size_t)pair->cap_points;
    return alloc_group({ { reinterpret_cast<void **>(&pair->d_rstate), (size_t)refine_state_words() * 4 },
                         { reinterpret_cast<void **>(&pair->d_rpoints), 4 * cap * 4 },
                         { reinterpret_cast<void **>(&pair->d_rreproj), reproj_bytes(cap) },
                         { &pair->d_rwork, refine_work_bytes(pair->cap_points) } });
}

int sfm_refine_two_view(sfm_pair *pair, const sfm_refine_params *p)
{
    SFM_REQUIRE(pair && p, SFM_E_INVALID, "null argument");
    SFM_FLUSH(pair);
    SFM_NEED(pair, kE);
    int rc = check_lm_params(*p, "sfm_refine_params");
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = refine_buffers(pair);
    if (rc != SFM_OK) return rc;
    rc = launch_refine(pair, *p);
    if (rc == SFM_OK) pair->state.refined();
    return rc;
}

int sfm_refine_pairs(sfm_pair *const *pairs, int num_pairs, const sfm_refine_params *p, const uint8_t *const *d_masks)
{
    // the checks that need no device first, all of them before anything is enqueued or any pair changes
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, SFM_E_INVALID, "num_pairs %d outside 0..65535", num_pairs);
    if (num_pairs == 0) return SFM_OK;          // (the five later batched calls check the parameters whatever the count; this one never did)
    SFM_REQUIRE(pairs, SFM_E_INVALID, "null pair list");
    int rc = list_entries_present(pairs, num_pairs, "pairs[%d] is null");
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(!p->d_mask, SFM_E_INVALID, "sfm_refine_params.d_mask must be null here: per-pair masks go through d_masks");
    rc = check_lm_params(*p, "sfm_refine_params");
    if (rc != SFM_OK) return rc;
    sfm_ctx *ctx = pairs[0]->ctx;
    rc = list_one_context_each_once(pairs, num_pairs, ctx, "pairs[%d] belongs to another context than pairs[0]", "pairs", "", "two blocks would write the same buffers");
    if (rc == SFM_OK) rc = list_flush(pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)kE; });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 0; i < num_pairs; ++i) { rc = refine_buffers(pairs[i]); if (rc != SFM_OK) return rc; }
    rc = launch_refine_pairs(ctx, pairs, num_pairs, *p, d_masks);
    for (int i = 0; i < num_pairs; ++i) if (rc == SFM_OK) pairs[i]->state.refined();
    return rc;
}

int sfm_get_refine_report(sfm_pair *pair, sfm_refine_report *r)
{
    SFM_REQUIRE(pair && r, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kRefined);
    return copy_out(pair, r, pair->d_rstate + refine_report_offset(), sizeof(*r));
}

int sfm_get_refined_pose(sfm_pair *pair, float h_P[16], float h_E[9])
{
    SFM_REQUIRE(pair && (h_P || h_E), SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kRefined);
    float v[25];
    const int rc = copy_out(pair, v, pair->d_rstate + refine_pose_offset(), sizeof(v));
    if (rc != SFM_OK) return rc;
    if (h_P) memcpy(h_P, v, 16 * sizeof(float));
    if (h_E) memcpy(h_E, v + 16, 9 * sizeof(float));
    return SFM_OK;
}

int sfm_get_refined_points(sfm_pair *pair, float *h_points)
{
    SFM_REQUIRE(pair && h_points, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kRefined);
    return copy_out(pair, h_points, pair->d_rpoints, (size_t)4 * pair->n * 4);
}

int sfm_get_reprojection_errors(sfm_pair *pair, float *h_err, uint8_t *h_used)
{
    SFM_REQUIRE(pair && h_err, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kRefined);
    const int rc = copy_out(pair, h_err, pair->d_rreproj, (size_t)pair->n * 4);
    if (rc != SFM_OK || !h_used) return rc;
    return copy_out(pair, h_used, reproj_flags(pair, pair->d_rreproj), (size_t)pair->n);
}

// ---- registering a further view (register.hip) ----------------------------------------------------
void sfm_register_default_params(sfm_register_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->num_hypotheses = 4096;
    p->seed = 0x5EED5F3Du;
    p->threshold_px = 4.0f;
    p->min_score = 0.85f;
    p->max_ambiguity = 0.95f;
    p->max_iterations = 10;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// the parameter checks of sfm_register_view and sfm_register_views (none needs a device)
static int check_register_params(const sfm_register_params &p)
{
    const int rc = check_lm_params(p, "sfm_register_params");
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p.num_hypotheses >= 1 && p.num_hypotheses <= (1u << 20), SFM_E_INVALID, "num_hypotheses %u outside 1..2^20", p.num_hypotheses);
    SFM_REQUIRE(isfinite(p.threshold_px) && p.threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    SFM_REQUIRE(isfinite(p.min_score) && isfinite(p.max_ambiguity), SFM_E_INVALID, "min_score / max_ambiguity must be finite");
    return SFM_OK;
}

// the registration's per-pair buffers: the per-point ones allocated at the first call, the per-hypothesis ones grown on demand
static int register_buffers(sfm_pair *pair, uint32_t num_hypotheses)
{
    int rc = SFM_OK;
    if (!pair->d_vstate) {                              // sized to the creation-time count: sfm_pair_reset needs no reallocation
        rc = alloc_group({ { reinterpret_cast<void **>(&pair->d_vstate), (size_t)register_state_words() * 4 },
                           { reinterpret_cast<void **>(&pair->d_vreproj), reproj_bytes((size_t)pair->cap_points) },
                           { &pair->d_vwork, register_work_bytes(pair->cap_points) } });
        if (rc != SFM_OK) return rc;
    }
    if (num_hypotheses > pair->cap_vhyps) {             // grows with the largest num_hypotheses seen (the old buffers may be in use)
        pair->state.view_dropped();
        pair->cap_vhyps = 0;                            // ... until BOTH buffers exist again (d_vhyp has no size of its own)
        size_t hyp_bytes = 0;
        rc = grow(&pair->d_vhyp, &hyp_bytes, register_hyp_bytes(num_hypotheses), pair->ctx->stream);
        if (rc == SFM_OK) rc = grow(&pair->d_vcounts, &pair->cap_vhyps, num_hypotheses, pair->ctx->stream);
    }
    return rc;
}

int sfm_register_view(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_register_params *p)
{
    SFM_REQUIRE(pair && d_sift && p, SFM_E_INVALID, "null argument");
    SFM_FLUSH(pair);
    int rc = check_register_params(*p);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p->d_points || !p->d_valid, SFM_E_INVALID, "d_valid needs d_points");
    SFM_NEED(pair, p->d_points ? kPoints : kPoints | kRefined);       // without d_points: the refined points, on the current points
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = register_buffers(pair, p->num_hypotheses);
    if (rc != SFM_OK) return rc;
    const float *d_points = p->d_points ? p->d_points : pair->d_rpoints;
    const uint8_t *d_valid = p->d_points ? p->d_valid : reproj_flags(pair, pair->d_rreproj);   // the used flags
    rc = launch_register(pair, d_sift, *p, d_points, d_valid);
    if (rc == SFM_OK) { pair->state.view_registered(); pair->view_hyps = p->num_hypotheses; }
    return rc;
}

int sfm_register_views(sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts, const sfm_register_params *p,
                       const float *const *d_points, const uint8_t *const *d_valid)
{
    // the checks that need no device first, all of them before anything is enqueued or any pair changes
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, SFM_E_INVALID, "num_pairs %d outside 0..65535", num_pairs);
    SFM_REQUIRE(!p->d_points && !p->d_valid, SFM_E_INVALID,
                "sfm_register_params.d_points / d_valid must be null here: per-pair points go through d_points / d_valid");
    int rc = check_register_params(*p);
    if (rc != SFM_OK) return rc;
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(pairs && d_sifts, SFM_E_INVALID, "null pair list or null d_sifts list");
    rc = list_entries_present(pairs, num_pairs, "pairs[%d] is null");
    if (rc != SFM_OK) return rc;
    for (int i = 0; i < num_pairs; ++i) {
        SFM_REQUIRE(d_sifts[i], SFM_E_INVALID, "d_sifts[%d] is null", i);
        SFM_REQUIRE(!(d_valid && d_valid[i]) || (d_points && d_points[i]), SFM_E_INVALID, "d_valid[%d] needs d_points[%d]", i, i);
    }
    sfm_ctx *ctx = pairs[0]->ctx;
    rc = list_one_context_each_once(pairs, num_pairs, ctx, "pairs[%d] belongs to another context than pairs[0]", "pairs", "", "a pair holds one registered view");
    if (rc == SFM_OK) rc = list_flush(pairs, num_pairs);
    // without points: the refined ones, on the current points
    if (rc == SFM_OK) rc = list_stages(pairs, num_pairs, "pairs", "", [&](int i) { return (uint32_t)((d_points && d_points[i]) ? kPoints : kPoints | kRefined); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 0; i < num_pairs; ++i) { rc = register_buffers(pairs[i], p->num_hypotheses); if (rc != SFM_OK) return rc; }
    std::vector<const float *> points((size_t)num_pairs);
    std::vector<const uint8_t *> valid((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const bool given = d_points && d_points[i];
        points[(size_t)i] = given ? d_points[i] : pairs[i]->d_rpoints;
        valid[(size_t)i] = given ? (d_valid ? d_valid[i] : nullptr) : reproj_flags(pairs[i], pairs[i]->d_rreproj);   // the used flags
    }
    rc = launch_register_views(ctx, pairs, num_pairs, d_sifts, *p, points.data(), valid.data());
    for (int i = 0; i < num_pairs; ++i) if (rc == SFM_OK) { pairs[i]->state.view_registered(); pairs[i]->view_hyps = p->num_hypotheses; }
    return rc;
}

int sfm_get_register_report(sfm_pair *pair, sfm_register_report *r)
{
    SFM_REQUIRE(pair && r, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kView);
    return copy_out(pair, r, pair->d_vstate + register_report_offset(), sizeof(*r));
}

int sfm_get_view_pose(sfm_pair *pair, float h_P[16], float h_P_ransac[16])
{
    SFM_REQUIRE(pair && (h_P || h_P_ransac), SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kView);
    float v[32];
    const int rc = copy_out(pair, v, pair->d_vstate + register_pose_offset(), sizeof(v));
    if (rc != SFM_OK) return rc;
    if (h_P) memcpy(h_P, v, 16 * sizeof(float));
    if (h_P_ransac) memcpy(h_P_ransac, v + 16, 16 * sizeof(float));
    return SFM_OK;
}

int sfm_get_view_errors(sfm_pair *pair, float *h_err, uint8_t *h_inlier)
{
    SFM_REQUIRE(pair && h_err, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kView);
    const int rc = copy_out(pair, h_err, pair->d_vreproj, (size_t)pair->n * 4);
    if (rc != SFM_OK || !h_inlier) return rc;
    return copy_out(pair, h_inlier, reproj_flags(pair, pair->d_vreproj), (size_t)pair->n);
}

int sfm_get_view_counts(sfm_pair *pair, int32_t *h_counts)
{
    SFM_REQUIRE(pair && h_counts, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kView);
    return copy_out(pair, h_counts, pair->d_vcounts, (size_t)pair->view_hyps * 4);
}

// ---- the pair's points over its registered view (view_points.hip) ---------------------------------
void sfm_view_points_default_params(sfm_view_points_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold_px = 4.0f;
    p->min_score = 0.85f;
    p->max_ambiguity = 0.95f;
    p->min_parallax_deg = 1.0f;
    p->max_iterations = 5;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// the parameter checks of sfm_triangulate_view and sfm_triangulate_views (none needs a device)
static int check_view_points_params(const sfm_view_points_params &p)
{
    const int rc = check_lm_params(p, "sfm_view_points_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(isfinite(p.threshold_px) && p.threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    SFM_REQUIRE(isfinite(p.min_score) && isfinite(p.max_ambiguity), SFM_E_INVALID, "min_score / max_ambiguity must be finite");
    SFM_REQUIRE(p.min_parallax_deg >= 0.0f && p.min_parallax_deg <= 90.0f, SFM_E_INVALID, "min_parallax_deg outside 0..90");
    return SFM_OK;
}

// the inputs a call reads where the caller gave none: the refined points and used flags, the refined pose, the view's refined pose
static ViewPointsInputs view_points_inputs(const sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_view_points_params &p)
{
    ViewPointsInputs in;
    in.sift = d_sift;
    in.points = p.d_points ? p.d_points : pair->d_rpoints;
    in.valid = p.d_points ? p.d_valid : reproj_flags(pair, pair->d_rreproj);
    in.pose2 = p.d_poses ? p.d_poses : pair->d_rstate + refine_pose_offset();
    in.pose3 = p.d_poses ? p.d_poses + 12 : pair->d_vstate + register_pose_offset();
    in.pose_rows = p.d_poses ? 3 : 4;
    return in;
}

int sfm_triangulate_view(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_view_points_params *p, const sfm_view_points_out *out)
{
    SFM_REQUIRE(pair && d_sift && p && out, SFM_E_INVALID, "null argument");
    int rc = check_view_points_params(*p);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p->d_points || !p->d_valid, SFM_E_INVALID, "d_valid needs d_points");
    SFM_REQUIRE(out->d_points && out->d_flags, SFM_E_INVALID, "sfm_view_points_out.d_points and d_flags are required");
    SFM_REQUIRE(out->d_points != p->d_points, SFM_E_INVALID, "the output points must not be the input points");
    SFM_REQUIRE((reinterpret_cast<uintptr_t>(d_sift) & 15) == 0, SFM_E_INVALID, "d_sift must be 16-byte aligned (the records are read with 16-byte loads)");
    SFM_FLUSH(pair);
    SFM_NEED(pair, kPoints | ((p->d_points && p->d_poses) ? 0u : (uint32_t)kRefined) | (p->d_poses ? 0u : (uint32_t)kView));
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    return launch_view_points(pair, view_points_inputs(pair, d_sift, *p), *p, *out);       // reads the pair: no stage changes
}

int sfm_triangulate_views(sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts, const sfm_view_points_params *p,
                          const sfm_view_points_out *outs)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, SFM_E_INVALID, "num_pairs %d outside 0..65535", num_pairs);
    SFM_REQUIRE(!p->d_points && !p->d_valid && !p->d_poses, SFM_E_INVALID,
                "sfm_view_points_params.d_points / d_valid / d_poses must be null here: every pair reads its own refinement and registration");
    int rc = check_view_points_params(*p);
    if (rc != SFM_OK) return rc;
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(pairs && d_sifts && outs, SFM_E_INVALID, "null pair list, d_sifts list or outs list");
    rc = list_entries_present(pairs, num_pairs, "pairs[%d] is null");
    if (rc != SFM_OK) return rc;
    for (int i = 0; i < num_pairs; ++i) {
        SFM_REQUIRE(d_sifts[i], SFM_E_INVALID, "d_sifts[%d] is null", i);
        SFM_REQUIRE((reinterpret_cast<uintptr_t>(d_sifts[i]) & 15) == 0, SFM_E_INVALID, "d_sifts[%d] must be 16-byte aligned", i);
        SFM_REQUIRE(outs[i].d_points && outs[i].d_flags, SFM_E_INVALID, "outs[%d]: d_points and d_flags are required", i);
    }
    sfm_ctx *ctx = pairs[0]->ctx;
    rc = list_one_context_each_once(pairs, num_pairs, ctx, "pairs[%d] belongs to another context than pairs[0]", "pairs", "", "one entry, one set of outputs, per pair");
    if (rc == SFM_OK) rc = list_flush(pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)(kPoints | kRefined | kView); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<ViewPointsInputs> in((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) in[(size_t)i] = view_points_inputs(pairs[i], d_sifts[i], *p);
    return launch_view_points_views(ctx, pairs, num_pairs, in.data(), *p, outs);
}

// ---- cameras 2 and 3 and the points adjusted over the pair's three views (adjust.hip) --------------
void sfm_adjust_default_params(sfm_adjust_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 20;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// the caller's buffers of one (in, out) set: inputs, then outputs.  n: the pair's record count, or 0 where the pair has not been
// looked at yet (bytes_until_known)
constexpr int kAdjustRanges = 10;
static void adjust_ranges(const sfm_adjust_in &in, const sfm_adjust_params &p, const sfm_adjust_out &out, int n, int owner, BufferRange r[kAdjustRanges])
{
    auto len = [n](size_t per_record) { return bytes_until_known(n, per_record); };
    r[0] = { in.d_sift, len(sizeof(sfm_sift_point)), false, owner, "in.d_sift" };
    r[1] = { in.d_points, len(16), false, owner, "in.d_points" }; r[2] = { in.d_flags, len(1), false, owner, "in.d_flags" };
    r[3] = { p.d_used2, len(1), false, owner, "params.d_used2" }; r[4] = { p.d_poses, 24 * sizeof(float), false, owner, "params.d_poses" };
    r[5] = { out.d_poses, 24 * sizeof(float), true, owner, "out.d_poses" }; r[6] = { out.d_points, len(16), true, owner, "out.d_points" };
    r[7] = { out.d_views, len(1), true, owner, "out.d_views" }; r[8] = { out.d_err, len(4), true, owner, "out.d_err" };
    r[9] = { out.d_report, sizeof(sfm_adjust_report), true, owner, "out.d_report" };
}

// The checks of one (in, out) set that need no device: required pointers, the alignment of d_sift, and no output on top of an
// input or of another output (buffer_ranges.hpp).  who: "" or "pairs[i]: ".
static int check_adjust_buffers(const sfm_adjust_in &in, const sfm_adjust_params &p, const sfm_adjust_out &out, int n, const char *who)
{
    SFM_REQUIRE(in.d_sift && in.d_points && in.d_flags, SFM_E_INVALID, "%ssfm_adjust_in.d_sift, d_points and d_flags are required", who);
    SFM_REQUIRE(out.d_poses && out.d_points && out.d_views && out.d_report, SFM_E_INVALID,
                "%ssfm_adjust_out.d_poses, d_points, d_views and d_report are required", who);
    SFM_REQUIRE((reinterpret_cast<uintptr_t>(in.d_sift) & 15) == 0, SFM_E_INVALID,
                "%sd_sift must be 16-byte aligned (the records are read with 16-byte loads)", who);
    BufferRange r[kAdjustRanges];
    adjust_ranges(in, p, out, n, 0, r);
    return check_ranges_in_set(r, kAdjustRanges, who);
}

// the adjustment's work buffer, allocated at the first call and sized to the creation-time count
static int adjust_buffers(sfm_pair *pair)
{
    if (pair->d_awork) return SFM_OK;
    return alloc_group({ { &pair->d_awork, adjust_work_bytes(pair->cap_points) } });
}

// the inputs a call reads where the caller gave none: the refinement's used flags, the refined pose, the view's refined pose
static AdjustInputs adjust_inputs(const sfm_pair *pair, const sfm_adjust_in &in, const sfm_adjust_params &p)
{
    AdjustInputs r;
    r.sift = in.d_sift; r.points = in.d_points; r.flags = in.d_flags;
    r.used2 = p.d_used2 ? p.d_used2 : reproj_flags(pair, pair->d_rreproj);
    r.pose2 = p.d_poses ? p.d_poses : pair->d_rstate + refine_pose_offset();
    r.pose3 = p.d_poses ? p.d_poses + 12 : pair->d_vstate + register_pose_offset();
    r.pose_rows = p.d_poses ? 3 : 4;
    return r;
}

int sfm_adjust_view(sfm_pair *pair, const sfm_adjust_in *in, const sfm_adjust_params *p, const sfm_adjust_out *out)
{
    SFM_REQUIRE(pair && in && p && out, SFM_E_INVALID, "null argument");
    int rc = check_lm_params(*p, "sfm_adjust_params");
    if (rc != SFM_OK) return rc;
    rc = check_adjust_buffers(*in, *p, *out, 0, "");
    if (rc != SFM_OK) return rc;
    SFM_FLUSH(pair);
    SFM_NEED(pair, kPoints | ((p->d_used2 && p->d_poses) ? 0u : (uint32_t)kRefined) | (p->d_poses ? 0u : (uint32_t)kView));
    rc = check_adjust_buffers(*in, *p, *out, pair->n, "");                                  // the same with the arrays' real lengths
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    rc = adjust_buffers(pair);
    if (rc != SFM_OK) return rc;
    return launch_adjust(pair, adjust_inputs(pair, *in, *p), *p, *out);                    // reads the pair: no stage changes
}

int sfm_adjust_views(sfm_pair *const *pairs, int num_pairs, const sfm_adjust_in *ins, const sfm_adjust_params *p, const sfm_adjust_out *outs)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, SFM_E_INVALID, "num_pairs %d outside 0..65535", num_pairs);
    SFM_REQUIRE(!p->d_used2 && !p->d_poses, SFM_E_INVALID,
                "sfm_adjust_params.d_used2 / d_poses must be null here: every pair reads its own refinement and registration");
    int rc = check_lm_params(*p, "sfm_adjust_params");
    if (rc != SFM_OK) return rc;
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(pairs && ins && outs, SFM_E_INVALID, "null pair list, ins list or outs list");
    rc = list_entries_present(pairs, num_pairs, "pairs[%d] is null");
    if (rc != SFM_OK) return rc;
    char who[32];
    for (int i = 0; i < num_pairs; ++i) {
        snprintf(who, sizeof(who), "pairs[%d]: ", i);
        rc = check_adjust_buffers(ins[i], *p, outs[i], 0, who);
        if (rc != SFM_OK) return rc;
    }
    sfm_ctx *ctx = pairs[0]->ctx;
    rc = list_one_context_each_once(pairs, num_pairs, ctx, "pairs[%d] belongs to another context than pairs[0]", "pairs", "", "two blocks would write the same work buffer");
    if (rc == SFM_OK) rc = list_flush(pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)(kPoints | kRefined | kView); });
    if (rc == SFM_OK) rc = check_ranges_of_entries(num_pairs, kAdjustRanges, "pairs", [&](int i, BufferRange *r) { adjust_ranges(ins[i], *p, outs[i], pairs[i]->n, i, r); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 0; i < num_pairs; ++i) { rc = adjust_buffers(pairs[i]); if (rc != SFM_OK) return rc; }
    std::vector<AdjustInputs> in((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) in[(size_t)i] = adjust_inputs(pairs[i], ins[i], *p);
    return launch_adjust_views(ctx, pairs, num_pairs, in.data(), *p, outs);
}

// ---- the similarity between two overlapping pairs' frames (align.hip) ------------------------------
void sfm_align_default_params(sfm_align_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->num_hypotheses = 4096;
    p->seed = 0x5EED5F3Du;
    p->threshold_px = 4.0f;
    p->max_iterations = 10;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// the parameter checks of sfm_align_pair and sfm_align_pairs (none needs a device)
static int check_align_params(const sfm_align_params &p)
{
    const int rc = check_lm_params(p, "sfm_align_params");
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p.num_hypotheses >= 1 && p.num_hypotheses <= (1u << 20), SFM_E_INVALID, "num_hypotheses %u outside 1..2^20", p.num_hypotheses);
    SFM_REQUIRE(isfinite(p.threshold_px) && p.threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    SFM_REQUIRE(p.d_points_a || !p.d_valid_a, SFM_E_INVALID, "d_valid_a needs d_points_a");
    SFM_REQUIRE(p.d_points_b || !p.d_valid_b, SFM_E_INVALID, "d_valid_b needs d_points_b");
    return SFM_OK;
}

// the caller's buffers of one link: inputs, then outputs.  na, nb: the pairs' record counts, or 0 where the pairs have not been
// looked at yet (bytes_until_known)
constexpr int kAlignRanges = 10;
static void align_ranges(const int32_t *d_index, const sfm_align_params &p, const sfm_align_out &out, int na, int nb, int owner, BufferRange r[kAlignRanges])
{
    r[0] = { d_index, bytes_until_known(na, 4), false, owner, "d_index" };
    r[1] = { p.d_points_a, bytes_until_known(na, 16), false, owner, "params.d_points_a" }; r[2] = { p.d_valid_a, bytes_until_known(na, 1), false, owner, "params.d_valid_a" };
    r[3] = { p.d_points_b, bytes_until_known(nb, 16), false, owner, "params.d_points_b" }; r[4] = { p.d_valid_b, bytes_until_known(nb, 1), false, owner, "params.d_valid_b" };
    r[5] = { out.d_sim, 26 * sizeof(float), true, owner, "out.d_sim" }; r[6] = { out.d_inlier, bytes_until_known(na, 1), true, owner, "out.d_inlier" };
    r[7] = { out.d_err, bytes_until_known(na, 4), true, owner, "out.d_err" }; r[8] = { out.d_counts, (size_t)p.num_hypotheses * 4, true, owner, "out.d_counts" };
    r[9] = { out.d_report, sizeof(sfm_align_report), true, owner, "out.d_report" };
}

// The checks of one link's buffers that need no device: required pointers, no output on top of an input or of another output
// (buffer_ranges.hpp).  who: "" or "links[i]: ".
static int check_align_buffers(const int32_t *d_index, const sfm_align_params &p, const sfm_align_out &out, int na, int nb, const char *who)
{
    SFM_REQUIRE(d_index, SFM_E_INVALID, "%sd_index is required", who);
    SFM_REQUIRE(out.d_sim && out.d_inlier && out.d_report, SFM_E_INVALID, "%ssfm_align_out.d_sim, d_inlier and d_report are required", who);
    BufferRange r[kAlignRanges];
    align_ranges(d_index, p, out, na, nb, 0, r);
    return check_ranges_in_set(r, kAlignRanges, who);
}

// the work buffers of pair `a`: the per-record one allocated at the first call, the per-hypothesis one grown on demand
static int align_buffers(sfm_pair *pair, uint32_t num_hypotheses)
{
    int rc = SFM_OK;
    if (!pair->d_lwork) {                               // sized to the creation-time count: sfm_pair_reset needs no reallocation
        rc = alloc_group({ { &pair->d_lwork, align_work_bytes(pair->cap_points) } });
        if (rc != SFM_OK) return rc;
    }
    if (num_hypotheses > pair->cap_lhyps) {             // grows with the largest num_hypotheses seen (the old buffer may be in use)
        pair->cap_lhyps = 0;
        size_t have = 0;
        rc = grow(&pair->d_lhyp, &have, align_hyp_bytes(num_hypotheses), pair->ctx->stream);
        if (rc == SFM_OK) pair->cap_lhyps = num_hypotheses;
    }
    return rc;
}

// the inputs a call reads where the caller gave none: each pair's refined points and the refinement's used flags
static AlignInputs align_inputs(const sfm_pair *a, const sfm_pair *b, const int32_t *d_index, const sfm_align_params &p)
{
    AlignInputs in;
    in.points_a = p.d_points_a ? p.d_points_a : a->d_rpoints;
    in.valid_a = p.d_points_a ? p.d_valid_a : reproj_flags(a, a->d_rreproj);
    in.points_b = p.d_points_b ? p.d_points_b : b->d_rpoints;
    in.valid_b = p.d_points_b ? p.d_valid_b : reproj_flags(b, b->d_rreproj);
    in.index = d_index;
    return in;
}

int sfm_align_index_from_matches(sfm_ctx *ctx, const sfm_sift_point *d_sift, int n, float min_score, float max_ambiguity, int32_t *d_index)
{
    SFM_REQUIRE(ctx && d_sift && d_index, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(n >= 0, SFM_E_INVALID, "n %d is negative", n);
    SFM_REQUIRE(isfinite(min_score) && isfinite(max_ambiguity), SFM_E_INVALID, "min_score / max_ambiguity must be finite");
    if (n == 0) return SFM_OK;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    return launch_align_index(ctx, d_sift, n, min_score, max_ambiguity, d_index);
}

int sfm_align_pair(sfm_pair *a, sfm_pair *b, const int32_t *d_index, const sfm_align_params *p, const sfm_align_out *out)
{
    SFM_REQUIRE(a && b && p && out, SFM_E_INVALID, "null argument");
    int rc = check_align_params(*p);
    if (rc != SFM_OK) return rc;
    rc = check_align_buffers(d_index, *p, *out, 0, 0, "");
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(a != b, SFM_E_INVALID, "a and b are the same pair");
    SFM_REQUIRE(a->ctx == b->ctx, SFM_E_INVALID, "a and b belong to different contexts");
    SFM_FLUSH(a);
    SFM_FLUSH(b);
    SFM_NEED(a, p->d_points_a ? kPoints : kPoints | kRefined);
    SFM_NEED(b, p->d_points_b ? kPoints : kPoints | kRefined);
    rc = check_align_buffers(d_index, *p, *out, a->n, b->n, "");                            // the same with the arrays' real lengths
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(a->ctx->device));
    rc = align_buffers(a, p->num_hypotheses);
    if (rc != SFM_OK) return rc;
    return launch_align(a, b, align_inputs(a, b, d_index, *p), *p, *out);                  // reads the pairs: no stage changes
}

int sfm_align_pairs(sfm_pair *const *as, sfm_pair *const *bs, int num_links, const int32_t *const *d_indices, const sfm_align_params *p,
                    const sfm_align_out *outs)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_links >= 0 && num_links <= 65535, SFM_E_INVALID, "num_links %d outside 0..65535", num_links);
    SFM_REQUIRE(!p->d_points_a && !p->d_valid_a && !p->d_points_b && !p->d_valid_b, SFM_E_INVALID,
                "sfm_align_params.d_points_* / d_valid_* must be null here: every pair reads its own refinement");
    int rc = check_align_params(*p);
    if (rc != SFM_OK) return rc;
    if (num_links == 0) return SFM_OK;
    SFM_REQUIRE(as && bs && d_indices && outs, SFM_E_INVALID, "null pair list, d_indices list or outs list");
    rc = list_entries_present(as, num_links, "links[%d]: null pair");
    if (rc == SFM_OK) rc = list_entries_present(bs, num_links, "links[%d]: null pair");
    if (rc != SFM_OK) return rc;
    char who[32];
    for (int i = 0; i < num_links; ++i) {
        SFM_REQUIRE(as[i] != bs[i], SFM_E_INVALID, "links[%d]: a and b are the same pair", i);
        snprintf(who, sizeof(who), "links[%d]: ", i);
        rc = check_align_buffers(d_indices[i], *p, outs[i], 0, 0, who);
        if (rc != SFM_OK) return rc;
    }
    sfm_ctx *ctx = as[0]->ctx;
    const char *other_ctx = "links[%d]: a pair belongs to another context than links[0]'s a";
    const auto need = [](int) { return (uint32_t)(kPoints | kRefined); };
    rc = list_one_context_each_once(as, num_links, ctx, other_ctx, "links", " as a", "two blocks would write the same work buffer");
    if (rc == SFM_OK) rc = list_one_context_each_once(bs, num_links, ctx, other_ctx, "links", "", nullptr);       // b is only read: as often as the caller likes
    if (rc == SFM_OK) rc = list_flush(as, num_links);
    if (rc == SFM_OK) rc = list_flush(bs, num_links);
    if (rc == SFM_OK) rc = list_stages(as, num_links, "links", "a: ", need);
    if (rc == SFM_OK) rc = list_stages(bs, num_links, "links", "b: ", need);
    if (rc == SFM_OK) rc = check_ranges_of_entries(num_links, kAlignRanges, "links",
                                                   [&](int i, BufferRange *r) { align_ranges(d_indices[i], *p, outs[i], as[i]->n, bs[i]->n, i, r); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 0; i < num_links; ++i) { rc = align_buffers(as[i], p->num_hypotheses); if (rc != SFM_OK) return rc; }
    std::vector<AlignInputs> in((size_t)num_links);
    for (int i = 0; i < num_links; ++i) in[(size_t)i] = align_inputs(as[i], bs[i], d_indices[i], *p);
    return launch_align_pairs(ctx, as, bs, num_links, in.data(), *p, outs);
}

// ---- a chain of aligned pairs fused into tracks and one point per track (fuse.hip) -----------------
void sfm_fuse_default_params(sfm_fuse_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold_px = 4.0f;
    p->max_iterations = 5;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
}

// What sfm_fuse_chain and sfm_fuse_ring share behind their argument checks, in two steps that each call keeps in its own order
// around its link checks.  fuse_check_pairs: every pair present, of this context and listed once (`visits`: the text for a pair
// listed twice), d_valid only with d_points, at most 2^26 records; handles and total are filled.
static int fuse_check_pairs(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const char *visits, std::vector<sfm_pair *> &handles,
                            long long &total)
{
    handles.resize((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) handles[(size_t)i] = pairs[i].pair;
    int rc = list_entries_present(handles.data(), num_pairs, "pairs[%d]: null pair");
    if (rc == SFM_OK) rc = list_one_context_each_once(handles.data(), num_pairs, ctx, "pairs[%d]: the pair belongs to another context", "pairs", "",
                                                      visits);
    if (rc != SFM_OK) return rc;
    total = 0;
    for (int i = 0; i < num_pairs; ++i) {
        SFM_REQUIRE(pairs[i].d_points || !pairs[i].d_valid, SFM_E_INVALID, "pairs[%d]: d_valid needs d_points", i);
        total += pairs[i].pair->n;
    }
    SFM_REQUIRE(total <= (1ll << 26), SFM_E_INVALID, "%lld records in all: more than 2^26", total);
    return SFM_OK;
}

// fuse_ready: no output on an input or on another output (num_links links: the chain's k - 1 or the ring's k; d_report: the ring's
// further output, or null), the pairs flushed and their stages there, the device set, and the FusePair of every pair with link i in
// pair i.  Every range is its own owner (its place in `entry`, which keeps the index its name takes): nothing is exempt, so the
// sweep is the whole check.
static int fuse_ready(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const sfm_fuse_link_in *links, int num_links,
                      const sfm_fuse_out *out, const sfm_fuse_ring_report *d_report, std::vector<sfm_pair *> &handles, long long total,
                      std::vector<FusePair> &fp)
{
    {
        std::vector<BufferRange> r;
        std::vector<int> entry;
        r.reserve((size_t)num_pairs * 8 + 12);
        entry.reserve((size_t)num_pairs * 8 + 12);
        auto add = [&](const void *ptr, size_t bytes, bool is_out, int who, const char *name) {
            r.push_back({ ptr, bytes, is_out, (int)entry.size(), name });
            entry.push_back(who);
        };
        const size_t N = (size_t)total, k = (size_t)num_pairs;
        for (int i = 0; i < num_pairs; ++i) {
            const size_t n = (size_t)pairs[i].pair->n;
            add(pairs[i].d_points, n * 16, false, i, "pairs[%d].d_points"); add(pairs[i].d_valid, n, false, i, "pairs[%d].d_valid");
            add(pairs[i].d_pose, 48, false, i, "pairs[%d].d_pose");
            if (i < num_links) {
                add(links[i].d_index, n * 4, false, i, "links[%d].d_index"); add(links[i].d_sim, 52, false, i, "links[%d].d_sim");
                add(links[i].d_inlier, n, false, i, "links[%d].d_inlier"); add(links[i].d_err, n * 4, false, i, "links[%d].d_err");
                add(links[i].d_report, sizeof(sfm_align_report), false, i, "links[%d].d_report");
            }
        }
        add(out->d_frames, k * 52, true, -1, "out.d_frames"); add(out->d_root, k * 4, true, -1, "out.d_root");
        add(out->d_cams, k * 96, true, -1, "out.d_cams"); add(out->d_track, N * 4, true, -1, "out.d_track");
        add(out->d_track_offset, (N + 1) * 4, true, -1, "out.d_track_offset"); add(out->d_obs_cam, N * 8, true, -1, "out.d_obs_cam");
        add(out->d_obs_record, N * 8, true, -1, "out.d_obs_record"); add(out->d_points, N * 16, true, -1, "out.d_points");
        add(out->d_flags, N, true, -1, "out.d_flags"); add(out->d_err, N * 4, true, -1, "out.d_err");
        add(out->d_counts, 32, true, -1, "out.d_counts"); add(d_report, sizeof(sfm_fuse_ring_report), true, -1, "d_report");
        if (const RangeConflict c = first_conflict_across_owners(r)) {
            char a[48], b[48];
            snprintf(a, sizeof(a), c.a->name, entry[(size_t)c.a->owner]); snprintf(b, sizeof(b), c.b->name, entry[(size_t)c.b->owner]);
            SFM_REQUIRE(false, SFM_E_INVALID, "%s overlaps %s", c.a->out ? a : b, c.a->out ? b : a);       // the output first
        }
    }
    int rc = list_flush(handles.data(), num_pairs);
    if (rc == SFM_OK) rc = list_stages(handles.data(), num_pairs, "pairs", "",
                                       [&](int i) { return (uint32_t)((pairs[i].d_points && pairs[i].d_pose) ? kPoints : kPoints | kRefined); });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    fp.resize((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const sfm_pair *pr = pairs[i].pair;
        FusePair &f = fp[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.points = pairs[i].d_points ? pairs[i].d_points : pr->d_rpoints;
        f.valid = pairs[i].d_points ? pairs[i].d_valid : reproj_flags(pr, pr->d_rreproj);
        f.X0 = pr->d_X[0]; f.X1 = pr->d_X[1]; f.K = pr->d_K;
        f.pose = pairs[i].d_pose ? pairs[i].d_pose : pr->d_rstate + refine_pose_offset();
        f.pose_rows = pairs[i].d_pose ? 3 : 4;
        f.n = pr->n; f.ld = pr->ld;
        if (i < num_links) {
            f.index = links[i].d_index; f.sim = links[i].d_sim; f.inlier = links[i].d_inlier; f.err = links[i].d_err; f.report = links[i].d_report;
        }
    }
    return SFM_OK;
}

// every field of links 0 .. num_links - 1 is there
static int fuse_links_complete(const sfm_fuse_link_in *links, int num_links)
{
    for (int i = 0; i < num_links; ++i)
        SFM_REQUIRE(links[i].d_index && links[i].d_sim && links[i].d_inlier && links[i].d_err && links[i].d_report, SFM_E_INVALID,
                    "links[%d]: d_index, d_sim, d_inlier, d_err and d_report are required", i);
    return SFM_OK;
}

static int fuse_out_required(const sfm_fuse_out *out)
{
    SFM_REQUIRE(out->d_frames && out->d_root && out->d_cams && out->d_track && out->d_track_offset && out->d_obs_cam && out->d_obs_record &&
                out->d_points && out->d_flags && out->d_counts, SFM_E_INVALID, "every buffer of sfm_fuse_out but d_err is required");
    return SFM_OK;
}

int sfm_fuse_chain(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const sfm_fuse_link_in *links, const sfm_fuse_params *p,
                   const sfm_fuse_out *out)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 4096, SFM_E_INVALID, "num_pairs %d outside 0..4096", num_pairs);
    int rc = check_lm_params(*p, "sfm_fuse_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(isfinite(p->threshold_px) && p->threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(ctx && pairs && out, SFM_E_INVALID, "null context, pair list or out");
    SFM_REQUIRE(links || num_pairs == 1, SFM_E_INVALID, "null link list");
    rc = fuse_out_required(out);
    if (rc != SFM_OK) return rc;
    std::vector<sfm_pair *> handles;
    std::vector<FusePair> fp;
    long long total = 0;
    rc = fuse_check_pairs(ctx, pairs, num_pairs, "a chain visits a pair once", handles, total);
    if (rc == SFM_OK) rc = fuse_links_complete(links, num_pairs - 1);
    if (rc == SFM_OK) rc = fuse_ready(ctx, pairs, num_pairs, links, num_pairs - 1, out, nullptr, handles, total, fp);
    if (rc != SFM_OK) return rc;
    return launch_fuse_chain(ctx, fp.data(), num_pairs, *p, *out);                           // reads the pairs: no stage changes
}

// ---- the same fusion over a closed ring, the seam joined (fuse_ring.hip) ---------------------------
void sfm_fuse_ring_default_params(sfm_fuse_ring_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    sfm_fuse_default_params(&p->fuse);
    p->max_closure_rotation_rad = 1e-3f;
    p->max_closure_log_scale = 1e-3f;
}

int sfm_fuse_ring(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const sfm_fuse_link_in *links, const sfm_fuse_ring_params *p,
                  const sfm_fuse_out *out, sfm_fuse_ring_report *d_report)
{
    // sfm_fuse_chain's contract: the checks that need no device first (here all k links before the pairs), all of them before
    // anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 3 && num_pairs <= 4096, SFM_E_INVALID, "num_pairs %d outside 3..4096", num_pairs);
    SFM_REQUIRE(ctx && pairs && links && out && d_report, SFM_E_INVALID, "null context, pair list, link list, out or d_report");
    int rc = fuse_out_required(out);
    if (rc == SFM_OK) rc = fuse_links_complete(links, num_pairs);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0 && p->reserved[3] == 0, SFM_E_INVALID,
                "sfm_fuse_ring_params.reserved[] must be zero");
    SFM_REQUIRE(p->max_closure_rotation_rad > 0.0f && p->max_closure_rotation_rad <= 1.57079637f, SFM_E_INVALID,
                "max_closure_rotation_rad must lie in (0, pi/2]");
    SFM_REQUIRE(isfinite(p->max_closure_log_scale) && p->max_closure_log_scale > 0.0f, SFM_E_INVALID,
                "max_closure_log_scale must be finite and > 0");
    rc = check_lm_params(p->fuse, "sfm_fuse_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(isfinite(p->fuse.threshold_px) && p->fuse.threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    std::vector<sfm_pair *> handles;
    std::vector<FusePair> fp;
    long long total = 0;
    rc = fuse_check_pairs(ctx, pairs, num_pairs, "a ring visits a pair once", handles, total);
    if (rc == SFM_OK) rc = fuse_ready(ctx, pairs, num_pairs, links, num_pairs, out, d_report, handles, total, fp);
    if (rc != SFM_OK) return rc;
    return launch_fuse_ring(ctx, fp.data(), num_pairs, *p, *out, d_report);                  // reads the pairs: no stage changes
}

// ---- one bundle adjustment over a fused chain (chain_adjust.hip) -----------------------------------
void sfm_adjust_chain_default_params(sfm_adjust_chain_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 10;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
    p->max_track_views = 8;
}

int sfm_adjust_chain(sfm_ctx *ctx, const sfm_adjust_chain_in *in, int num_pairs, const sfm_adjust_chain_params *p, const sfm_adjust_chain_out *out)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 4096, SFM_E_INVALID, "num_pairs %d outside 0..4096", num_pairs);
    int rc = check_lm_params(*p, "sfm_adjust_chain_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p->max_track_views >= 2 && p->max_track_views <= kChainMaxViews, SFM_E_INVALID, "max_track_views %d outside 2..%d",
                p->max_track_views, kChainMaxViews);
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(ctx && in && out, SFM_E_INVALID, "null context, in or out");
    SFM_REQUIRE(in->pairs && in->d_root && in->d_cams && in->d_track_offset && in->d_obs_cam && in->d_obs_record && in->d_points && in->d_flags &&
                in->d_counts, SFM_E_INVALID, "every field of sfm_adjust_chain_in is required");
    SFM_REQUIRE(out->d_cams && out->d_points && out->d_used && out->d_reports, SFM_E_INVALID, "every buffer of sfm_adjust_chain_out but d_err is required");
    rc = list_entries_present(in->pairs, num_pairs, "pairs[%d]: null pair");
    if (rc == SFM_OK) rc = list_one_context_each_once(in->pairs, num_pairs, ctx, "pairs[%d]: the pair belongs to another context", "pairs", "",
                                                      "a chain visits a pair once");
    if (rc != SFM_OK) return rc;
    long long total = 0;
    for (int i = 0; i < num_pairs; ++i) total += in->pairs[i]->n;
    SFM_REQUIRE(total <= (1ll << 26), SFM_E_INVALID, "%lld records in all: more than 2^26", total);
    {
        // no output on an input or on another output: every range its own owner, so the sweep is the whole check
        const size_t N = (size_t)total, k = (size_t)num_pairs;
        std::vector<BufferRange> r = {
            { in->d_root, k * 4, false, 0, "in.d_root" }, { in->d_cams, k * 96, false, 1, "in.d_cams" },
            { in->d_track_offset, (N + 1) * 4, false, 2, "in.d_track_offset" }, { in->d_obs_cam, N * 8, false, 3, "in.d_obs_cam" },
            { in->d_obs_record, N * 8, false, 4, "in.d_obs_record" }, { in->d_points, N * 16, false, 5, "in.d_points" },
            { in->d_flags, N, false, 6, "in.d_flags" }, { in->d_counts, 32, false, 7, "in.d_counts" },
            { out->d_cams, k * 96, true, 8, "out.d_cams" }, { out->d_points, N * 16, true, 9, "out.d_points" },
            { out->d_used, N, true, 10, "out.d_used" }, { out->d_err, N * 4, true, 11, "out.d_err" },
            { out->d_reports, k * sizeof(sfm_adjust_chain_report), true, 12, "out.d_reports" } };
        if (const RangeConflict c = first_conflict_across_owners(r))
            SFM_REQUIRE(false, SFM_E_INVALID, "%s overlaps %s", c.a->out ? c.a->name : c.b->name, c.a->out ? c.b->name : c.a->name);      // the output first
    }
    rc = list_flush(in->pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(in->pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)kPoints; });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<FusePair> fp((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const sfm_pair *pr = in->pairs[i];
        FusePair &f = fp[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = pr->d_X[0]; f.X1 = pr->d_X[1]; f.K = pr->d_K;                    // what fuse_view reads
        f.n = pr->n; f.ld = pr->ld;
    }
    return launch_adjust_chain(ctx, fp.data(), num_pairs, *in, *p, *out);       // reads the pairs: no stage changes
}

// ---- one bundle adjustment over a closed ring (ring_adjust.hip) -------------------------------------
void sfm_adjust_ring_default_params(sfm_adjust_ring_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 10;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
    p->max_track_views = 8;
}

int sfm_adjust_ring(sfm_ctx *ctx, const sfm_adjust_ring_in *in, int num_pairs, const sfm_adjust_ring_params *p, const sfm_adjust_ring_out *out)
{
    // sfm_adjust_chain's contract in its order: the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 3 && num_pairs <= 4096, SFM_E_INVALID, "num_pairs %d outside 3..4096", num_pairs);
    int rc = check_lm_params(*p, "sfm_adjust_ring_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(p->max_track_views >= 2 && p->max_track_views <= kChainMaxViews, SFM_E_INVALID, "max_track_views %d outside 2..%d",
                p->max_track_views, kChainMaxViews);
    SFM_REQUIRE(ctx && in && out, SFM_E_INVALID, "null context, in or out");
    SFM_REQUIRE(in->pairs && in->d_root && in->d_cams && in->d_track_offset && in->d_obs_cam && in->d_obs_record && in->d_points && in->d_flags &&
                in->d_counts && in->d_ring_report, SFM_E_INVALID, "every field of sfm_adjust_ring_in is required");
    SFM_REQUIRE(out->d_cams && out->d_points && out->d_used && out->d_report, SFM_E_INVALID, "every buffer of sfm_adjust_ring_out but d_err is required");
    rc = list_entries_present(in->pairs, num_pairs, "pairs[%d]: null pair");
    if (rc == SFM_OK) rc = list_one_context_each_once(in->pairs, num_pairs, ctx, "pairs[%d]: the pair belongs to another context", "pairs", "",
                                                      "a ring visits a pair once");
    if (rc != SFM_OK) return rc;
    long long total = 0;
    for (int i = 0; i < num_pairs; ++i) total += in->pairs[i]->n;
    SFM_REQUIRE(total <= (1ll << 26), SFM_E_INVALID, "%lld records in all: more than 2^26", total);
    {
        // no output on an input or on another output: every range its own owner, so the sweep is the whole check
        const size_t N = (size_t)total, k = (size_t)num_pairs;
        std::vector<BufferRange> r = {
            { in->d_root, k * 4, false, 0, "in.d_root" }, { in->d_cams, k * 96, false, 1, "in.d_cams" },
            { in->d_track_offset, (N + 1) * 4, false, 2, "in.d_track_offset" }, { in->d_obs_cam, N * 8, false, 3, "in.d_obs_cam" },
            { in->d_obs_record, N * 8, false, 4, "in.d_obs_record" }, { in->d_points, N * 16, false, 5, "in.d_points" },
            { in->d_flags, N, false, 6, "in.d_flags" }, { in->d_counts, 32, false, 7, "in.d_counts" },
            { in->d_ring_report, sizeof(sfm_fuse_ring_report), false, 8, "in.d_ring_report" },
            { out->d_cams, k * 96, true, 9, "out.d_cams" }, { out->d_points, N * 16, true, 10, "out.d_points" },
            { out->d_used, N, true, 11, "out.d_used" }, { out->d_err, N * 4, true, 12, "out.d_err" },
            { out->d_report, sizeof(sfm_adjust_ring_report), true, 13, "out.d_report" } };
        if (const RangeConflict c = first_conflict_across_owners(r))
            SFM_REQUIRE(false, SFM_E_INVALID, "%s overlaps %s", c.a->out ? c.a->name : c.b->name, c.a->out ? c.b->name : c.a->name);      // the output first
    }
    rc = list_flush(in->pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(in->pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)kPoints; });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<FusePair> fp((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const sfm_pair *pr = in->pairs[i];
        FusePair &f = fp[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = pr->d_X[0]; f.X1 = pr->d_X[1]; f.K = pr->d_K;                    // what fuse_view reads
        f.n = pr->n; f.ld = pr->ld;
    }
    return launch_adjust_ring(ctx, fp.data(), num_pairs, *in, *p, *out);        // reads the pairs: no stage changes
}

// ---- every track of a fused table intersected under a given camera table (intersect.hip) -----------
void sfm_intersect_default_params(sfm_intersect_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold_px = 4.0f;
    p->max_iterations = 5;
    p->huber_px = 1.0f;
    p->min_rel_decrease = 1e-6f;
    p->initial_lambda = 1e-3f;
    p->wave_min_views = 0;                                // the library's default (intersect_math.hpp)
}

int sfm_intersect_tracks(sfm_ctx *ctx, const sfm_intersect_in *in, int num_pairs, const sfm_intersect_params *p, const sfm_intersect_out *out)
{
    // sfm_adjust_chain's contract in its order: the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_pairs >= 0 && num_pairs <= 4096, SFM_E_INVALID, "num_pairs %d outside 0..4096", num_pairs);
    int rc = check_lm_params(*p, "sfm_intersect_params", 50);
    if (rc != SFM_OK) return rc;
    SFM_REQUIRE(isfinite(p->threshold_px) && p->threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    SFM_REQUIRE(p->wave_min_views == 0 || p->wave_min_views >= 2, SFM_E_INVALID, "wave_min_views %d is neither 0 nor at least 2", p->wave_min_views);
    if (num_pairs == 0) return SFM_OK;
    SFM_REQUIRE(ctx && in && out, SFM_E_INVALID, "null context, in or out");
    SFM_REQUIRE(in->pairs && in->d_cams && in->d_track_offset && in->d_obs_cam && in->d_obs_record && in->d_points && in->d_flags && in->d_counts,
                SFM_E_INVALID, "every field of sfm_intersect_in but d_skip is required");
    SFM_REQUIRE(out->d_points && out->d_flags && out->d_counts, SFM_E_INVALID, "every buffer of sfm_intersect_out but d_err is required");
    rc = list_entries_present(in->pairs, num_pairs, "pairs[%d]: null pair");
    if (rc == SFM_OK) rc = list_one_context_each_once(in->pairs, num_pairs, ctx, "pairs[%d]: the pair belongs to another context", "pairs", "",
                                                      "a table holds a pair once");
    if (rc != SFM_OK) return rc;
    long long total = 0;
    for (int i = 0; i < num_pairs; ++i) total += in->pairs[i]->n;
    SFM_REQUIRE(total <= (1ll << 26), SFM_E_INVALID, "%lld records in all: more than 2^26", total);
    {
        // no output on an input or on another output: every range its own owner, so the sweep is the whole check
        const size_t N = (size_t)total, k = (size_t)num_pairs;
        std::vector<BufferRange> r = {
            { in->d_cams, k * 96, false, 0, "in.d_cams" }, { in->d_track_offset, (N + 1) * 4, false, 1, "in.d_track_offset" },
            { in->d_obs_cam, N * 8, false, 2, "in.d_obs_cam" }, { in->d_obs_record, N * 8, false, 3, "in.d_obs_record" },
            { in->d_points, N * 16, false, 4, "in.d_points" }, { in->d_flags, N, false, 5, "in.d_flags" },
            { in->d_counts, 32, false, 6, "in.d_counts" }, { in->d_skip, N, false, 7, "in.d_skip" },
            { out->d_points, N * 16, true, 8, "out.d_points" }, { out->d_flags, N, true, 9, "out.d_flags" },
            { out->d_err, N * 4, true, 10, "out.d_err" }, { out->d_counts, 32, true, 11, "out.d_counts" } };
        if (const RangeConflict c = first_conflict_across_owners(r))
            SFM_REQUIRE(false, SFM_E_INVALID, "%s overlaps %s", c.a->out ? c.a->name : c.b->name, c.a->out ? c.b->name : c.a->name);      // the output first
    }
    rc = list_flush(in->pairs, num_pairs);
    if (rc == SFM_OK) rc = list_stages(in->pairs, num_pairs, "pairs", "", [](int) { return (uint32_t)kPoints; });
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<FusePair> fp((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const sfm_pair *pr = in->pairs[i];
        FusePair &f = fp[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = pr->d_X[0]; f.X1 = pr->d_X[1]; f.K = pr->d_K;                    // what fuse_view reads
        f.n = pr->n; f.ld = pr->ld;
    }
    return launch_intersect_tracks(ctx, fp.data(), num_pairs, *in, *p, *out);   // reads the pairs: no stage changes
}

// ---- a ring of aligned pairs closed: the drift spread over the links (ring.hip) -------------------
void sfm_ring_default_params(sfm_ring_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold_px = 4.0f;
    p->max_rotation_rad = 0.35f;
    p->max_log_scale = 0.693147182f;                      // ln 2
}

int sfm_close_ring(sfm_ctx *ctx, const sfm_ring_link_in *links, int num_links, const sfm_fuse_pair_in *last_pair, const sfm_ring_params *p,
                   const sfm_ring_out *out)
{
    // the checks that need no device first, all of them before anything is enqueued
    SFM_REQUIRE(p, SFM_E_INVALID, "null params");
    SFM_REQUIRE(num_links >= 3 && num_links <= 4096, SFM_E_INVALID, "num_links %d outside 3..4096", num_links);
    SFM_REQUIRE(ctx && links && last_pair && out, SFM_E_INVALID, "null context, link list, last_pair or out");
    for (int i = 0; i < num_links; ++i)
        SFM_REQUIRE(links[i].d_sim && links[i].d_report, SFM_E_INVALID, "links[%d]: d_sim and d_report are required", i);
    SFM_REQUIRE(last_pair->pair, SFM_E_INVALID, "last_pair: null pair");
    SFM_REQUIRE(last_pair->d_points || !last_pair->d_valid, SFM_E_INVALID, "last_pair: d_valid needs d_points");
    SFM_REQUIRE(out->d_links && out->d_frames && out->d_report, SFM_E_INVALID, "every buffer of sfm_ring_out but d_seam_err is required");
    SFM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0 && p->reserved[3] == 0, SFM_E_INVALID,
                "sfm_ring_params.reserved[] must be zero");
    SFM_REQUIRE(p->max_rotation_rad > 0.0f && p->max_rotation_rad <= 1.57079637f, SFM_E_INVALID, "max_rotation_rad must lie in (0, pi/2]");
    SFM_REQUIRE(isfinite(p->max_log_scale) && p->max_log_scale > 0.0f, SFM_E_INVALID, "max_log_scale must be finite and > 0");
    SFM_REQUIRE(isfinite(p->threshold_px) && p->threshold_px > 0.0f, SFM_E_INVALID, "threshold_px must be finite and > 0");
    if (p->weights) {
        double sum = 0.0;
        for (int i = 0; i < num_links; ++i) {
            SFM_REQUIRE(isfinite(p->weights[i]) && p->weights[i] >= 0.0f, SFM_E_INVALID, "links[%d]: its weight must be finite and >= 0", i);
            sum += (double)p->weights[i];
        }
        SFM_REQUIRE(sum > 0.0, SFM_E_INVALID, "the weights must have a positive sum");
    }
    sfm_pair *pr = last_pair->pair;
    SFM_REQUIRE(pr->ctx == ctx, SFM_E_INVALID, "last_pair: the pair belongs to another context");
    {
        // no output on an input or on another output: every range its own owner, so the sweep is the whole check
        std::vector<BufferRange> r;
        std::vector<int> entry;
        r.reserve((size_t)num_links * 2 + 6);
        entry.reserve((size_t)num_links * 2 + 6);
        auto add = [&](const void *ptr, size_t bytes, bool is_out, int who, const char *name) {
            r.push_back({ ptr, bytes, is_out, (int)entry.size(), name });
            entry.push_back(who);
        };
        const size_t n = (size_t)pr->n, k = (size_t)num_links;
        for (int i = 0; i < num_links; ++i) {
            add(links[i].d_sim, 52, false, i, "links[%d].d_sim");
            add(links[i].d_report, sizeof(sfm_align_report), false, i, "links[%d].d_report");
        }
        add(last_pair->d_points, n * 16, false, -1, "last_pair.d_points"); add(last_pair->d_valid, n, false, -1, "last_pair.d_valid");
        add(out->d_links, k * 52, true, -1, "out.d_links"); add(out->d_frames, k * 52, true, -1, "out.d_frames");
        add(out->d_seam_err, n * 12, true, -1, "out.d_seam_err"); add(out->d_report, sizeof(sfm_ring_report), true, -1, "out.d_report");
        if (const RangeConflict c = first_conflict_across_owners(r)) {
            char a[48], b[48];
            snprintf(a, sizeof(a), c.a->name, entry[(size_t)c.a->owner]); snprintf(b, sizeof(b), c.b->name, entry[(size_t)c.b->owner]);
            SFM_REQUIRE(false, SFM_E_INVALID, "%s overlaps %s", c.a->out ? a : b, c.a->out ? b : a);       // the output first
        }
    }
    SFM_FLUSH(pr);
    const uint32_t stages = last_pair->d_points ? kPoints : kPoints | kRefined;
    SFM_REQUIRE(pr->state.has(stages), SFM_E_STATE, "last_pair: %s", pair_stage_hint(pr->state.missing(stages)));
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    std::vector<RingLink> rl((size_t)num_links);
    for (int i = 0; i < num_links; ++i) rl[(size_t)i] = { links[i].d_sim, links[i].d_report, p->weights ? (double)p->weights[i] : 0.0 };
    FusePair f;
    memset(&f, 0, sizeof(f));
    f.points = last_pair->d_points ? last_pair->d_points : pr->d_rpoints;
    f.valid = last_pair->d_points ? last_pair->d_valid : reproj_flags(pr, pr->d_rreproj);
    f.X0 = pr->d_X[0]; f.X1 = pr->d_X[1]; f.K = pr->d_K;
    f.n = pr->n; f.ld = pr->ld;
    return launch_close_ring(ctx, rl.data(), num_links, f, *p, *out);                        // reads the pair: no stage changes
}

// ---- accessors ------------------------------------------------------------------------------------
int sfm_pair_ld(const sfm_pair *pair) { return pair ? pair->ld : 0; }
int sfm_pair_num_points(const sfm_pair *pair) { return pair ? pair->n : 0; }

// The stage a buffer id's contents belong to: without it sfm_pair_device_ptr answers (NULL, 0) where the getters answer SFM_E_STATE.
static uint32_t buffer_stage(int which)
{
    switch (which) {
    case SFM_BUF_REFINED_POSE: case SFM_BUF_REFINED_POINTS: case SFM_BUF_REPROJ: return kRefined;
    case SFM_BUF_VIEW_POSE: case SFM_BUF_VIEW_COUNTS: case SFM_BUF_VIEW_REPROJ: return kView;
    default: return 0;
    }
}

int sfm_pair_device_ptr(sfm_pair *pair, int which, void **d_ptr, size_t *bytes)
{
    SFM_REQUIRE(pair && d_ptr, SFM_E_INVALID, "null argument");
    void *p = nullptr; size_t b = 0;
    *d_ptr = nullptr;
    if (bytes) *bytes = 0;
    if (!pair->state.has(buffer_stage(which))) return SFM_OK;
    switch (which) {
    case SFM_BUF_X0: p = pair->d_X[0]; b = (size_t)3 * pair->ld * 4; break;
    case SFM_BUF_X1: p = pair->d_X[1]; b = (size_t)3 * pair->ld * 4; break;
    case SFM_BUF_U0: p = pair->d_U[0]; b = (size_t)3 * pair->ld * 4; break;
    case SFM_BUF_U1: p = pair->d_U[1]; b = (size_t)3 * pair->ld * 4; break;
    case SFM_BUF_E: p = pair->d_E; b = 36; break;
    case SFM_BUF_P: p = pair->d_P; b = 256; break;
    case SFM_BUF_PINV: p = pair->d_Pinv; b = 256; break;
    case SFM_BUF_POINTS: p = pair->d_points; b = (size_t)4 * pair->n * 4; break;
    case SFM_BUF_COUNTS: p = pair->slot[0].counts; b = (size_t)pair->state.last_count * 4; break;
    case SFM_BUF_MASK: p = pair->d_mask; b = (size_t)pair->n; break;
    case SFM_BUF_KEY: p = pair->slot[0].key; b = 8; break;
    case SFM_BUF_ECAND: p = pair->slot[0].Ecand; b = (size_t)pair->state.last_count * 36; break;
    case SFM_BUF_PIND: p = pair->d_Pind; b = 4; break;
    // the refinement's outputs (buffer_stage: NULL / 0 bytes unless they describe the current points)
    case SFM_BUF_REFINED_POSE: p = pair->d_rstate + refine_pose_offset(); b = 25 * 4; break;
    case SFM_BUF_REFINED_POINTS: p = pair->d_rpoints; b = (size_t)4 * pair->n * 4; break;
    case SFM_BUF_REPROJ: p = pair->d_rreproj; b = reproj_bytes((size_t)pair->n); break;
    // the registration's outputs: the same rule (sfm_register_view)
    case SFM_BUF_VIEW_POSE: p = pair->d_vstate + register_pose_offset(); b = 32 * 4; break;
    case SFM_BUF_VIEW_COUNTS: p = pair->d_vcounts; b = (size_t)pair->view_hyps * 4; break;
    case SFM_BUF_VIEW_REPROJ: p = pair->d_vreproj; b = reproj_bytes((size_t)pair->n); break;
#if SFM_AB
    // lab bench: what the pre-filter works from (profiles/fuzz_case.py): the per-hypothesis records of the last launch (64 bytes each; 16 with the
    // per-tile rule), the bound words (bound, -, eight box words), the cell table
    case SFM_AB_BUF_PF_RECORDS: p = pair->slot[0].pf; b = (size_t)pair->state.last_count * 64; break;
    case SFM_AB_BUF_BOUND_WORDS: p = pair->d_bound; b = 10 * sizeof(unsigned long long); break;
    case SFM_AB_BUF_CELLS: p = pair->d_cells; b = pair->d_cells ? ((size_t)pair->cells_mask + 1) * sizeof(uint32_t) : 0; break;
#endif
    default: set_error("unknown buffer id %d", which); return SFM_E_INVALID;
    }
    *d_ptr = p;
    if (bytes) *bytes = b;
    return SFM_OK;
}

int sfm_get_XU(sfm_pair *pair, int which, float *h_out)
{
    SFM_REQUIRE(pair && h_out, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(which >= SFM_BUF_X0 && which <= SFM_BUF_U1, SFM_E_INVALID, "which must be SFM_BUF_X0..U1");
    const float *src = which == SFM_BUF_X0 ? pair->d_X[0] : which == SFM_BUF_X1 ? pair->d_X[1]
                     : which == SFM_BUF_U0 ? pair->d_U[0] : pair->d_U[1];
    SFM_HIP_TRY(hipMemcpy2DAsync(h_out, (size_t)pair->n * 4, src, (size_t)pair->ld * 4, (size_t)pair->n * 4, 3,
                                 hipMemcpyDeviceToHost, pair->ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(pair->ctx->stream));
    return SFM_OK;
}

int sfm_get_E(sfm_pair *pair, float h_E[9])
{
    SFM_REQUIRE(pair && h_E, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kE);
    return copy_out(pair, h_E, pair->d_E, 36);
}

int sfm_get_best(sfm_pair *pair, uint32_t *hyp, uint32_t *count)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_NEED(pair, kE);
    uint32_t b[2];
    int rc = copy_out(pair, b, pair->d_best, sizeof(b));
    if (rc != SFM_OK) return rc;
    if (hyp) *hyp = b[0];
    if (count) *count = b[1];
    SFM_REQUIRE(b[0] != 0xFFFFFFFFu, SFM_E_STATE, "the finalized key named no hypothesis (empty shards, uninitialised key or failed all-reduce)");
    return SFM_OK;
}

int sfm_get_key(sfm_pair *pair, uint64_t *key)
{
    SFM_REQUIRE(pair && key, SFM_E_INVALID, "null argument");
    return copy_out(pair, key, pair->slot[0].key, 8);
}

int sfm_get_inlier_counts(sfm_pair *pair, int32_t *h_counts, size_t capacity)
{
    SFM_REQUIRE(pair && h_counts, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(capacity >= pair->state.last_count, SFM_E_INVALID, "capacity %zu < %u hypotheses", capacity, pair->state.last_count);
    if (pair->state.last_count == 0) return SFM_OK;
    return copy_out(pair, h_counts, pair->slot[0].counts, (size_t)pair->state.last_count * 4);
}

int sfm_get_E_candidates(sfm_pair *pair, float *h_E, size_t capacity_hyps)
{
    SFM_REQUIRE(pair && h_E, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(capacity_hyps >= pair->state.last_count, SFM_E_INVALID, "capacity too small");
    if (pair->state.last_count == 0) return SFM_OK;
    return copy_out(pair, h_E, pair->slot[0].Ecand, (size_t)pair->state.last_count * 36);
}

int sfm_get_inlier_mask(sfm_pair *pair, uint8_t *h_mask)
{
    SFM_REQUIRE(pair && h_mask, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kE);
    return copy_out(pair, h_mask, pair->d_mask, (size_t)pair->n);
}

int sfm_get_pose_candidates(sfm_pair *pair, float h_P[64])
{
    SFM_REQUIRE(pair && h_P, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kP);
    return copy_out(pair, h_P, pair->d_P, 256);
}

int sfm_get_pose_inverses(sfm_pair *pair, float h_Pinv[64])
{
    SFM_REQUIRE(pair && h_Pinv, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kPose);
    return copy_out(pair, h_Pinv, pair->d_Pinv, 256);
}

int sfm_get_pose_index(sfm_pair *pair, int *index)
{
    SFM_REQUIRE(pair && index, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kPose);
    int v[8];
    int rc = copy_out(pair, v, pair->d_Pind, sizeof(v));
    if (rc != SFM_OK) return rc;
    *index = v[0];
    if (v[5] & (1 << v[0])) { set_error("chosen pose candidate %d is singular", v[0]); return SFM_E_SINGULAR; }
    return SFM_OK;
}

int sfm_get_result(sfm_pair *pair, float h_record[28])
{
    SFM_REQUIRE(pair && h_record, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kE | kPose);
    float P[64]; int v[8]; uint32_t b[2];
    hipStream_t st = pair->ctx->stream;
    SFM_HIP_TRY(hipMemcpyAsync(h_record, pair->d_E, 9 * sizeof(float), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(P, pair->pose_mode == SFM_POSE_REFERENCE ? pair->d_Pinv : pair->d_P, sizeof(P), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(v, pair->d_Pind, sizeof(v), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(b, pair->d_best, sizeof(b), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    const int ind = v[0] >= 0 && v[0] < 4 ? v[0] : 0;
    for (int k = 0; k < 16; ++k) h_record[9 + k] = P[16 * ind + k];
    h_record[25] = (float)v[0]; h_record[26] = (float)b[1]; h_record[27] = (float)b[0];
    SFM_REQUIRE(b[0] != 0xFFFFFFFFu, SFM_E_STATE, "the finalized key named no hypothesis (empty shards, uninitialised key or failed all-reduce)");
    if (v[5] & (1 << ind)) { set_error("chosen pose candidate %d is singular", ind); return SFM_E_SINGULAR; }
    return SFM_OK;
}

int sfm_get_points(sfm_pair *pair, float *h_points)
{
    SFM_REQUIRE(pair && h_points, SFM_E_INVALID, "null argument");
    SFM_NEED(pair, kPoints3d);
    return copy_out(pair, h_points, pair->d_points, (size_t)4 * pair->n * 4);
}

int sfm_copy_points_to_vbo(sfm_pair *pair, float *d_positions, float *d_velocities, float scale)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_NEED(pair, kPoints3d);
    SFM_REQUIRE((((uintptr_t)d_positions | (uintptr_t)d_velocities) & 15u) == 0, SFM_E_INVALID, "vertex buffers must be 16-byte aligned");
    SFM_HIP_TRY(hipSetDevice(pair->ctx->device));
    return launch_points_to_vbo(pair, d_positions, d_velocities, scale);
}

int sfm_ransac_last_clock(sfm_pair *pair, double *shader_mhz)
{
    SFM_REQUIRE(pair && shader_mhz, SFM_E_INVALID, "null argument");
    unsigned long long c[2] = { 0, 0 };
    int rc = copy_out(pair, c, pair->d_clk, sizeof(c));
    if (rc != SFM_OK) return rc;
    *shader_mhz = c[1] ? 100.0 * (double)c[0] / (double)c[1] : 0.0;
    return SFM_OK;
}

#if SFM_AB
int sfm_ransac_last_phases(sfm_pair *pair, uint64_t ticks[8])
{
    SFM_REQUIRE(pair && ticks, SFM_E_INVALID, "null argument");
    constexpr int kN = 8;
    unsigned long long c[kN] = { 0 };
    int rc = copy_out(pair, c, pair->d_clk, sizeof(c));
    if (rc != SFM_OK) return rc;
    for (int k = 0; k < kN; ++k) ticks[k] = c[k];
    return SFM_OK;
}

int sfm_ransac_last_trace(sfm_pair *pair, uint64_t *words, size_t capacity, size_t *count)
{
    SFM_REQUIRE(pair && words && count, SFM_E_INVALID, "null argument");
    const size_t nblocks = (size_t)(pair->last_grid < kTraceBlocks ? pair->last_grid : kTraceBlocks);
    const size_t need = nblocks * kTraceWords;
    *count = 0;
    if (pair->last_kernel != SFM_KERNEL_PREFILTER || need == 0) return SFM_OK;
    SFM_REQUIRE(capacity >= need, SFM_E_INVALID, "capacity %zu < %zu words", capacity, need);
    int rc = copy_out(pair, words, pair->d_clk + 8, need * sizeof(uint64_t));
    if (rc == SFM_OK) *count = need;
    return rc;
}

int sfm_prefilter_probe(sfm_ctx *ctx, const float h_E[9], float threshold, float bound, const float h_point[4], int survive_all, float h_out[100])
{
    SFM_REQUIRE(ctx && h_E && h_point && h_out, SFM_E_INVALID, "null argument");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    float *d = nullptr;
    SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), 256 * sizeof(float)));      // result (100) + E (9 at 100) + one PfRecord at 128
    hipError_t e = hipMemcpyAsync(d + 100, h_E, 9 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    int rc = e == hipSuccess ? launch_prefilter_probe(ctx, d + 100, threshold, bound, h_point, survive_all, d) : SFM_E_HIP;
    if (rc == SFM_OK) {
        e = hipMemcpyAsync(h_out, d, 100 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { set_error("probe copy failed: %s", hipGetErrorString(e)); rc = SFM_E_HIP; }
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    return rc;
}

int sfm_prefilter_band_probe(sfm_ctx *ctx, const float h_E[9], float threshold, float bound, const float h_box[8], int b_safe, const float h_point[4],
                             int survive_all, float h_out[104])
{
    SFM_REQUIRE(ctx && h_E && h_point && h_out && h_box, SFM_E_INVALID, "null argument");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    float *d = nullptr;
    SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), 256 * sizeof(float)));      // result (104) + E (9 at 112) + one PfRecord at 128
    hipError_t e = hipMemsetAsync(d, 0, 256 * sizeof(float), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + 112, h_E, 9 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    int rc = e == hipSuccess ? launch_prefilter_band_probe(ctx, d + 112, threshold, bound, h_box, b_safe, h_point, survive_all, d) : SFM_E_HIP;
    if (rc == SFM_OK) {
        e = hipMemcpyAsync(h_out, d, 104 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { set_error("probe copy failed: %s", hipGetErrorString(e)); rc = SFM_E_HIP; }
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    return rc;
}
#endif

int sfm_ransac_last_launch(sfm_pair *pair, int *kernel, int *grid, int *block, int *lds_bytes)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    if (kernel) *kernel = pair->last_kernel;
    if (grid) *grid = pair->last_grid;
    if (block) *block = pair->last_block;
    if (lds_bytes) *lds_bytes = pair->last_lds;
    return SFM_OK;
}

int sfm_ransac_last_prefilter_rule(sfm_pair *pair, int *rule)
{
    SFM_REQUIRE(pair, SFM_E_INVALID, "null pair");
    SFM_REQUIRE(rule, SFM_E_INVALID, "null rule");
    *rule = pair->last_kernel == SFM_KERNEL_PREFILTER ? pair->pf_rule : 0;
    return SFM_OK;
}

} // extern "C"
