// pairs.hip -- sfm_process_pairs: the many-pairs driver behind BASELINE configs[4] (host code only), and the lanes it shares
// with sfm_extract_views (views.hip).
#include "common.hpp"
#include "pairs_batch.hpp"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace sfm {

// ---- lanes: the caller's context + auxiliary contexts with streams of their own (sfm_extract_views, sfm_process_pairs) ----
// out[0] = ctx, out[1 .. n) = the first n - 1 lane contexts, created on first use; every call hands them the caller's matcher
// choice and SFM_QUIRK_* flags (every pair of one call honours the same ones)
int lane_contexts(sfm_ctx *ctx, int n, sfm_ctx **out)
{
    out[0] = ctx;
    for (int l = 1; l < n; ++l) {
        if (!ctx->lane[l - 1]) {
            int rc = sfm_ctx_create(ctx->device, &ctx->lane[l - 1]);
            if (rc == SFM_OK) rc = sfm_ctx_own_stream(ctx->lane[l - 1]);
            if (rc != SFM_OK) return rc;
        }
        out[l] = ctx->lane[l - 1];
        out[l]->match_kernel = ctx->match_kernel;
        out[l]->quirks = ctx->quirks;
    }
    return SFM_OK;
}

// lanes 1 .. n - 1 start after everything already enqueued on the caller's stream (the features, typically)
int start_lanes_after(sfm_ctx *ctx, sfm_ctx *const *lanes, int n, hipEvent_t event)
{
    if (n <= 1) return SFM_OK;
    SFM_HIP_TRY(hipEventRecord(event, ctx->stream));
    for (int l = 1; l < n; ++l) SFM_HIP_TRY(hipStreamWaitEvent(lanes[l]->stream, event, 0));
    return SFM_OK;
}

// the caller's stream waits for lanes 1 .. n - 1; the first failure is kept in *rc (an earlier one is not overwritten)
static void join_lanes(sfm_ctx *ctx, sfm_ctx *const *lanes, int n, int *rc)
{
    for (int l = 1; l < n; ++l) {
        const hipError_t e1 = hipEventRecord(ctx->lane_ev[l], lanes[l]->stream);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(ctx->stream, ctx->lane_ev[l], 0) : e1;
        if (e2 != hipSuccess && *rc == SFM_OK) { set_error("lane join failed: %s", hipGetErrorString(e2)); *rc = SFM_E_HIP; }
    }
}

// Where the lanes' work of a call ends, whatever rc it got to: the caller's stream waits for them -- also when an enqueue failed,
// what the lanes already hold must not outlive this call's view of the buffers -- and a failed call waits for that stream.
static int close_lanes(sfm_ctx *ctx, sfm_ctx *const *lanes, int n, int rc)
{
    join_lanes(ctx, lanes, n, &rc);
    if (rc != SFM_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// Pairs that share their FIRST view stay on one lane in list order: the k-th distinct first view goes to lane k % nlanes.
static sfm_ctx *lane_of_first_view(std::vector<const void *> &first_views, const void *sift1, sfm_ctx *const *lanes, int nlanes)
{
    size_t v = 0;
    while (v < first_views.size() && first_views[v] != sift1) ++v;
    if (v == first_views.size()) first_views.push_back(sift1);
    return lanes[v % (size_t)nlanes];
}

// ---- many view pairs --------------------------------------------------------------------------------
// a pair sfm_process_pairs can work on: enough features for the 8-point solver, a second view (if given) that is not empty
static bool usable(const sfm_pair_desc &d) { return d.n1 >= 8 && (!d.d_sift2 || d.n2 >= 1); }

struct OwnedPair { int index, slot; bool usable; };      // index in the caller's list, slot in h_records / h_status

// one sfm_process_pairs call: what its steps share
struct PairsCall {
    sfm_ctx *ctx;
    const float *h_K, *h_Kinv;
    const sfm_pair_desc *pairs;
    uint32_t num_hypotheses;
    int pose_mode;
    std::vector<OwnedPair> owned;                        // the pairs first, first + stride, ... in list order
    int max_n = 0;
    // the context itself + up to three auxiliary contexts on streams of their own.  Pairs that share their FIRST view stay on
    // one lane in list order (MatchSiftData writes that view's match fields, fillXU reads them); everything else of a record
    // is only read, so different lanes may work on pairs that share views.
    sfm_ctx *lanes[sfm_ctx::kPairLanes] = {};
    int nlanes = 1;
    // host staging of the batched path's job arrays: they outlive every asynchronous copy made from them
    std::vector<PairJob> jobs;
    std::vector<int> db_rows;                            // per job: the rows of its second view the matcher visits
    std::vector<std::vector<MatchJob>> match_jobs;
};

static int own_pairs(PairsCall &c, int num_pairs, int first, int stride)
{
    for (int i = first, slot = 0; i < num_pairs; i += stride, ++slot) {
        const sfm_pair_desc &d = c.pairs[i];
        SFM_REQUIRE(d.n1 >= 0 && d.n2 >= 0, SFM_E_INVALID, "pair %d: negative feature count", i);
        SFM_REQUIRE(d.n1 == 0 || d.d_sift1, SFM_E_INVALID, "pair %d: null feature pointer", i);
        if (d.n1 > c.max_n) c.max_n = d.n1;
        c.owned.push_back({ i, slot, usable(d) });
    }
    return SFM_OK;
}

static int open_lanes(PairsCall &c)
{
    static_assert(sfm_ctx::kViewLanes >= sfm_ctx::kPairLanes, "the lane contexts are shared with sfm_extract_views");
    c.nlanes = c.owned.size() >= 8 ? sfm_ctx::kPairLanes : 1;
    const int rc = lane_contexts(c.ctx, c.nlanes, c.lanes);
    if (rc != SFM_OK) return rc;
    for (int l = 0; l < c.nlanes; ++l)
        if (!c.ctx->lane_ev[l]) SFM_HIP_TRY(hipEventCreateWithFlags(&c.ctx->lane_ev[l], hipEventDisableTiming));
    return SFM_OK;
}

// ONE pooled Image_pair per lane at the largest size (the reference constructs one per pair: ~20 cudaMalloc / cudaFree each)
static int pool_pairs(PairsCall &c)
{
    if (c.max_n < 8) return SFM_OK;
    for (int l = 0; l < c.nlanes; ++l) {
        sfm_ctx *lc = c.lanes[l];
        if (lc->pool_pair && (lc->pool_pair->cap_points < c.max_n || memcmp(lc->pool_K, c.h_K, 36) != 0 || memcmp(lc->pool_Kinv, c.h_Kinv, 36) != 0)) {
            (void)sfm_pair_destroy(lc->pool_pair);
            lc->pool_pair = nullptr;
        }
        if (!lc->pool_pair) {
            const int rc = sfm_pair_create(lc, c.h_K, c.h_Kinv, 2, c.max_n, &lc->pool_pair);
            if (rc == SFM_OK) { lc->pool_pair->holds_ctx_ref = false; lc->refs--; }      // the context's own pair: destroyed WITH the context
            if (rc != SFM_OK) return rc;
            memcpy(lc->pool_K, c.h_K, 36); memcpy(lc->pool_Kinv, c.h_Kinv, 36);
        }
    }
    return SFM_OK;
}

static uint32_t pair_hypotheses(const PairsCall &c, const sfm_pair_desc &d) { return c.num_hypotheses ? c.num_hypotheses : (uint32_t)(d.n1 / 8); }

// The batched path (pairs_batch.hpp) is taken for the reference's own pipeline: SFM_POSE_REFERENCE, K^-1 with last row (0 0 1),
// 1 .. 4096 hypotheses per pair, every usable pair with a second view.  Returns the largest hypothesis count, 0: not batchable.
static uint32_t batchable(const PairsCall &c, bool unbatched_env)
{
    if (c.pose_mode != SFM_POSE_REFERENCE || !unit_z_Kinv(c.h_Kinv) || c.owned.size() < 4 || unbatched_env) return 0;
    uint32_t max_H = 0;
    for (const OwnedPair &o : c.owned) {
        if (!o.usable) continue;
        // already matched pairs (no second view given) read match_xpos / match_ypos of the records: not supported by the batch
        // kernels -- such lists take the per-pair loop, decided HERE, before anything has been launched for them
        if (!c.pairs[o.index].d_sift2) return 0;
        const uint32_t H = pair_hypotheses(c, c.pairs[o.index]);
        if (H > 4096u || H < 1u) return 0;
        max_H = std::max(max_H, H);
    }
    return max_H;
}

// the batch workspace: the job array in front, then every job's arrays (run over a null base: the bytes to allocate)
static size_t carve_batch(Carver &ws, std::vector<PairJob> &jobs)
{
    (void)ws.take<PairJob>(jobs.size());
    for (PairJob &j : jobs) carve_pair_job(ws, j);
    return ws.used;
}

// one PairJob per usable pair, its arrays in the context's workspace; the jobs go to the device
static int upload_jobs(PairsCall &c)
{
    sfm_ctx *ctx = c.ctx;
    for (const OwnedPair &o : c.owned) {
        if (!o.usable) continue;
        const sfm_pair_desc &d = c.pairs[o.index];
        PairJob j{};
        j.s1 = d.d_sift1; j.s2 = d.d_sift2; j.n = d.n1; j.ld = round_up(d.n1, 128);
        j.H = pair_hypotheses(c, d);
        sfm_ransac_params dp; sfm_ransac_default_params(&dp, d.n1);
        j.seed = dp.seed; j.thr = dp.threshold;
        j.record = ctx->pool_records + (size_t)o.slot * SFM_RECORD_FLOATS;
        c.jobs.push_back(j);
        c.db_rows.push_back(match_db_rows(ctx, d.n2));
    }
    Carver sizes(nullptr);
    const int rc = grow(&ctx->batch_ws, &ctx->batch_ws_bytes, carve_batch(sizes, c.jobs), ctx->stream);
    if (rc != SFM_OK) return rc;
    Carver ws(ctx->batch_ws);
    carve_batch(ws, c.jobs);
    SFM_HIP_TRY(hipMemcpyAsync(ctx->batch_ws, c.jobs.data(), c.jobs.size() * sizeof(PairJob), hipMemcpyHostToDevice, ctx->stream));
    return SFM_OK;
}

// MatchSiftData per pair: the SiftPoint fields of the first view as always (pairs that share their first view stay on one lane
// in list order: the fields end up as after the sequential loop) + the index array the batch reads
static int enqueue_matches(PairsCall &c)
{
    const int ldf = (int)(sizeof(sfm_sift_point) / sizeof(float));
    std::vector<const void *> first_views;
    const std::vector<MatchRun> runs = plan_match_runs(c.jobs.data(), c.db_rows.data(), c.jobs.size(),
                                                       [&](int n1, int n2) { return match_pick_jobs(c.ctx, n1, n2); });
    for (const MatchRun &r : runs) {
        const PairJob &j = c.jobs[r.begin];
        sfm_sift_point *s1 = const_cast<sfm_sift_point *>(j.s1);
        sfm_ctx *lc = lane_of_first_view(first_views, j.s1, c.lanes, c.nlanes);
        int rc;
        if (r.end - r.begin < 2) {
            rc = match_records(lc, s1, j.n, j.s2, c.db_rows[r.begin], const_cast<int *>(j.m_idx));      // (trimming again changes nothing)
        } else {
            std::vector<MatchJob> mj(r.end - r.begin);
            for (size_t k = r.begin; k < r.end; ++k) {
                MatchJob &m = mj[k - r.begin];
                m.db = c.jobs[k].s2->data; m.ndb = c.db_rows[k]; m.lddb = ldf; m.sift2 = c.jobs[k].s2;
                m.out_idx = const_cast<int *>(c.jobs[k].m_idx);
            }
            mj.back().sift1 = s1;                                           // as after the sequential loop: the last match's fields
            c.match_jobs.push_back(std::move(mj));
            std::vector<MatchJob> &kept = c.match_jobs.back();
            rc = launch_match_jobs(lc, j.s1->data, j.n, ldf, kept.data(), (int)kept.size(), r.kernel);
            if (rc == SFM_OK && (lc->quirks & SFM_QUIRK_MATCH_AMBIGUITY))    // the record fields are the LAST match's: so is the reference's ambiguity
                rc = launch_match_ambiguity_quirk(lc, j.s1->data, j.n, ldf, kept.back().db, kept.back().ndb, ldf, s1, nullptr);
        }
        if (rc != SFM_OK) return rc;
    }
    return SFM_OK;
}

// the rest of the chain for ALL pairs of the call, on the caller's stream: fill_xu_pairs | ransac_pairs_solve +
// ransac_fused_pairs | choose_pose_pairs + triangulate_pairs -- five launches
static int enqueue_batch_chain(PairsCall &c, uint32_t max_H)
{
    const PairJob *d_jobs = static_cast<const PairJob *>(c.ctx->batch_ws);
    const int njobs = (int)c.jobs.size();
    int max_ld = 0, max_n = 0;
    for (const PairJob &j : c.jobs) { max_ld = std::max(max_ld, j.ld); max_n = std::max(max_n, j.n); }
    int rc = launch_fill_xu_pairs(c.ctx, d_jobs, njobs, max_ld, c.h_Kinv);
    // eight blocks of eight wavefronts per pair: each stages the pair's points once and runs its share of the batches
    const int bpp = (int)std::min<uint32_t>(8u, (max_H + 7u) / 8u);
    if (rc == SFM_OK) rc = launch_fused_pairs(c.ctx, d_jobs, njobs, bpp, max_H);
    if (rc == SFM_OK) rc = launch_finalize_pose_pairs(c.ctx, d_jobs, njobs, max_n);
    return rc;
}

// The batched path: the matcher stays one launch per pair or run of pairs (it fills the chip), everything after it is FIVE
// launches for all pairs of the call -- 630 pairs x 5 small launches are bound by the host's launch rate, not by the GPU.
// Results are bit-identical to the per-pair path (same device functions on the same inputs:
// tests/test_gpu_dino.py::test_dino_ring_batched_equals_per_pair, tests/test_gpu_pairs_paths.py).
static int run_batched(PairsCall &c, uint32_t max_H)
{
    int rc = upload_jobs(c);
    if (rc == SFM_OK) rc = start_lanes_after(c.ctx, c.lanes, c.nlanes, c.ctx->lane_ev[0]);
    if (rc == SFM_OK) rc = enqueue_matches(c);
    rc = close_lanes(c.ctx, c.lanes, c.nlanes, rc);
    if (rc != SFM_OK) return rc;
    rc = enqueue_batch_chain(c, max_H);
    if (rc != SFM_OK) return close_lanes(c.ctx, c.lanes, c.nlanes, rc);
    c.ctx->last_pairs_batched = 1;
    return SFM_OK;
}

// per pair: MatchSiftData (optional) -> fillXU -> estimateE -> pose candidates -> choosePose -> linear triangulation
// (src/main.cpp:282-307), everything enqueued back to back, no host synchronisation, the record stays on the device
static int enqueue_pair(PairsCall &c, const OwnedPair &o, sfm_ctx *lc)
{
    const sfm_pair_desc &d = c.pairs[o.index];
    sfm_pair *ip = lc->pool_pair;
    int rc = d.d_sift2 ? sfm_match(lc, d.d_sift1, d.n1, d.d_sift2, d.n2) : SFM_OK;
    if (rc == SFM_OK) rc = sfm_pair_reset(ip, d.n1);
    if (rc == SFM_OK) rc = sfm_fill_xu(ip, d.d_sift1);
    if (rc != SFM_OK) return rc;
    sfm_ransac_params p;
    sfm_ransac_default_params(&p, d.n1);
    if (c.num_hypotheses) p.num_hypotheses = c.num_hypotheses;
    rc = sfm_estimate_E(ip, &p);
    // poses, triangulation and the record: one launch in SFM_POSE_REFERENCE (sfm_pose_chain), four otherwise
    if (rc == SFM_OK) rc = pose_chain(ip, c.pose_mode, c.ctx->pool_records + (size_t)o.slot * SFM_RECORD_FLOATS);
    return rc;
}

static int run_per_pair(PairsCall &c)
{
    std::vector<const void *> first_views;
    int rc = SFM_OK;
    for (const OwnedPair &o : c.owned) {
        if (!o.usable) continue;
        rc = enqueue_pair(c, o, lane_of_first_view(first_views, c.pairs[o.index].d_sift1, c.lanes, c.nlanes));
        if (rc != SFM_OK) break;
    }
    return close_lanes(c.ctx, c.lanes, c.nlanes, rc);
}

// ONE read-back for all pairs of this rank; unusable pairs: a record of -1, SFM_E_INVALID
static int read_records(const PairsCall &c, float *h_records, int *h_status)
{
    sfm_ctx *ctx = c.ctx;
    std::vector<float> rec(c.owned.size() * SFM_RECORD_FLOATS);
    SFM_HIP_TRY(hipMemcpyAsync(rec.data(), ctx->pool_records, rec.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    int worst = SFM_OK;
    for (const OwnedPair &o : c.owned) {
        float *out = h_records + (size_t)o.slot * 28;
        const float *in = rec.data() + (size_t)o.slot * SFM_RECORD_FLOATS;
        int status = o.usable ? SFM_OK : SFM_E_INVALID;
        if (!o.usable) {
            for (int k = 0; k < 28; ++k) out[k] = -1.0f;
        } else {
            memcpy(out, in, 28 * sizeof(float));
            if (in[28] != 0.0f) {
                set_error("pair %d: chosen pose candidate is singular", o.index);
                status = worst = SFM_E_SINGULAR;
            }
        }
        if (h_status) h_status[o.slot] = status;
    }
    return h_status ? SFM_OK : worst;
}

} // namespace sfm

using namespace sfm;

extern "C" {

int sfm_process_pairs(sfm_ctx *ctx, const float h_K[9], const float h_Kinv[9], const sfm_pair_desc *pairs, int num_pairs,
                      int first, int stride, uint32_t num_hypotheses, int pose_mode, float *h_records, int *h_status)
{
    SFM_REQUIRE(ctx && h_K && h_Kinv && h_records, SFM_E_INVALID, "null argument");
    SFM_REQUIRE(num_pairs >= 0 && first >= 0 && stride >= 1, SFM_E_INVALID, "bad pair range (%d pairs, first %d, stride %d)", num_pairs, first, stride);
    SFM_REQUIRE(pose_mode == SFM_POSE_REFERENCE || pose_mode == SFM_POSE_CORRECT, SFM_E_INVALID, "unknown pose mode %d", pose_mode);
    SFM_REQUIRE(num_pairs == 0 || pairs, SFM_E_INVALID, "null pair list");
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    PairsCall c{ ctx, h_K, h_Kinv, pairs, num_hypotheses, pose_mode };
    int rc = own_pairs(c, num_pairs, first, stride);
    if (rc != SFM_OK || c.owned.empty()) return rc;
    rc = open_lanes(c);
    if (rc == SFM_OK) rc = pool_pairs(c);
    if (rc == SFM_OK) rc = grow(&ctx->pool_records, &ctx->pool_records_cap, c.owned.size() * SFM_RECORD_FLOATS, ctx->stream);
    if (rc != SFM_OK) return rc;
    rc = start_lanes_after(ctx, c.lanes, c.nlanes, ctx->lane_ev[0]);
    if (rc != SFM_OK) return close_lanes(ctx, c.lanes, c.nlanes, rc);       // from here on every failure leaves through close_lanes
    ctx->last_pairs_batched = 0;
    const bool unbatched_env = getenv("SFM_PAIRS_UNBATCHED") != nullptr;      // A/B and tests: read on EVERY call (sfm_ctx_last_pairs_batched says what ran)
    const uint32_t max_H = batchable(c, unbatched_env);
    rc = max_H > 0 ? run_batched(c, max_H) : run_per_pair(c);
    if (rc != SFM_OK) return rc;
    return read_records(c, h_records, h_status);
}

int sfm_ctx_last_pairs_batched(sfm_ctx *ctx, int *batched)
{
    SFM_REQUIRE(ctx && batched, SFM_E_INVALID, "null argument");
    *batched = ctx->last_pairs_batched;
    return SFM_OK;
}

} // extern "C"
