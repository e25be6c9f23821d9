// common.hpp -- host-side state behind the C ABI (include/sfm_amd.h) and launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <atomic>
#include <type_traits>
#include "../../include/sfm_amd.h"
#include "pair_state.hpp"
#include "job_order.hpp"
#if SFM_AB
#include "../../include/sfm_amd_ab.h"
#endif

// A/B switches (sfm_ransac_params.reserved[]): read only by the lab-bench flavour of the library (make ab, -DSFM_AB=1).  In the
// product build they fold to 0 -- the variants they select are not compiled in -- and resolve_shard() (abi.hip) refuses
// non-zero values with SFM_E_INVALID.
#if SFM_AB
#define SFM_SW(p, i) ((p).reserved[i])
#else
#define SFM_SW(p, i) 0
#endif

namespace sfm {

void set_error(const char *fmt, ...);

#define SFM_HIP_TRY(expr)                                                                      \
    do {                                                                                       \
        hipError_t err__ = (expr);                                                             \
        if (err__ != hipSuccess) {                                                             \
            ::sfm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), __FILE__, __LINE__); \
            return err__ == hipErrorOutOfMemory ? SFM_E_NOMEM : SFM_E_HIP;                     \
        }                                                                                      \
    } while (0)

#define SFM_REQUIRE(cond, code, ...)                                                           \
    do {                                                                                       \
        if (!(cond)) { ::sfm::set_error(__VA_ARGS__); return (code); }                         \
    } while (0)

// a pending pipelined burst (sfm_estimate_E_pipelined) is ordered in front of whatever the entry point enqueues on the context's stream
#define SFM_FLUSH(pair)                                                                        \
    do { if ((pair)->pipe_pending) { const int rcf__ = sfm_pair_flush(pair); if (rcf__ != SFM_OK) return rcf__; } } while (0)

// the pair's results the call reads must describe its current points (pair_state.hpp)
#define SFM_NEED(pair, stages)                                                                 \
    SFM_REQUIRE((pair)->state.has(stages), SFM_E_STATE, "%s", ::sfm::pair_stage_hint((pair)->state.missing(stages)))

constexpr int kTraceBlocks = 1024;     // blocks of a scoring launch whose start / end stamps are kept (sfm_ransac_last_trace)
constexpr int kTraceWords = 20;        // per block: start, end of wavefront 0, (XCC id << 32 | hardware id), tile << 32 | column, 16 wavefront ends (100 MHz ticks)
constexpr int kClkWords = 8 + kTraceBlocks * kTraceWords;
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Grows a scratch buffer to at least `need` elements (bytes for a void *), contents lost.  What is already enqueued on `st` may
// still use the old one: wait for it before freeing.
template <typename T, typename N>
inline int grow(T **buf, N *have, size_t need, hipStream_t st)
{
    if (need <= (size_t)*have) return SFM_OK;
    SFM_HIP_TRY(hipStreamSynchronize(st));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    SFM_HIP_TRY(hipMalloc(reinterpret_cast<void **>(buf), need * sizeof(std::conditional_t<std::is_void<T>::value, char, T>)));
    *have = (N)need;
    return SFM_OK;
}

// the last row of K^-1 is (0 0 1): every normalised z is exactly 1
inline bool unit_z_Kinv(const float h_Kinv[9]) { return h_Kinv[6] == 0.0f && h_Kinv[7] == 0.0f && h_Kinv[8] == 1.0f; }

// Consecutive arrays carved out of one device buffer.  A buffer's layout is ONE function that takes its arrays from a Carver
// and returns used: run over the buffer it yields the pointers, run over a null base the size to allocate.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(void *buffer) : base(reinterpret_cast<uintptr_t>(buffer)) {}
    // the array starts at the next multiple of `align` bytes (a power of two) from the base
    template <typename T> T *take(size_t count, size_t align = 1)
    {
        used = (used + align - 1) & ~(align - 1);
        T *p = reinterpret_cast<T *>(base + used);
        used += count * sizeof(T);
        return p;
    }
};

// The job array of a batched call (one per call in sfm_ctx: sfm_refine_pairs, sfm_register_views, sfm_triangulate_views,
// sfm_adjust_views, sfm_align_pairs, sfm_fuse_chain): a context-owned device array + pinned staging, grown on demand, and the
// event that sits behind the upload.  One mechanism, parameterised by the element size.
struct JobArray {
    void *dev = nullptr, *pinned = nullptr;
    size_t cap = 0;                    // jobs
    hipEvent_t ev = nullptr;
};

// Room for `count` jobs of `elem` bytes (growth is rare: the stream is drained before the old device buffer goes).  The staging
// buffer is rewritten by the host: the upload of the call before must have left it -- the only host wait of a batched call.
inline int job_array_reserve(JobArray &j, size_t count, size_t elem, hipStream_t st)
{
    if (!j.ev) SFM_HIP_TRY(hipEventCreateWithFlags(&j.ev, hipEventDisableTiming));
    SFM_HIP_TRY(hipEventSynchronize(j.ev));                            // (an event never recorded is complete)
    if (count <= j.cap) return SFM_OK;
    const size_t want = count > 2 * j.cap ? count : 2 * j.cap;
    if (j.pinned) (void)hipHostFree(j.pinned);
    j.pinned = nullptr;
    j.cap = 0;                                                         // the size counts for both: it is set when both exist
    SFM_HIP_TRY(hipHostMalloc(&j.pinned, want * elem, hipHostMallocDefault));
    size_t have = 0;
    const int rc = grow(&j.dev, &have, want * elem, st);
    if (rc != SFM_OK) return rc;
    j.cap = want;
    return SFM_OK;
}

// the staged jobs to the device: ONE copy, the event behind it
inline int job_array_upload(JobArray &j, size_t count, size_t elem, hipStream_t st)
{
    SFM_HIP_TRY(hipMemcpyAsync(j.dev, j.pinned, count * elem, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipEventRecord(j.ev, st));
    return SFM_OK;
}

// The prologue of a batched launch (count >= 1): room for the jobs, the caller's entries by decreasing key (job_order.hpp),
// fill(h_jobs[k], i) for job k from caller index i, the upload.  *d_jobs: the device array; *largest: the key of job 0.
template <typename Job, typename Key, typename Fill>
inline int job_array_stage(JobArray &j, int count, hipStream_t st, Key key, Fill fill, const Job **d_jobs, int *largest)
{
    int rc = job_array_reserve(j, (size_t)count, sizeof(Job), st);
    if (rc != SFM_OK) return rc;
    const std::vector<int> order = order_by_decreasing_key(count, key);
    Job *h_jobs = static_cast<Job *>(j.pinned);
    for (int k = 0; k < count; ++k) fill(h_jobs[k], order[(size_t)k]);
    *d_jobs = static_cast<const Job *>(j.dev);
    *largest = key(order[0]);
    return job_array_upload(j, (size_t)count, sizeof(Job), st);
}

inline void job_array_free(JobArray &j)
{
    if (j.pinned) (void)hipHostFree(j.pinned);
    if (j.dev) (void)hipFree(j.dev);
    if (j.ev) (void)hipEventDestroy(j.ev);
    j = JobArray();
}

} // namespace sfm

struct sfm_ctx {
    // Objects that point at the context (every sfm_pair, every sfm_comm) hold a reference: sfm_ctx_destroy on a context that still
    // has some only marks it, the last of them to go destroys it -- whatever order a host language's finalizers run in (Python's
    // cyclic collector destroys a context and its pairs in arbitrary order), nobody is left with a dangling pointer.
    std::atomic<int> refs{0};          // (pairs may be destroyed on a worker thread while the owner lets go of the context)
    std::atomic<bool> destroy_requested{false};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;           // created by sfm_ctx_own_stream, destroyed with the context
    int num_cus = 256;
    unsigned int quirks = 0;           // SFM_QUIRK_* (sfm_ctx_set_quirks)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // optional per-kernel stopwatch (sfm_ctx_kernel_timing): event triples around solve / score
    bool timing = false;
    static constexpr int kTimingSlots = 256;
    hipEvent_t tev[kTimingSlots][3] = {};
    int tcount = 0;
    // matcher scratch: per-split partial (best, second, index) records
    void *match_ws = nullptr;
    size_t match_ws_bytes = 0;
    size_t match_ticket_bytes = 0;
    unsigned int match_epoch = 0;      // one-match launches of the exact matcher tag their partials with it (match.hip: POLL)
    void *match_poll_ws = nullptr;     // ... in a buffer nothing else writes (epoch-tagged 64-bit words)
    size_t match_poll_ws_bytes = 0;
    unsigned int *match_poll_flag = nullptr;   // pinned host word: raised by a polled merge that gave up (match.hip: match_poll_check)
    void *match_jobs_ws = nullptr;     // launch_match_jobs: the job array, tickets and per-split partials of every match of the launch
    size_t match_jobs_ws_bytes = 0;     // zeroed ticket area in front of the partials (grows with the query-block count)
    // pre-filter matcher (match_prefilter.hip): fp16 copies, norms, per-split partials, candidate lists
    void *match_pf_ws = nullptr;
    size_t match_pf_ws_bytes = 0;
    int match_kernel = 0;              // SFM_MATCH_AUTO / _EXACT / _PREFILTER / _FUSED (sfm_ctx_set_match_kernel)
    int last_match_kernel = 0;         // what the last sfm_match / sfm_match_soa call ran
    int last_pairs_batched = 0;        // the last sfm_process_pairs call took the batched path (sfm_ctx_last_pairs_batched)
    void *homo_ws = nullptr;           // homography RANSAC scratch
    size_t homo_ws_bytes = 0;
    void *sift_temp = nullptr;         // pyramid + DoG planes when the caller passes no temp memory
    size_t sift_temp_bytes = 0;
    void *sift_ws = nullptr;           // counters, candidates, secondary orientations
    size_t sift_ws_bytes = 0;
    // many-pairs driver (sfm_process_pairs): pooled Image_pair and device-side result records; up to three auxiliary
    // contexts with streams of their own, so that the small single-wave stages of one pair overlap another pair's matcher
    static constexpr int kPairLanes = 4;               // streams of sfm_process_pairs
    static constexpr int kViewLanes = 8;               // streams (and worker threads) of sfm_extract_views: a view is a chain of thirteen
                                                       // small launches + a count read-back, ~0.15 ms of latency whatever the GPU is doing
    sfm_ctx *lane[kViewLanes - 1] = {};
    hipEvent_t lane_ev[kViewLanes] = {};
    sfm_pair *pool_pair = nullptr;
    // many-views front end (sfm_extract_views): pinned staging + device image, one per context
    float *views_pinned = nullptr, *views_image = nullptr;
    size_t views_floats = 0;
    hipEvent_t views_ev = nullptr;
    float pool_K[9] = {}, pool_Kinv[9] = {};
    float *pool_records = nullptr;
    size_t pool_records_cap = 0;       // floats
    void *batch_ws = nullptr;          // sfm_process_pairs, batched path: the PairJob array + every pair's buffers (pairs_batch.hpp)
    size_t batch_ws_bytes = 0;
    // sfm_refine_pairs / sfm_register_views / sfm_triangulate_views: the RefineArgs (refine.hip) / RegisterArgs (register.hip) /
    // ViewPointsArgs (view_points.hip) of a call; sfm_adjust_views: the AdjustArgs (adjust.hip); sfm_align_pairs: the AlignArgs
    // (align.hip); sfm_fuse_chain and sfm_adjust_chain: the FusePair (fuse_math.hpp) of every pair
    // sfm_close_ring: the RingLink (ring_math.hpp) of every link
    sfm::JobArray refine_jobs, register_jobs, view_points_jobs, adjust_jobs, align_jobs, fuse_jobs, chain_jobs, ring_jobs;
    sfm::JobArray fundamental_jobs;    // sfm_pair_fundamentals: the FundamentalJob (pair_fundamentals.hip) of every pair
    sfm::JobArray guided_jobs;         // sfm_match_guided_pairs: the pinned staging of the launches' GuidedJob tables (match_guided_pairs.hip); the tables themselves sit in match_jobs_ws
    void *fuse_ws = nullptr;           // sfm_fuse_chain: per-node keys, successors, path lengths and classes, the block counts (fuse.hip)
    size_t fuse_ws_bytes = 0;
    void *chain_ws = nullptr;          // sfm_adjust_chain and sfm_adjust_ring: states, points, partial bands, the band and the segments (chain_adjust.hip); sfm_intersect_tracks: the list of long tracks
    size_t chain_ws_bytes = 0;
    void *ring_ws = nullptr;           // sfm_close_ring: the fp64 frames, weights and running sums, the seam's block partials (ring.hip)
    size_t ring_ws_bytes = 0;
    void *sift_job = nullptr;          // the extraction in flight (sift.hip: SiftJob), sfm_extract_sift_begin .. _end
    // kernels that already opted in to > 64 KiB of dynamic LDS on THIS context's device (function attributes are
    // per device; a context is used by one host thread at a time, so no process-wide flag)
    static constexpr int kBigLdsSlots = 16;
    const void *big_lds_done[kBigLdsSlots] = {};
};

// Allows `kernel` up to 160 KiB of dynamic LDS on the context's device, once per context.
inline int allow_big_lds(sfm_ctx *ctx, const void *kernel)
{
    for (int i = 0; i < sfm_ctx::kBigLdsSlots; ++i) {
        if (ctx->big_lds_done[i] == kernel) return SFM_OK;
        if (ctx->big_lds_done[i] == nullptr) {
            SFM_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->big_lds_done[i] = kernel;
            return SFM_OK;
        }
    }
    SFM_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));   // table full: just set it
    return SFM_OK;
}

// The per-shard buffers of a scoring launch, grown on demand (ransac.hip: ensure_hyp_capacity) -- except the key, which the pair
// allocates.  A launch is handed ONE of the pair's two and the stream it goes to; it touches no other.
struct ShardSlot {
    int *counts = nullptr;
    uint32_t *tick = nullptr;          // pre-filter kernel: per 32-hypothesis group, how many tiles have been added
    float *Ecand = nullptr;
    void *pf = nullptr;                // pre-filter kernel: one PfRecord (64 bytes, prefilter_record.hpp) per hypothesis of the shard
    unsigned long long *key = nullptr; // [0] packed best of the slot's last score, [1] scratch
    size_t cap_hyps = 0;
};

inline void shard_slot_free(ShardSlot &s)
{
    for (void *b : { (void *)s.counts, (void *)s.tick, (void *)s.Ecand, s.pf, (void *)s.key }) if (b) (void)hipFree(b);
    s = ShardSlot();
}

struct sfm_pair {
    sfm_ctx *ctx = nullptr;
    int image_count = 2;
    int n = 0;          // num_points
    int cap_points = 0; // creation-time num_points (sfm_pair_reset may shrink n below it)
    int ld = 0;         // padded row length of X / U (multiple of 128, tail = NaN)
    float *d_K = nullptr, *d_Kinv = nullptr;
    float *d_U[2] = { nullptr, nullptr };
    float *d_X[2] = { nullptr, nullptr };
    float4 *d_pts4 = nullptr;          // (x1x, x1y, x2x, x2y) per correspondence, written by fillXU: ONE 16-byte gather per sampled point
    uint32_t sorted_epoch = 0;         // the fillXU epoch d_pts4s was built for
    uint32_t pf_seen_epoch = 0;        // the fillXU epoch of the last pre-filter launch (the first launch of an epoch runs per-hypothesis records)
    int pf_rule = 0;                   // the rule of the launch being issued (prefilter_pick_rule)
    uint32_t *d_buckets = nullptr;     // scratch of the bucket ordering: per-block histograms + bucket bases (pf_bucket_*_kernel)
    size_t bucket_words = 0;
    uint32_t *d_tile_boxes = nullptr;  // eight words per scoring tile of d_pts4s: ordered bits of its coordinate maxima (pf_bucket_scatter_kernel)
    int boxes_words = 0, boxes_tile = 0;   // words allocated / the tile size the boxes were computed for
    float4 *d_pts4s = nullptr;         // the same records in Morton order of the first view's position (pre-filter scoring: tiles with small
                                       // bounding boxes, ransac_prefilter.hip: pf_bucket_*_kernel); built by the second scoring launch after a fillXU (launch_pf_cells)
    float *d_E = nullptr;              // 9
    float *d_P = nullptr;              // 4 x 16 candidates
    float *d_Pinv = nullptr;           // 4 x 16 inverses
    int   *d_Pind = nullptr;           // chosen index (+ 4 cheirality vote counters)
    float *d_points = nullptr;         // 4 x n
    uint8_t *d_mask = nullptr;         // n
    uint32_t *d_best = nullptr;        // [0] hyp, [1] count of the finalized hypothesis
    // [8 ...]: trace of the last pre-filter scoring launch, kTraceWords per block (sfm_ransac_last_trace)
    unsigned long long *d_clk = nullptr;   // [0] shader-clock ticks, [1] 100 MHz ticks over block 0 of the last ransac_score_waves launch
    // slot[0]: the serial calls' per-shard buffers (what the getters and a finalize of the pair's own key read), its key allocated with
    // the pair.  slot[1]: sfm_ransac_score_into_slot's second set -- two shards in flight on two streams -- its key allocated by the first
    // such call.  The fused / MFMA families reduce into the slot's key, then copy to the caller's.
    ShardSlot slot[2];
    unsigned long long *d_bound = nullptr; // (fillXU epoch << 32) | bits of the largest |coordinate| <= 48 over all points: atomicMax, never reset;
                                           // words 2..9: the same for the coordinate ranges of the two views (pf_cells_build_kernel; prefilter_math.hpp: pf_box_from_words)
    uint32_t bound_epoch = 0;
    uint32_t *d_cells = nullptr;       // pre-filter: open-addressing table of the occupied zero-divisor grid cells of ALL points (launch_pf_cells)
    hipEvent_t cells_ev = nullptr;     // recorded behind the build: launches on ANOTHER stream (two-slot pipelining) wait for it
    hipStream_t cells_stream = nullptr;
    uint32_t cells_cap = 0, cells_mask = 0, cells_epoch = 0;   // slots allocated / in use - 1 / the fillXU epoch the table was built for
    uint32_t cand_h0 = 0, cand_seed = 0;   // what slot[0].Ecand holds after a serial score call: shard start, sampler settings
    const int32_t *cand_indices = nullptr;
    int cand_sweeps = 0;
    bool cand_given = false;               // slot[0].Ecand holds caller-supplied matrices (sfm_ransac_score_candidates), not tuple-derived ones
    // sfm_estimate_E_pipelined: odd steps run on this stream, even steps on the context's; one event per slot
    hipStream_t pipe_stream = nullptr;
    hipEvent_t pipe_final[2] = { nullptr, nullptr }, pipe_call = nullptr;
    uint64_t *pipe_keys = nullptr;
    unsigned long long pipe_step = 0;
    bool pipe_pending = false;
    bool holds_ctx_ref = false;        // this pair counts in ctx->refs (every pair but the context's own pooled one)
    sfm::PairState state;              // which results are current + what was derived from the points (pair_state.hpp)
    float h_Kinv[9] = {};
    int pose_mode = SFM_POSE_REFERENCE;
    // sfm_refine_two_view: allocated at the first call, sized to cap_points (refine.hip)
    float *d_rstate = nullptr;         // candidates, refined pose + E, report
    float *d_rpoints = nullptr;        // 4 x n refined / re-triangulated points
    float *d_rreproj = nullptr;        // n errors, then n uint8 used flags
    void *d_rwork = nullptr;           // start points of the four candidates, compacted observations / points, index maps, votes
    // sfm_register_view: allocated at the first call (per-point buffers sized to cap_points, per-hypothesis buffers grown on
    // demand) (register.hip)
    float *d_vstate = nullptr;         // refined + RANSAC pose, report, key, candidate count
    float *d_vreproj = nullptr;        // n errors, then n uint8 inlier flags
    void *d_vwork = nullptr;           // candidates (X / W, observation), point -> candidate map, winner's inlier flags
    void *d_vhyp = nullptr;            // per hypothesis: accumulator (uint64), pose (12 floats, SoA)
    int *d_vcounts = nullptr;          // per hypothesis: inlier count
    size_t cap_vhyps = 0;
    uint32_t view_hyps = 0;            // num_hypotheses of the last registration
    // sfm_adjust_view: allocated at the first call, sized to cap_points (adjust.hip)
    void *d_awork = nullptr;           // per record: observations, start point, compact index; per used record: the same, compacted, and the points
    // sfm_align_pair with this pair as `a`: allocated at the first call (per-record buffer sized to cap_points, per-hypothesis
    // buffer grown on demand) (align.hip)
    void *d_lwork = nullptr;           // key, candidate count; candidates (both points, both observations), record -> candidate map, winner's inlier flags
    void *d_lhyp = nullptr;            // per hypothesis: accumulator (uint64), link (13 floats, SoA)
    size_t cap_lhyps = 0;
    int last_kernel = 0, last_grid = 0, last_block = 0, last_lds = 0;
};

namespace sfm {

// abi.hip
int match_db_rows(const sfm_ctx *ctx, int n2);                    // rows of the second view MatchSiftData visits (SFM_QUIRK_MATCH_TAIL)
// MatchSiftData on SiftPoint records: the first view's match fields, + the index of the best match per point when out_idx is given
int match_records(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2, int *out_idx);
int pose_chain(sfm_pair *pair, int mode, float *d_record);        // sfm_pose_chain + the pair's record on the device

// pairs.hip: the caller's context + auxiliary contexts with streams of their own (sfm_extract_views, sfm_process_pairs)
int lane_contexts(sfm_ctx *ctx, int n, sfm_ctx **out);
int start_lanes_after(sfm_ctx *ctx, sfm_ctx *const *lanes, int n, hipEvent_t event);

// The scoring launchers work on the slot and the stream they are handed: none of them looks up either in the pair or the context.
// ransac.hip.  serial: the call owns slot[0] until the caller's next one (score_shard, sfm_estimate_E), so the pair remembers what the
// slot holds (last_count, cand_*); a call of sfm_ransac_score_into_slot leaves the pair with nothing the plain getters describe.
int launch_ransac_score(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t h0, uint32_t count,
                        unsigned long long *key2 = nullptr, const float *d_E_given = nullptr, bool serial = true);
int launch_ransac_finalize(sfm_pair *pair, const sfm_ransac_params &p, const unsigned long long *d_key, uint32_t hyp_host, bool from_key,
                           hipStream_t stream = nullptr, bool rederive = false);
int launch_permutation_indices(sfm_ctx *ctx, int n, uint32_t seed, int32_t *d_indices);
// ransac_prefilter.hip
bool prefilter_usable(const sfm_pair *pair, const sfm_ransac_params &p, uint32_t count);
int prefilter_pick_rule(sfm_pair *pair, const sfm_ransac_params &p, uint32_t count);   // the rule of this launch (kPfRuleBandTile / kPfRuleBandPack; lab bench: any), kept in pair->pf_rule
int launch_score_prefilter(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t h0, uint32_t count, unsigned long long *key2);
bool prefilter_sums_counts(const sfm_pair *pair, const sfm_ransac_params &p, uint32_t count);          // after prefilter_pick_rule: the launch sums into zeroed counts[], keys from ransac_argmax_counts
int launch_pf_prep(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t count);         // PfRecords from the slot's Ecand (paths whose solve kernel does not write them)
int prefilter_tile_points(const sfm_pair *pair, const sfm_ransac_params &p);      // points per scoring tile of a launch on this pair
int launch_pf_cells(sfm_pair *pair, hipStream_t stream, bool want_sorted = false, int tile = 0);                        // the pair's cell table, (re)built when the points changed
#if SFM_AB
// ab/ransac_prefilter_r2.hip (the round-2 kernel: sfm_ransac_params.reserved[3] == 2)
int launch_score_prefilter_r2(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t h0, uint32_t count, unsigned long long *key2);
// ab/ransac_mfma.hip (SFM_KERNEL_MFMA: E.X on the f32 matrix cores, measured slower)
int launch_score_mfma(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t h0, uint32_t count);
int launch_prefilter_probe(sfm_ctx *ctx, const float *d_E, float thr, float B, const float pt[4], int survive_all, float *d_out);
int launch_prefilter_band_probe(sfm_ctx *ctx, const float *d_E, float thr, float B, const float box[8], int b_safe, const float pt[4], int survive_all, float *d_out);
#endif
// ransac_fused.hip
int launch_ransac_fused(sfm_pair *pair, ShardSlot &slot, hipStream_t stream, const sfm_ransac_params &p, uint32_t h0, uint32_t count);
int launch_finalize_block(sfm_pair *pair, const sfm_ransac_params &p, const unsigned long long *d_key, uint32_t hyp_host, bool from_key,
                          hipStream_t stream, bool rederive);

// pose.hip
int launch_fill_xu(sfm_pair *pair, const sfm_sift_point *d_data);
int launch_set_points(sfm_pair *pair, const float *d_X0, const float *d_X1);
int launch_pose_candidates(sfm_pair *pair, int mode);
int launch_choose_pose(sfm_pair *pair, int mode);
int launch_triangulate(sfm_pair *pair, int mode);
int launch_points_to_vbo(sfm_pair *pair, float *d_positions, float *d_velocities, float scale);
int launch_pair_record(sfm_pair *pair, int mode, float *d_record);
int launch_pose_chain(sfm_pair *pair, float *d_record);          // REFERENCE mode: candidates + choosePose + triangulation (+ record) in one launch

// refine.hip
int launch_refine(sfm_pair *pair, const sfm_refine_params &p);   // start (grid), LM solve (one block), finish (grid)
// the same three stages for many pairs of one context in three launches (grid = pairs); d_masks: null, or one entry per pair (null = its own)
int launch_refine_pairs(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const sfm_refine_params &p, const uint8_t *const *d_masks);
size_t refine_work_bytes(int cap_points);                         // bytes of pair->d_rwork
int refine_state_words();                                         // floats of pair->d_rstate
int refine_pose_offset();                                         // refined P + E inside d_rstate
int refine_report_offset();                                       // sfm_refine_report inside d_rstate

// register.hip
int launch_register(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_register_params &p, const float *d_points, const uint8_t *d_valid);
// the same four stages for many pairs of one context in four launches (grid = pairs); one entry of d_sifts / d_points / d_valid per pair
int launch_register_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts, const sfm_register_params &p,
                          const float *const *d_points, const uint8_t *const *d_valid);
size_t register_work_bytes(int cap_points);                       // bytes of pair->d_vwork
size_t register_hyp_bytes(size_t num_hypotheses);                 // bytes of pair->d_vhyp
int register_state_words();                                       // floats of pair->d_vstate
int register_pose_offset();                                       // refined pose, then the RANSAC pose, inside d_vstate
int register_report_offset();                                     // sfm_register_report inside d_vstate

// view_points.hip: the pair's points over its registered view, one lane per point; d_points / d_valid / d_pose2 / d_pose3 resolved
// by the caller (pose_rows: 3 = [R|t] as R (9) then t (3), 4 = a 4 x 4 row-major matrix as the pair stores its poses)
struct ViewPointsInputs { const sfm_sift_point *sift; const float *points; const uint8_t *valid; const float *pose2, *pose3; int pose_rows; };
int launch_view_points(sfm_pair *pair, const ViewPointsInputs &in, const sfm_view_points_params &p, const sfm_view_points_out &out);
// the same for many pairs of one context in one launch (grid = point blocks x pairs)
int launch_view_points_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const ViewPointsInputs *in, const sfm_view_points_params &p,
                             const sfm_view_points_out *outs);

// adjust.hip: cameras 2 and 3 and the used points adjusted over the pair's three views; d_used2 / d_poses resolved by the caller
// (pose_rows as in ViewPointsInputs)
struct AdjustInputs { const sfm_sift_point *sift; const float *points; const uint8_t *flags, *used2; const float *pose2, *pose3; int pose_rows; };
int launch_adjust(sfm_pair *pair, const AdjustInputs &in, const sfm_adjust_params &p, const sfm_adjust_out &out);      // gather (grid), LM solve (one block), scatter (grid)
// the same three stages for many pairs of one context in three launches
int launch_adjust_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const AdjustInputs *in, const sfm_adjust_params &p, const sfm_adjust_out *outs);
size_t adjust_work_bytes(int cap_points);                         // bytes of pair->d_awork

// align.hip: the similarity that carries pair a's frame into pair b's; points / valid resolved by the caller
struct AlignInputs { const float *points_a; const uint8_t *valid_a; const float *points_b; const uint8_t *valid_b; const int32_t *index; };
int launch_align(sfm_pair *a, sfm_pair *b, const AlignInputs &in, const sfm_align_params &p, const sfm_align_out &out);   // gate, solve, score, refine
// the same four stages for many links of one context in four launches
int launch_align_pairs(sfm_ctx *ctx, sfm_pair *const *as, sfm_pair *const *bs, int num_links, const AlignInputs *in, const sfm_align_params &p,
                       const sfm_align_out *outs);
int launch_align_index(sfm_ctx *ctx, const sfm_sift_point *d_sift, int n, float min_score, float max_ambiguity, int32_t *d_index);
size_t align_work_bytes(int cap_points);                          // bytes of pair->d_lwork
size_t align_hyp_bytes(size_t num_hypotheses);                    // bytes of pair->d_lhyp

// fuse.hip: a chain of aligned pairs fused into tracks and one point per track; pairs: HOST array, every pointer resolved by the
// caller (offset and block0 are filled in here)
struct FusePair;
int launch_fuse_chain(sfm_ctx *ctx, const FusePair *pairs, int num_pairs, const sfm_fuse_params &p, const sfm_fuse_out &out);
// fuse_ring.hip: the same over a closed ring of num_pairs pairs and as many links (pair k - 1 holds the closing one)
int launch_fuse_ring(sfm_ctx *ctx, const FusePair *pairs, int num_pairs, const sfm_fuse_ring_params &p, const sfm_fuse_out &out,
                     sfm_fuse_ring_report *d_report);

// chain_adjust.hip: one bundle adjustment over a fused chain; pairs: HOST array (X0, X1, K, n, ld resolved by the caller)
int launch_adjust_chain(sfm_ctx *ctx, const FusePair *pairs, int num_pairs, const sfm_adjust_chain_in &in, const sfm_adjust_chain_params &p,
                        const sfm_adjust_chain_out &out);
// ring_adjust.hip: the same over a CLOSED ring, one camera per view (the chain's job array and work buffer)
int launch_adjust_ring(sfm_ctx *ctx, const FusePair *pairs, int num_pairs, const sfm_adjust_ring_in &in, const sfm_adjust_ring_params &p,
                       const sfm_adjust_ring_out &out);
// intersect.hip: every track of a fused table intersected under a camera table (the chain's job array and work buffer)
int launch_intersect_tracks(sfm_ctx *ctx, const FusePair *pairs, int num_pairs, const sfm_intersect_in &in, const sfm_intersect_params &p,
                            const sfm_intersect_out &out);

// ring.hip: the drift of a ring measured and spread over its links; links: HOST array, last: pair k - 1 (points, valid, X1, K, n, ld
// resolved by the caller)
struct RingLink;
int launch_close_ring(sfm_ctx *ctx, const RingLink *links, int num_links, const FusePair &last, const sfm_ring_params &p, const sfm_ring_out &out);

// sift.hip
void sift_layout(int width, int height, int num_octaves, int scale_up, sfm_sift_layout *L);
int launch_extract_sift_begin(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height, int pitch,
                              int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up, float *d_temp);
int launch_extract_sift_end(sfm_ctx *ctx, int *num_pts, int *num_stored);
void sift_job_free(sfm_ctx *ctx);
int launch_extract_sift(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height, int pitch,
                        int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up, float *d_temp,
                        int *num_pts, int *num_stored);
// homography.hip
int launch_homography(sfm_ctx *ctx, const sfm_sift_point *d_sift, int n, const int *h_pts, int L, float thresh,
                      float min_score, float max_ambiguity, uint32_t seed, int *num_valid,
                      float h_H[9], int *num_matches, int *h_counts, float *h_homo);
// match.hip
struct MatchJob {                       // one database of a many-matches launch (launch_match_jobs)
    const float *db; int ndb, lddb;     // descriptors of the second view: rows, row stride in floats
    const sfm_sift_point *sift2;        // its records (positions for match_xpos / match_ypos), or null
    sfm_sift_point *sift1;              // first view's records to update in place (MatchSiftData), or null
    int *out_idx;                       // index of the best match per query, or null
    float *ws_best, *ws_second; int *ws_idx; unsigned int *tickets; int rows_per_split, nsplit;      // filled by the launcher
};
int launch_match_jobs(sfm_ctx *ctx, const float *d1, int n1, int ld1, MatchJob *h_jobs, int njobs, int kernel);
int match_pick(const sfm_ctx *ctx, int n1, int n2);
int match_pick_jobs(const sfm_ctx *ctx, int n1, int n2);
int match_partials_workspace(sfm_ctx *ctx, int qblocks, int nsplit, int n1, unsigned int **tickets, float **ws_best, float **ws_second, int **ws_idx);
int match_jobs_workspace(sfm_ctx *ctx, int n1, int qblocks, int rows_unit, int rounds, MatchJob *h_jobs, int njobs, const MatchJob **d_jobs, int *max_split_out);
int launch_match_fused(sfm_ctx *ctx, const float *d1, int n1, int ld1, const float *d2, int n2, int ld2,
                       float *d_best, float *d_second, int32_t *d_index, sfm_sift_point *sift1, const sfm_sift_point *sift2);
int launch_match_fused_jobs(sfm_ctx *ctx, const float *d1, int n1, int ld1, MatchJob *h_jobs, int njobs);
int launch_match_none(sfm_ctx *ctx, int n1, sfm_sift_point *sift1);
int launch_match_prefilter(sfm_ctx *ctx, const float *d1, int n1, int ld1, const float *d2, int n2, int ld2,
                           float *d_best, float *d_second, int32_t *d_index,
                           sfm_sift_point *sift1, const sfm_sift_point *sift2);
int launch_match_ambiguity_quirk(sfm_ctx *ctx, const float *d1, int n1, int ld1, const float *d2, int n2, int ld2, sfm_sift_point *sift1, float *d_second);   // SFM_QUIRK_MATCH_AMBIGUITY
int match_poll_check(sfm_ctx *ctx);                                                // SFM_E_HIP once after a polled merge gave up (match.hip)
int launch_match(sfm_ctx *ctx, const float *d1, int n1, int ld1, const float *d2, int n2, int ld2,
                 float *d_best, float *d_second, int32_t *d_index,
                 sfm_sift_point *sift1, const sfm_sift_point *sift2);
// match_guided.hip: the exact matcher behind the epipolar gate of d_F (ticket merge), and F from a pair's E and K^-1
int launch_match_guided(sfm_ctx *ctx, sfm_sift_point *sift1, int n1, const sfm_sift_point *sift2, int n2, const float *d_F, float band_px);
int launch_pair_fundamental(sfm_pair *pair, int refined, float *d_F);
int launch_pair_fundamentals(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, int refined, float *d_F);

} // namespace sfm
