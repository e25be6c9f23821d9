/*
 * sfm_amd.h -- C ABI of the MI355X-native two-view geometric-estimation path.
 *
 * This is the drop-in boundary for the hot path of Black-Phoenix/CUDA-SfM:
 *     MatchSiftData            (CudaSift/cudaSift.h:42, CudaSift/matching.cu:1090-1206)
 *     SfM::Image_pair::*       (SfM/sfm.h:20-60, SfM/sfm.cu:28-359)
 * The reference has no FFI layer (a C++ class and free functions linked statically,
 * src/main.cpp:282,298-307); the C++ facade in cuda-sfm_amd/host/ keeps those names on top of
 * this ABI, and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns SFM_OK (0) or a negative SFM_E_* code; sfm_last_error() returns a
 *     thread-local description of the last failure (reference convention: print + exit(),
 *     SfM/common.cu:3-15, CudaSift/cudautils.h:15-39 -- the facade can reproduce that).
 *   - pointers named d_* are DEVICE pointers (HIP), h_* are host pointers; plain sizes.
 *   - all matrices are row-major (SfM/common.h:19-20).
 *   - work is enqueued on the context's HIP stream; functions that return host values
 *     synchronise that stream, everything else is asynchronous.
 *   - one context per host thread per device; calls on one context are not re-entrant.
 */
#ifndef SFM_AMD_H
#define SFM_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#pragma GCC visibility push(default)

/* 1: rounds 1-3.  2: sfm_ransac_params.reserved[] must be zero, kernel id 3 and the probe / trace hooks moved to the lab-bench
 * flavour (include/sfm_amd_ab.h, libsfm_amd_ab.so); sfm_ctx_last_pairs_batched added; sfm_amd_comm.h: count-sized feature exchange, sfm_comm_last_exchange.
 * 3: sfm_ctx_retain / sfm_ctx_release and reference-counted contexts (sfm_ctx_destroy on a context that pairs or communicators
 * still point at returns SFM_OK and defers to the last of them; the count is atomic); sfm_ctx_synchronize and sfm_match* report a
 * polled matcher merge that gave up (SFM_E_HIP, once); SFM_QUIRK_MATCH_AMBIGUITY. */
#define SFM_ABI_VERSION 3

#define SFM_OK           0
#define SFM_E_INVALID   (-1)   /* bad argument                                     */
#define SFM_E_HIP       (-2)   /* HIP runtime / launch failure                     */
#define SFM_E_NOMEM     (-3)   /* device allocation failed                         */
#define SFM_E_STATE     (-4)   /* call order violated (e.g. triangulate before E)  */
#define SFM_E_SINGULAR  (-5)   /* singular pose candidate (kernels.h:143-161)      */

/* Feature record, identical layout to the reference's SiftPoint (CudaSift/cudaSift.h:6-22). */
typedef struct sfm_sift_point {
    float xpos, ypos, scale, sharpness, edgeness, orientation;
    float score, ambiguity;
    int32_t match;
    float match_xpos, match_ypos, match_error, subsampling;
    float empty[3];
    float data[128];
} sfm_sift_point;   /* 576 bytes */

typedef struct sfm_ctx  sfm_ctx;    /* device + stream + matcher scratch                      */
typedef struct sfm_pair sfm_pair;   /* state of one SfM::Image_pair (sfm.h:20-60)             */

/* ---- context -------------------------------------------------------------------------------- */
int  sfm_abi_version(void);
const char *sfm_last_error(void);
int  sfm_ctx_create(int device_id, sfm_ctx **out);          /* replaces InitCuda + cuBLAS/cuSOLVER handle setup (sfm.cu:46-75) */
/* Destroys the context -- once nothing points at it any more: every sfm_pair (and every sfm_comm of libsfm_amd_rccl.so) holds a
 * reference, and a context destroyed while some are alive is only marked; the last of them to be destroyed takes it down.  A host
 * language whose finalizers run in no particular order (Python's cyclic collector) can therefore never leave a pair with a
 * dangling context.  sfm_ctx_retain / sfm_ctx_release are that reference count for objects built ON the ABI (the communicator). */
int  sfm_ctx_destroy(sfm_ctx *ctx);
int  sfm_ctx_retain(sfm_ctx *ctx);
int  sfm_ctx_release(sfm_ctx *ctx);
int  sfm_ctx_set_stream(sfm_ctx *ctx, void *hip_stream);    /* NULL = default stream                                          */
/* Behaviours of the reference that the product fixes, selectable for A/B runs against it (SURVEY.md, quirk list):
 * SFM_QUIRK_MATCH_TAIL -- FindMaxCorr10's tile loop (matching.cu:325) never visits the last num_pts2 % 32 points of the
 * second set; with the flag sfm_match searches only the first num_pts2 - num_pts2 % 32 (none: match = -1, score = 0). */
#define SFM_QUIRK_MATCH_TAIL 1u
/* SFM_QUIRK_MATCH_AMBIGUITY -- FindMaxCorr10 keeps eight (best, second) pairs per query, one per group of rows (row mod 32) / 4 of
 * the second set, and its final merge (matching.cu:378-396) compares only their BEST scores with the running pair: the second-best
 * scores of groups 1..7 never enter, so its `ambiguity` = second / (best + 1e-6) is a lower bound of the true ratio (equal for most
 * queries).  FindHomography gates on it (matching.cu:1034-1037).  With the flag sfm_match writes that value into `ambiguity`
 * (sfm_match_soa: into d_second), bit for bit the reference's; score, match and match_xpos / ypos are unchanged.  Costs one extra
 * plain-FMA pass over all pairs (~18 us at 2048 x 2048): for A/B runs against the reference, together with SFM_QUIRK_MATCH_TAIL. */
#define SFM_QUIRK_MATCH_AMBIGUITY 2u
int  sfm_ctx_set_quirks(sfm_ctx *ctx, unsigned int flags);
/* Which matcher sfm_match / sfm_match_soa run (results are bit-identical; A/B runs and tests):
 * SFM_MATCH_EXACT     -- every score as the exact fp32 chain on v_mfma_f32_32x32x2_f32 (match.hip);
 * SFM_MATCH_PREFILTER -- fp16 matrix-core scores select the few rows per query that can be its best or second best, the
 *                        exact chain runs on those only (match_prefilter.hip);
 * SFM_MATCH_FUSED     -- the same idea in ONE launch: the threshold is a running one (the second-largest approximate score seen
 *                        so far), scores, candidate lists and exact chains never leave the block (match_fused.hip);
 * SFM_MATCH_AUTO      -- exact below 2560 x 2560 points, fused up to 6144 x 6144, the pre-filter from there on; the batched path
 *                        of sfm_process_pairs (many matches in one launch) uses fused below that size (default); plain descriptor
 *                        arrays with rows a multiple of 512 bytes apart (sfm_match_soa, ld = 128): exact up to 3400 x 3400, then the
 *                        pre-filter.
 * sfm_ctx_last_match_kernel: what the last call ran. */
#define SFM_MATCH_AUTO      0
#define SFM_MATCH_EXACT     1
#define SFM_MATCH_PREFILTER 2
#define SFM_MATCH_FUSED     3
int  sfm_ctx_set_match_kernel(sfm_ctx *ctx, int kernel);
int  sfm_ctx_last_match_kernel(sfm_ctx *ctx, int *kernel);
/* A stream of the context's own (hipStreamNonBlocking, destroyed with the context): callers without HIP headers get a
 * second context that runs concurrently with the first (which sits on the default stream unless told otherwise). */
int  sfm_ctx_own_stream(sfm_ctx *ctx);
int  sfm_ctx_synchronize(sfm_ctx *ctx);
int  sfm_ctx_get_stream(sfm_ctx *ctx, void **hip_stream);    /* the stream work is enqueued on (for callers that add their own, e.g. RCCL) */
int  sfm_ctx_get_device(sfm_ctx *ctx, int *device_id);
/* HIP-event stopwatch on the context's stream (for callers without their own event API). */
int  sfm_ctx_timer_start(sfm_ctx *ctx);
int  sfm_ctx_timer_stop(sfm_ctx *ctx, float *elapsed_ms);   /* synchronises */
/* Per-kernel stopwatch for the RANSAC launches: when enabled, HIP events are recorded on the
 * context's stream around the solve and score kernels of every sfm_ransac_score / sfm_estimate_E
 * call (up to 256 calls between reads).  sfm_ctx_kernel_timing_read synchronises, returns the summed
 * kernel milliseconds and the number of calls, and resets the counters. */
int  sfm_ctx_kernel_timing(sfm_ctx *ctx, int enable);
int  sfm_ctx_kernel_timing_read(sfm_ctx *ctx, float *solve_ms, float *score_ms, int *calls);

/* Device memory helpers so that a host without HIP bindings (C, Go/cgo, JNI, ctypes ...) can own the
 * buffers the reference allocates with cudaMalloc (InitSiftData, CudaSift/cudaSiftH.cu:234-264).
 * Copies are synchronous with respect to the context's stream. */
int  sfm_device_alloc(sfm_ctx *ctx, size_t bytes, void **d_ptr);
int  sfm_device_free(sfm_ctx *ctx, void *d_ptr);
int  sfm_copy_to_device(sfm_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int  sfm_copy_to_host(sfm_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int  sfm_copy_to_host_2d(sfm_ctx *ctx, void *h_dst, size_t dst_pitch, const void *d_src, size_t src_pitch,
                         size_t width_bytes, size_t height);          /* cudaMemcpy2D of matching.cu:1195-1199 */
int  sfm_copy_to_device_2d(sfm_ctx *ctx, void *d_dst, size_t dst_pitch, const void *h_src, size_t src_pitch,
                           size_t width_bytes, size_t height);        /* CudaImage::Download, cudaImage.cu:59-69 */

/* ---- descriptor match: MatchSiftData (matching.cu:1090-1206, kernel FindMaxCorr10 :301-397) ---
 * For every record of d_sift1: best / second-best dot product over d_sift2 (128-d, fused d-ordered
 * accumulation), lowest index on ties; writes score, match, match_xpos, match_ypos, ambiguity
 * in place.  n1 == 0 or n2 == 0 is a no-op (matching.cu:1095-1096). */
int sfm_match(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2);
/* Same contraction on bare descriptor matrices (row stride ld floats, 16-byte aligned rows);
 * mirrors the layout of the reference's stand-alone benchmark CudaSift/match.cu:916-1081. */
int sfm_match_soa(sfm_ctx *ctx, const float *d_desc1, int n1, int ld1,
                  const float *d_desc2, int n2, int ld2,
                  float *d_best, float *d_second, int32_t *d_index);

/* ---- guided match: the descriptor match restricted to a pair's epipolar band ---------------------
 * For every record of d_sift1: best / second-best dot product (sfm_match's scores, bit for bit) over the rows of d_sift2
 * that pass the gate under d_F, lowest index on ties; writes score, match, match_xpos, match_ypos and ambiguity exactly as
 * sfm_match does (no row in the band: match -1, score 0, positions 0, ambiguity 0).  d_F: 9 DEVICE floats, row-major, in
 * pixel coordinates; a true correspondence has u2^T F u1 = 0 with u1 = (xpos, ypos, 1) of the d_sift1 record (view 1) and
 * u2 = (xpos, ypos, 1) of the d_sift2 record (view 2: what the match leaves in match_xpos / match_ypos); the scale of F
 * does not matter.  A row passes when u2 lies within band_px pixels of the line F u1 AND u1 within band_px pixels of the
 * line F^T u2.  NaN positions, a feature on the epipole, and an F that is zero or not finite pass nothing.
 * The quirk flags and sfm_ctx_set_match_kernel do not apply (sfm_ctx_last_match_kernel keeps its value); n1 == 0 or
 * n2 == 0 is a no-op.  All checks precede the first enqueue: on SFM_E_INVALID (null arguments, negative sizes, band_px not
 * finite or <= 0, non-zero reserved) nothing is written. */
typedef struct sfm_match_guided_params {
    float   band_px;       /* finite, > 0; default 4.0 (the registration's threshold_px) */
    int32_t reserved[4];   /* must be zero (else SFM_E_INVALID)                           */
} sfm_match_guided_params;
void sfm_match_guided_default_params(sfm_match_guided_params *p);
int sfm_match_guided(sfm_ctx *ctx, sfm_sift_point *d_sift1, int n1, const sfm_sift_point *d_sift2, int n2,
                     const float *d_F, const sfm_match_guided_params *p);            /* enqueue only */
/* The fundamental matrix of a pair for sfm_match_guided: F = Kinv^T E Kinv from the pair's own K^-1, transposed so that the
 * pair's OWN records satisfy the convention above -- view 1 (u1) is (xpos, ypos), the side fillXU reads into X0 / U0, view 2
 * (u2) is (match_xpos, match_ypos).  refined = 0: the E of estimateE (needs E); refined = 1: the refined E of
 * sfm_refine_two_view (needs the refinement); SFM_E_STATE otherwise.  Computed in fp64 on the device, scaled to unit
 * Frobenius norm (all zero where E is zero or not finite), rounded once.  Reads the pair, writes d_F (9 DEVICE floats). */
int sfm_pair_fundamental(sfm_pair *pair, int refined, float *d_F);                   /* enqueue only */
/* sfm_pair_fundamental for many pairs of one context in ONE launch: pair i's F at d_F + 9 i, bit-equal to the single call.
 * SFM_E_INVALID for null arguments, num_pairs < 0, refined outside {0, 1}, pairs of different contexts or a pair named twice;
 * SFM_E_STATE for a pair without E (refined = 0) or without the refinement (refined = 1).  All checks precede the first
 * enqueue: nothing is written on a refusal.  Pending pipelined work of the pairs is flushed as the single call flushes it;
 * num_pairs == 0 is a no-op. */
int sfm_pair_fundamentals(sfm_pair *const *pairs, int num_pairs, int refined,
                          float *d_F /* 9 * num_pairs device floats */);             /* enqueue only */
/* sfm_match_guided for a list of jobs in at most two launches: job k leaves in its d_sift1 exactly what
 * sfm_match_guided(ctx, d_sift1, n1, d_sift2, n2, d_F, p) leaves -- the five match fields bit for bit, every other byte of both
 * record arrays untouched.  One band_px serves all jobs.  SFM_E_INVALID for null ctx, jobs or p, num_jobs < 0, a bad band_px or
 * a non-zero reserved word, a job with a negative size, a job with a null pointer whose sizes are both positive, a job whose
 * d_sift1 bytes overlap ANOTHER job's d_sift1, d_sift2 or d_F (two pairs that share a view each hold their own copy of the
 * records they write; within one job the single call's rules hold), and a plan beyond the launch limits (more than 2^31 - 1
 * (job, query block, split) units in a launch, byte counts beyond size_t).  All checks precede the first enqueue and the first
 * device allocation: nothing is written on a refusal.  No C++ exception leaves the call; a failed allocation is SFM_E_NOMEM.
 * num_jobs == 0 is a no-op, and so is a job with n1 == 0 or n2 == 0 inside a list that otherwise runs.  The quirk flags and
 * sfm_ctx_set_match_kernel do not apply; sfm_ctx_last_match_kernel keeps its value. */
typedef struct sfm_match_guided_job {
    sfm_sift_point       *d_sift1; int32_t n1;   /* updated in place, as sfm_match_guided does */
    const sfm_sift_point *d_sift2; int32_t n2;
    const float          *d_F;                   /* 9 device floats, e.g. sfm_pair_fundamentals' d_F + 9 i */
} sfm_match_guided_job;
int sfm_match_guided_pairs(sfm_ctx *ctx, const sfm_match_guided_job *jobs, int num_jobs,
                           const sfm_match_guided_params *p);      /* enqueue only */

/* ---- SIFT extraction: ExtractSift (CudaSift/cudaSiftH.cu:72-232; cudaSift.h:37-39) ---------------------
 * d_image: height x pitch floats on the device (8-bit grey values as float, what CudaImage::Download
 * uploads).  Builds the pyramid (optional 2x upsampling, low pass init_blur, num_octaves levels),
 * finds DoG extrema above thresh with scale >= lowest_scale, assigns one or two orientations and writes
 * xpos, ypos, scale, sharpness, edgeness, orientation, subsampling and the 128-d descriptor of every
 * point into d_sift (other fields untouched).  *num_pts = the count the reference reports
 * (cudaSiftH.cu:123; excludes the finest octave's secondary orientations), *num_stored (optional) =
 * records written, both clipped to max_pts.  Points come coarsest octave first; within an octave in
 * (y, x, scale) order, secondary orientations after them in parent order -- deterministic, unlike the
 * reference's atomic append.  d_temp: sfm_sift_temp_layout(...).total_floats floats, or NULL to use a
 * buffer owned by the context; afterwards it holds every pyramid level and DoG plane at the offsets of
 * the layout.  1 <= num_octaves <= 7.  Synchronous.  When more than max_pts points exist the first
 * max_pts in that order are kept (the reference keeps an arbitrary subset). */
typedef struct {
    int32_t num_octaves;
    int32_t width[8], height[8], pitch[8];   /* level 0 = full (or upsampled) resolution; pitch in floats */
    int64_t image_offset[8];                 /* low-passed image of every level, floats from d_temp */
    int64_t dog_offset[8];                   /* 7 DoG planes (height x pitch each) of every level */
    int64_t up_offset;                       /* upsampled input when scale_up */
    int64_t total_floats;
} sfm_sift_layout;
int sfm_sift_temp_layout(int width, int height, int num_octaves, int scale_up, sfm_sift_layout *layout);
int sfm_extract_sift(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height,
                     int pitch, int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up,
                     float *d_temp, int *num_pts, int *num_stored);
/* ExtractSift in two halves: _begin enqueues the whole extraction on the context's stream and returns at once, _end waits
 * for it and returns the counts (and runs the rare exact second pass when a level overflowed its candidate stash).
 * The per-level kernels of one image do not fill an MI355X: two contexts (two streams) extract two images concurrently
 * -- _begin on both, then _end on both (the dino pair of src/main.cpp:273-274: 0.25 -> 0.15 ms).  One extraction in
 * flight per context; d_sift, d_image and d_temp must stay valid until _end. */
int sfm_extract_sift_begin(sfm_ctx *ctx, sfm_sift_point *d_sift, int max_pts, const float *d_image, int width, int height,
                           int pitch, int num_octaves, double init_blur, float thresh, float lowest_scale, int scale_up,
                           float *d_temp);
int sfm_extract_sift_end(sfm_ctx *ctx, int *num_pts, int *num_stored);

/* ---- homography RANSAC pre-filter: FindHomography (matching.cu:1000-1087) -------------------------
 * 4-point DLT hypotheses from the matched records of d_sift (xpos, ypos -> match_xpos, match_ypos),
 * sampled among the points with score > min_score and ambiguity < max_ambiguity; a point supports a
 * hypothesis when its transfer error is below thresh pixels.  num_loops is rounded up to a multiple of
 * 16 as in the reference.  h_H receives the best homography (row-major 3x3, h33 = 1; identity when
 * fewer than 8 usable points), num_matches its support.  Optional: h_pts = explicit 4 x num_loops host
 * sample (layout pts[k * num_loops + i], as the reference's h_randPts) instead of the seeded sampler;
 * h_counts[num_loops] / h_homo[8 x num_loops] receive every hypothesis (parity tests).  Synchronous. */
int sfm_find_homography(sfm_ctx *ctx, const sfm_sift_point *d_sift, int num_pts, float h_H[9], int *num_matches,
                        int num_loops, float min_score, float max_ambiguity, float thresh, uint32_t seed,
                        const int32_t *h_pts, int32_t *h_counts, float *h_homo);

/* ---- Image_pair ------------------------------------------------------------------------------ */
/* Image_pair::Image_pair(k, k_inv, image_count, num_points), sfm.cu:28-78.  h_K / h_Kinv: host. */
int sfm_pair_create(sfm_ctx *ctx, const float h_K[9], const float h_Kinv[9],
                    int image_count, int num_points, sfm_pair **out);
int sfm_pair_destroy(sfm_pair *pair);                                      /* sfm.cu:346-359 */
/* Re-use an Image_pair for another correspondence set of at most its creation-time size: no allocation, no
 * synchronisation (the reference constructs one Image_pair per image pair, main.cpp:298 -- ~20 cudaMalloc/cudaFree
 * each; a many-pairs driver creates one at the largest size and resets it). */
int sfm_pair_reset(sfm_pair *pair, int num_points);

/* Image_pair::fillXU(SiftPoint *data), sfm.cu:80-92 (+ copy_point kernels.h:261-279). */
int sfm_fill_xu(sfm_pair *pair, const sfm_sift_point *d_data);
/* Bypass for callers that already hold normalised coordinates: 3 x num_points row-major each. */
int sfm_set_points(sfm_pair *pair, const float *d_X0, const float *d_X1);

#define SFM_KERNEL_AUTO   0
#define SFM_KERNEL_SPLIT  1   /* solve: one hypothesis per lane; score: one hypothesis per wavefront */
#define SFM_KERNEL_FUSED  2   /* everything one hypothesis per wavefront in LDS                      */
                              /* 3: not in this library (a recorded A/B variant, include/sfm_amd_ab.h) -> SFM_E_INVALID */
#define SFM_KERNEL_PREFILTER 4 /* lane solve; scoring: fp16-split matrix-core pre-filter (32 hypotheses x 32 points per  */
                              /* MFMA tile) rejects the pairs that cannot be inliers, the exact test runs on the rest; */
                              /* needs z == 1 points (fillXU) and 1e-9 <= threshold <= 1e-2, else SFM_KERNEL_SPLIT runs */

typedef struct sfm_ransac_params {
    uint32_t num_hypotheses;  /* H: global hypothesis count (reference: N/8, sfm.cu:95)                 */
    uint32_t hyp_begin;       /* shard [hyp_begin, hyp_begin + hyp_count) scored by this call           */
    uint32_t hyp_count;       /* 0 = all of [hyp_begin, H)                                              */
    uint32_t seed;            /* keyed sampler seed (used when d_indices == NULL)                       */
    const int32_t *d_indices; /* optional device int32[8*H]: explicit 8-tuples, global hypothesis order */
    float    threshold;       /* inlier iff residual < threshold; reference 1e-6 (sfm.cu:220)           */
    int32_t  jacobi_sweeps;   /* null vector of the 8x9 system: 0 (default) = Householder QR of A^T;       */
                              /* k > 0 = normal equations A^T A + k sweeps of 9x9 Jacobi (7 converges)    */
    int32_t  kernel;          /* SFM_KERNEL_*                                                           */
    int32_t  reserved[4];     /* must be zero (anything else: SFM_E_INVALID)                            */
} sfm_ransac_params;

void sfm_ransac_default_params(sfm_ransac_params *p, int num_points);
/* Reference-mode sampler (sfm.cu:97-106, Q2): H = n/8 disjoint 8-tuples of one seeded permutation.
 * Writes int32[8*(n/8)] to d_indices (device). */
int sfm_ransac_permutation_indices(sfm_ctx *ctx, int num_points, uint32_t seed, int32_t *d_indices);

/* Image_pair::estimateE(), sfm.cu:94-153: score all hypotheses of the shard, arg-max (first
 * maximum, thrust::max_element semantics without the off-by-one of sfm.cu:137), winner's E and
 * inlier mask.  No host synchronisation. */
int sfm_estimate_E(sfm_pair *pair, const sfm_ransac_params *p);
/* estimateE for a STREAM of calls (many pairs, repeated estimates): step k runs on slot k % 2 -- a stream and a set of
 * per-shard buffers of its own -- so consecutive calls overlap on the device (the lane-solve kernel and the launch gaps
 * of one call fill what the scoring kernel of the other leaves idle: 851 -> 815 us per call at 2^20 hypotheses,
 * 155 -> 119 us at 131072; profiles/overlap_probe.py).  E, mask and best are those of the last call once
 * sfm_pair_flush has made the context stream wait for it; every other entry point that works on the pair (the sfm_get_*
 * readers, sfm_fill_xu, sfm_set_points, the pose stages, sfm_ransac_score / _finalize, sfm_estimate_E) flushes by itself. */
int sfm_estimate_E_pipelined(sfm_pair *pair, const sfm_ransac_params *p);
int sfm_pair_flush(sfm_pair *pair);
/* The same in two steps for multi-GPU use: score the local shard (device key = (count << 32) |
 * (0xFFFFFFFF - hyp), 0 if the shard is empty), exchange keys with one all-reduce(max), then
 * finalize the winning hypothesis id on every rank. */
int sfm_ransac_score(sfm_pair *pair, const sfm_ransac_params *p);
int sfm_ransac_finalize(sfm_pair *pair, const sfm_ransac_params *p, uint32_t hyp);
/* calculateInliers on its own (sfm.cu:155-236 takes the E candidates as its input): scores hyp_count caller-supplied
 * candidates (d_E: 9 floats each, row-major, DEVICE memory; candidate k has hypothesis id hyp_begin + k) instead of
 * solving them from 8-tuples.  Leaves the counts (sfm_get_inlier_counts), the candidates (sfm_get_E_candidates) and
 * the packed key (sfm_get_key).  The finalize calls (sfm_ransac_finalize, sfm_ransac_finalize_key) return SFM_E_STATE
 * after this call: they take the winner's E from the scored candidates where this rank holds it and re-derive it from the
 * hypothesis' 8-tuple elsewhere, which is only the same matrix when the candidates came from tuples. */
int sfm_ransac_score_candidates(sfm_pair *pair, const sfm_ransac_params *p, const float *d_E);
/* Device-resident variants: copy the local key into caller memory (e.g. the tensor handed to the
 * RCCL all-reduce) and finalize from a reduced key without any host round trip. */
int sfm_ransac_export_key(sfm_pair *pair, uint64_t *d_key_out);
/* sfm_ransac_score that also leaves the shard's key in caller memory (the 8 bytes handed to the all-reduce): the scoring
 * blocks write both copies, so the multi-GPU step needs no export in between. */
int sfm_ransac_score_into(sfm_pair *pair, const sfm_ransac_params *p, uint64_t *d_key_out);
int sfm_ransac_finalize_key(sfm_pair *pair, const sfm_ransac_params *p, const uint64_t *d_key);
/* sfm_ransac_score_into on one of TWO sets of per-shard buffers (slot 0 = the pair's usual ones, slot 1 = a second set,
 * allocated on first use) and on the given stream of the same device (NULL = the context's): consecutive shards -- of the
 * same pair or of a stream of calls -- can then be in flight together (one's lane-solve kernel fills the tail and the
 * launch gaps of the other's scoring kernel: 155 -> 119 us per 131072-hypothesis shard, profiles/overlap_probe.py).
 * The caller orders the streams and re-uses a slot only after its key has been consumed; sfm_get_inlier_counts /
 * sfm_get_E_candidates do not describe slot shards. */
int sfm_ransac_score_into_slot(sfm_pair *pair, const sfm_ransac_params *p, uint64_t *d_key_out, int slot, void *hip_stream);
/* sfm_ransac_finalize_key enqueued on ANOTHER stream of the same device (NULL = the context's): for callers that overlap
 * pair k's exchange + finalize with pair k+1's scoring (sfm_amd_comm.h, sfm_estimate_E_sharded_pipelined).  The winner's E
 * is always re-derived from the hypothesis id (bit-identical to the scored candidate), never read from the candidate
 * buffer the next score call is rewriting.  The caller orders the streams (events); the getters synchronise the context
 * stream only. */
int sfm_ransac_finalize_key_on(sfm_pair *pair, const sfm_ransac_params *p, const uint64_t *d_key, void *hip_stream);

/* Image_pair::computePosecandidates(), sfm.cu:238-252 + candidate_kernels kernels.h:357-385. */
#define SFM_POSE_REFERENCE 0   /* as written in the reference (quirks Q7, Q8, Q9, Q11 of SURVEY.md) */
#define SFM_POSE_CORRECT   1   /* textbook decomposition, majority-vote cheirality                  */
int sfm_pose_candidates(sfm_pair *pair, int mode);
/* Image_pair::choosePose(), sfm.cu:254-307. */
int sfm_choose_pose(sfm_pair *pair, int mode);
/* Image_pair::linear_triangulation(), sfm.cu:309-344. */
int sfm_triangulate(sfm_pair *pair, int mode);
/* The three calls above as the caller issues them (src/main.cpp:302-306: computePosecandidates, choosePose,
 * linear_triangulation) in ONE launch for SFM_POSE_REFERENCE -- the choosePose chain and the triangulation of every point
 * against all four candidates run side by side, results bit-identical to the three calls; SFM_POSE_CORRECT (majority
 * vote over all points before the choice) runs the three launches.  sfm_process_pairs uses it per pair. */
int sfm_pose_chain(sfm_pair *pair, int mode);

/* ---- two-view bundle adjustment after estimateE --------------------------------------------------
 * Levenberg-Marquardt over camera 2's pose (camera 1 = [I|0], |t| = 1: 5 degrees of freedom) and the 3-D point of every used
 * correspondence; residuals are pixel reprojection errors K2x2 (pi(X) - x / z) of both views (K2x2 = [[fx, s], [0, fy]] of the
 * pair's K) under a Huber loss.  Start: the SFM_POSE_CORRECT candidates of the pair's E, the one most masked points see in
 * front of both cameras (first maximum), the masked points triangulated against it exactly as sfm_triangulate(CORRECT) does;
 * a masked point is used when that start point is finite and in front of both cameras.  sfm_refine_two_view only enqueues
 * (flushes the pair first); the getters synchronise.  Nothing estimateE or the pose stages wrote changes. */
#define SFM_REFINE_CONVERGED  0    /* the relative decrease of the cost fell below min_rel_decrease                     */
#define SFM_REFINE_MAX_ITER   1    /* max_iterations reached, or lambda grew beyond 1e16                                 */
#define SFM_REFINE_DEGENERATE 2    /* fewer than 16 used points: the start pose and the start points are returned          */
typedef struct sfm_refine_params {
    int32_t  max_iterations;    /* LM iterations, accepted + rejected, 0..200 (0 = start only); default 20                */
    float    huber_px;          /* Huber threshold on each view's 2-D pixel residual; 0 = plain LS; default 1.0          */
    float    min_rel_decrease;  /* stop when (cost_prev - cost) / cost_prev < this; default 1e-6                          */
    float    initial_lambda;    /* Marquardt damping, diagonal scaled by (1 + lambda); default 1e-3                       */
    const uint8_t *d_mask;      /* optional DEVICE uint8[num_points]: points to use; NULL = last estimateE's inlier mask   */
    int32_t  reserved[4];       /* must be zero (else SFM_E_INVALID)                                                     */
} sfm_refine_params;
void sfm_refine_default_params(sfm_refine_params *p);

typedef struct sfm_refine_report {
    int32_t status;             /* SFM_REFINE_*                                                                          */
    int32_t iterations, accepted;
    int32_t num_used;           /* masked points that passed the cheirality test at the start                            */
    int32_t pose_index;         /* SFM_POSE_CORRECT candidate (0..3) chosen by the start vote                            */
    float   initial_rms_px, final_rms_px;   /* sqrt(sum of squared pixel residuals / (4 num_used)), no Huber weighting   */
    float   final_cost;         /* robust cost at the end                                                                */
    float   lambda;
} sfm_refine_report;

int sfm_refine_two_view(sfm_pair *pair, const sfm_refine_params *p);              /* enqueue only */
/* The same refinement for many pairs of ONE context in three launches (grid = pairs) on its stream: afterwards every pair is
 * exactly as after sfm_refine_two_view(pair, p) with its mask -- bit for bit, whatever the order of the list -- and the getters
 * and SFM_BUF_REFINED_* / SFM_BUF_REPROJ serve it per pair.  pairs: HOST array of num_pairs (0..65535) handles, none listed
 * twice; p: one parameter set for all of them, p->d_mask must be NULL; d_masks: optional HOST array of num_pairs DEVICE
 * pointers (NULL, or a NULL entry: that pair's estimateE inlier mask).  Every check precedes the first launch: SFM_E_INVALID
 * (arguments) or SFM_E_STATE (the text names the first pair without a current E) leave every pair as it was. */
int sfm_refine_pairs(sfm_pair *const *pairs, int num_pairs, const sfm_refine_params *p,
                     const uint8_t *const *d_masks);                              /* enqueue only */
int sfm_get_refine_report(sfm_pair *pair, sfm_refine_report *r);                   /* synchronises */
/* [R|t; 0 0 0 1] (X2 = R X1 + t, |t| = 1) and E = [t]x R, row-major */
int sfm_get_refined_pose(sfm_pair *pair, float h_P[16], float h_E[9]);
/* 4 x num_points (X, Y, Z, 1) in camera 1's frame: used points refined, every other point triangulated (sfm_triangulate's
 * DLT) against the refined pose */
int sfm_get_refined_points(sfm_pair *pair, float *h_points);
/* h_err[num_points]: the larger of the two views' pixel errors under the refined pose (+inf behind a camera);
 * h_used (optional) uint8[num_points]: 1 for the points the solve used */
int sfm_get_reprojection_errors(sfm_pair *pair, float *h_err, uint8_t *h_used);

/* ---- registering a further view against the pair's 3-D points ------------------------------------
 * One more view gets a pose X3 = R3 X + t3 in the pair's gauge (camera 1 = [I|0], the pair's |t| = 1 fixes the scale: |t3| is
 * NOT normalised) from 2-D / 3-D correspondences: P3P RANSAC (Lambda Twist on a 4-point sample, one hypothesis per lane), then
 * Levenberg-Marquardt over the 6 pose parameters on the winner's inliers, Huber loss on the pixel residual.  Every view shares
 * the pair's K.
 * Correspondences: the pair's point i is feature record i of view 1 (as in fillXU); d_sift holds view 1's records re-matched
 * against the new view (sfm_match(ctx, d_sift1, n1, d_sift3, n3)).  Record i is a candidate when match >= 0,
 * score > min_score, ambiguity < max_ambiguity and point i is usable (finite, W != 0, Z / W > 0, and its valid flag set); its
 * observation is K^-1 (match_xpos, match_ypos, 1), dehomogenised.
 * 3-D points: d_points NULL = the pair's refined points where the refinement's used flag is 1 (SFM_E_STATE unless
 * sfm_refine_two_view ran on the current points); else the caller's DEVICE 4 x num_points (camera-1 frame) and optional
 * uint8 d_valid[num_points].
 * Inlier test, shared by the scoring kernel and the final mask: Y = R3 X + t3 in fp32, (x, y) the observation, inlier iff Y.z > 0
 * and (fx (Y.x - x Y.z) + s (Y.y - y Y.z))^2 + (fy (Y.y - y Y.z))^2 < (threshold_px Y.z)^2, no division, no contraction.
 * Fewer than 4 candidates or a winner with fewer than 6 inliers: status SFM_REFINE_DEGENERATE (not an error), the winner's pose
 * unrefined ([I|0] if no sample gave one), zero masks.  sfm_register_view only enqueues (flushes the pair first); the getters
 * synchronise.  Nothing estimateE, the pose stages or the refinement wrote changes. */
typedef struct sfm_register_params {
    uint32_t num_hypotheses;    /* 1..2^20, default 4096                                                               */
    uint32_t seed;              /* sampler seed (sample4: the hash sampler of sample8), default 0x5EED5F3D              */
    float    threshold_px;      /* inlier iff the pixel reprojection error is below this (test above), default 4.0      */
    float    min_score, max_ambiguity;      /* candidate gate, defaults 0.85 / 0.95 (sfm_find_homography's)             */
    int32_t  max_iterations;    /* pose LM, accepted + rejected, 0..200 (0 = RANSAC winner only), default 10           */
    float    huber_px;          /* Huber threshold on the 2-D pixel residual; 0 = plain LS; default 1.0               */
    float    min_rel_decrease;  /* stop when (cost_prev - cost) / cost_prev < this; default 1e-6                         */
    float    initial_lambda;    /* Marquardt damping, diagonal scaled by (1 + lambda); default 1e-3                      */
    const float   *d_points;    /* optional DEVICE 4 x num_points; NULL = refined points + the refinement's used flags   */
    const uint8_t *d_valid;     /* optional DEVICE uint8[num_points] with d_points (NULL: every point)                   */
    int32_t  reserved[4];       /* must be zero (else SFM_E_INVALID)                                                    */
} sfm_register_params;
void sfm_register_default_params(sfm_register_params *p);

typedef struct sfm_register_report {
    int32_t  status;            /* SFM_REFINE_CONVERGED / _MAX_ITER / _DEGENERATE                                      */
    int32_t  num_candidates;    /* records that passed the gate                                                        */
    int32_t  ransac_inliers;    /* the winner's count: the points the LM runs over                                     */
    int32_t  num_inliers;       /* final mask: candidates that pass the inlier test under the refined pose             */
    uint32_t best_hypothesis;   /* first maximum of the counts                                                         */
    int32_t  iterations, accepted;
    float    initial_rms_px, final_rms_px;  /* sqrt(sum of squared pixel residuals / (2 ransac_inliers)) over the winner's
                                               inliers, at the winner's and at the refined pose; no Huber weighting      */
    float    final_cost;        /* robust cost at the end                                                              */
    float    lambda;
} sfm_register_report;

int sfm_register_view(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_register_params *p);   /* enqueue only */
/* The same registration for many pairs of ONE context in four launches (grid = pairs) on its stream: afterwards every pair is
 * exactly as after sfm_register_view with the same parameters and its own d_sift / points / valid -- bit for bit, wherever it
 * stands in the list -- and the getters and SFM_BUF_VIEW_* serve it per pair.  pairs: HOST array of num_pairs (0..65535)
 * handles, none listed twice (a pair holds one registered view); d_sifts: HOST array of num_pairs DEVICE pointers, d_sifts[i] =
 * view 1's records of pair i re-matched against that pair's new view (the same pointer may serve several pairs); p: one
 * parameter set for all of them, p->d_points and p->d_valid must be NULL; d_points, d_valid: optional HOST arrays of num_pairs
 * DEVICE pointers (d_points NULL, or a NULL entry: that pair's refined points and the refinement's used flags; d_valid[i]
 * without d_points[i] is SFM_E_INVALID).  Every check precedes the first launch: SFM_E_INVALID (arguments) or SFM_E_STATE (the
 * text names the first pair without the stage it needs) leave every pair as it was. */
int sfm_register_views(sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts, const sfm_register_params *p,
                       const float *const *d_points, const uint8_t *const *d_valid);   /* enqueue only */
int sfm_get_register_report(sfm_pair *pair, sfm_register_report *r);                               /* synchronises */
/* refined [R3|t3; 0 0 0 1] and the RANSAC winner's, row-major; either pointer may be NULL */
int sfm_get_view_pose(sfm_pair *pair, float h_P[16], float h_P_ransac[16]);
/* h_err[num_points]: pixel error under the refined pose, +inf for non-candidates and behind the camera; h_inlier (optional)
 * uint8[num_points]: the final inlier mask */
int sfm_get_view_errors(sfm_pair *pair, float *h_err, uint8_t *h_inlier);
/* the inlier count of every hypothesis of the last registration (num_hypotheses int32) */
int sfm_get_view_counts(sfm_pair *pair, int32_t *h_counts);

/* ---- triangulating and refining the pair's points over its registered view ------------------------
 * The intersection step behind the resection: with the cameras [I|0], [R|t] and [R3|t3] fixed, every record of view 1 that the
 * new view sees (match >= 0, score > min_score, ambiguity < max_ambiguity: the registration's gate) gets a point from all the
 * views that have one.  A record whose input point is usable (the registration's point test) starts at X / W and is refined over
 * views 1, 2 and 3; one without a usable point -- a wrong match in view 2 -- is triangulated from views 1 and 3 (the DLT of
 * sfm_triangulate) and refined over those two.  The refinement is a Levenberg-Marquardt on the three point coordinates, Huber
 * loss on the pixel residuals, fp32, one lane per point.  A result is accepted when every view used passes the registration's
 * inlier test at threshold_px (in front of the camera included) and, for a new point, the rays of cameras 1 and 3 subtend at
 * least min_parallax_deg; otherwise the input column is kept.
 * The call READS the pair and writes only the caller's buffers: no stage, buffer id or getter belongs to it, every SFM_BUF_* is
 * the same afterwards.  Observations: views 1 and 2 from the pair's X0 / X1 (dehomogenised), view 3 as K^-1 (match_xpos,
 * match_ypos, 1) of d_sift (sfm_register_view's records).  d_sift must be 16-byte aligned (SFM_E_INVALID otherwise): a record's
 * fields are read with one 8-byte and one 16-byte load; every device allocation is. */
#define SFM_VP_UNSEEN        0   /* view 3 does not see the record: input column copied, err = +inf                       */
#define SFM_VP_NEW           1   /* no usable input point: triangulated from views 1 and 3, refined, accepted             */
#define SFM_VP_REFINED       2   /* usable input point refined over views 1, 2 and 3, accepted                            */
#define SFM_VP_NEW_REJECTED  3   /* as SFM_VP_NEW, but the result failed the acceptance test: input column copied         */
#define SFM_VP_KEPT          4   /* as SFM_VP_REFINED, but the result failed the test (view 3 disagrees): input column copied */
typedef struct sfm_view_points_params {
    float   threshold_px;              /* acceptance: the registration's inlier test, default 4.0                          */
    float   min_score, max_ambiguity;  /* the gate on view 3's match, defaults 0.85 / 0.95                                 */
    float   min_parallax_deg;          /* SFM_VP_NEW only: angle between the rays of cameras 1 and 3; 0..90, default 1.0   */
    int32_t max_iterations;            /* point LM, accepted + rejected, 0..50 (0 = start point only), default 5           */
    float   huber_px, min_rel_decrease, initial_lambda;   /* as sfm_register_params; 1.0 / 1e-6 / 1e-3                     */
    const float   *d_points;           /* optional DEVICE 4 x num_points; NULL = refined points + the refinement's used flags */
    const uint8_t *d_valid;            /* optional DEVICE uint8[num_points], only with d_points (NULL: every point)        */
    const float   *d_poses;            /* optional DEVICE float[24]: [R|t] of camera 2, then of camera 3, each row-major R (9)
                                          then t (3); NULL = the refined pose and the registered view's refined pose        */
    int32_t reserved[4];               /* must be zero (else SFM_E_INVALID)                                                */
} sfm_view_points_params;
typedef struct sfm_view_points_out {   /* DEVICE buffers of the caller; none may overlap an input or a buffer of the pair  */
    float   *d_points;                 /* 4 x num_points, required: (X, Y, Z, 1) for SFM_VP_NEW / _REFINED, else the input column */
    uint8_t *d_flags;                  /* num_points, required: SFM_VP_*                                                    */
    float   *d_err;                    /* num_points, optional: the largest pixel error over the views used, at the point that
                                          was attempted (also for the rejected classes; +inf where there is none)           */
    int32_t *d_counts;                 /* 8, optional: [0..4] the number of points per class, [5..7] zero                    */
} sfm_view_points_out;
void sfm_view_points_default_params(sfm_view_points_params *p);
/* Needs points; the refinement unless d_points AND d_poses are given; the registration unless d_poses is given (SFM_E_STATE). */
int sfm_triangulate_view(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_view_points_params *p,
                         const sfm_view_points_out *out);                                          /* enqueue only */
/* The same for many pairs of ONE context in one launch: every outs[i] ends byte for byte as after sfm_triangulate_view on
 * pairs[i].  pairs, d_sifts, outs: HOST arrays of num_pairs (0..65535) entries, no pair twice; p: one parameter set,
 * p->d_points, p->d_valid and p->d_poses must be NULL, so every pair needs its refinement and its registration.  Every check
 * precedes the launch: on SFM_E_INVALID / SFM_E_STATE (the text names the first offending pair) nothing is written. */
int sfm_triangulate_views(sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts,
                          const sfm_view_points_params *p, const sfm_view_points_out *outs);     /* enqueue only */

/* ---- adjusting both cameras and all points over the pair's three views ---------------------------
 * A Levenberg-Marquardt bundle adjustment over views 1, 2 and the registered view: camera 1 stays [I|0]; camera 2 moves with the
 * two-view refinement's 5 degrees of freedom (R <- exp([w]x) R, t on the unit sphere, which fixes the scale); camera 3 with the
 * registration's 6 (R3 <- exp([w]x) R3, t3 <- t3 + dt); and the 3-D point of every used record.  Residuals (pixels), Huber loss,
 * damping, accept test and stop rules are sfm_refine_two_view's.  in->d_points / in->d_flags are what sfm_triangulate_view wrote
 * (SFM_VP_*), in->d_sift the same records (16-byte aligned).  View 3 sees a record whose flag is NEW or REFINED; view 2 sees it
 * when its used2 flag is set and the flag is UNSEEN, REFINED or KEPT; view 1 always.  A record is used when view 2 or 3 sees it,
 * its input column passes the registration's point test and X / W lies in front of every camera that sees it at the start poses.
 * Fewer than 16 records in view 2 or fewer than 6 in view 3: SFM_REFINE_DEGENERATE -- the start poses and the input columns are
 * returned with d_views filled; not an error.
 * The call READS the pair and writes only the caller's buffers: no stage, buffer id or getter belongs to it. */
typedef struct sfm_adjust_params {
    int32_t max_iterations;            /* 0..200, 0 = evaluate the start only; default 20                                   */
    float   huber_px, min_rel_decrease, initial_lambda;   /* 1.0 / 1e-6 / 1e-3, as sfm_refine_params                        */
    const uint8_t *d_used2;            /* optional DEVICE uint8[num_points]: records with an observation in view 2; NULL = the
                                          two-view refinement's used flags (needs the refinement)                           */
    const float   *d_poses;            /* optional DEVICE float[24], layout of sfm_view_points_params.d_poses: the start; NULL =
                                          the refined pose and the registered view's refined pose                           */
    int32_t reserved[4];               /* must be zero (else SFM_E_INVALID)                                                */
} sfm_adjust_params;
typedef struct sfm_adjust_in {         /* DEVICE, all required */
    const sfm_sift_point *d_sift;      /* view 1's records re-matched against view 3, 16-byte aligned                       */
    const float   *d_points;           /* 4 x num_points: sfm_view_points_out.d_points                                      */
    const uint8_t *d_flags;            /* num_points: sfm_view_points_out.d_flags                                           */
} sfm_adjust_in;
typedef struct sfm_adjust_report {
    int32_t status;                    /* SFM_REFINE_*                                                                      */
    int32_t iterations, accepted;
    int32_t num_points, num_view2, num_view3;    /* used records; those view 2 / view 3 sees                                */
    float   initial_rms_px, final_rms_px;        /* sqrt(sum of squares / (2 (num_points + num_view2 + num_view3)))         */
    float   final_cost, lambda;
} sfm_adjust_report;
typedef struct sfm_adjust_out {        /* DEVICE buffers of the caller; none may overlap an input or another output          */
    float   *d_poses;                  /* 24, required: adjusted [R|t] of cameras 2 and 3, the layout d_poses accepts        */
    float   *d_points;                 /* 4 x num_points, required: (X, Y, Z, 1) for used records, the input column otherwise */
    uint8_t *d_views;                  /* num_points, required: bit 0 / 1 / 2 = views 1 / 2 / 3 used, 0 = record not used    */
    float   *d_err;                    /* num_points, optional: the largest pixel error over the record's views at the final
                                          state, +inf where unused                                                          */
    sfm_adjust_report *d_report;       /* required, DEVICE                                                                   */
} sfm_adjust_out;
void sfm_adjust_default_params(sfm_adjust_params *p);
/* Needs points; the refinement unless d_used2 AND d_poses are given; the registration unless d_poses is given (SFM_E_STATE). */
int sfm_adjust_view(sfm_pair *pair, const sfm_adjust_in *in, const sfm_adjust_params *p, const sfm_adjust_out *out);   /* enqueue only */
/* The same for many pairs of ONE context in three launches: every outs[i] ends byte for byte as after sfm_adjust_view on
 * pairs[i].  pairs, ins, outs: HOST arrays of num_pairs (0..65535) entries, no pair twice; p->d_used2 and p->d_poses must be
 * NULL.  Every check precedes the launches: on SFM_E_INVALID / SFM_E_STATE (the text names the first offending pair) nothing
 * is written. */
int sfm_adjust_views(sfm_pair *const *pairs, int num_pairs, const sfm_adjust_in *ins, const sfm_adjust_params *p,
                     const sfm_adjust_out *outs);                                                     /* enqueue only */

/* ---- aligning two overlapping pairs: the similarity between their frames -------------------------
 * Pair A = (view i, view i+1) and pair B = (view i+1, view i+2) each live in their own gauge (camera 1 = [I|0], |t| = 1).  A
 * link is (s, R, t), s > 0, with X_B = s R X_A + t: with exact data R and t / s are A's camera-2 pose and s the ratio of the two
 * gauges.  Correspondences: point j of A is record j of view i; d_index[j] is the index of the same feature among view i+1's
 * records, which is B's point index (sfm_align_index_from_matches builds it from A's records), or any value outside
 * [0, num_points of B) for none.  Record j is a candidate when d_index[j] is in range and both points are usable (the
 * registration's point test: finite, W != 0, Z / W > 0, valid flag set).
 * 3-point RANSAC (orthonormal triads of the sample in both frames, one hypothesis per lane), then Levenberg-Marquardt over 7
 * parameters (R <- exp([w]x) R, t <- t + dt, s <- s exp(dsigma)) on the winner's inliers, Huber loss per residual pair.
 * Residuals and the inlier test are pixels, never 3-D distances: forward, Y = s R X_A + t against B's view-1 observation (B's X0,
 * dehomogenised) through B's K; backward, Z = R^T (X_B - t) against A's view-1 observation through A's K.  A candidate is an
 * inlier iff both pass sfm_register_view's division-free test at threshold_px (in front of the camera included); scoring, the
 * LM's point set and the final mask share it.
 * Fewer than 3 candidates or a winner with fewer than 6 inliers: status SFM_REFINE_DEGENERATE (not an error), the winner's link
 * unrefined (the identity, s = 1, if no sample gave one), zero masks.
 * The calls READ both pairs and write only the caller's buffers: no stage, buffer id or getter belongs to them. */
typedef struct sfm_align_params {
    uint32_t num_hypotheses;    /* 1..2^20, default 4096                                                               */
    uint32_t seed;              /* sampler seed, default 0x5EED5F3D                                                     */
    float    threshold_px;      /* both pixel errors below this (test above), default 4.0                               */
    int32_t  max_iterations;    /* LM, accepted + rejected, 0..200 (0 = RANSAC winner only), default 10                 */
    float    huber_px, min_rel_decrease, initial_lambda;   /* as sfm_register_params; 1.0 / 1e-6 / 1e-3                 */
    const float   *d_points_a;  /* optional DEVICE 4 x num_points of A; NULL = A's refined points + the refinement's used flags */
    const uint8_t *d_valid_a;   /* optional DEVICE uint8[num_points of A], only with d_points_a (NULL: every point)     */
    const float   *d_points_b;  /* the same for B                                                                       */
    const uint8_t *d_valid_b;
    int32_t  reserved[4];       /* must be zero (else SFM_E_INVALID)                                                    */
} sfm_align_params;
typedef struct sfm_align_report {
    int32_t  status;            /* SFM_REFINE_CONVERGED / _MAX_ITER / _DEGENERATE                                      */
    int32_t  num_candidates;    /* records that passed the gate                                                        */
    int32_t  ransac_inliers;    /* the winner's count: the candidates the LM runs over                                 */
    int32_t  num_inliers;       /* final mask: candidates that pass the test under the refined link                    */
    uint32_t best_hypothesis;   /* first maximum of the counts                                                         */
    int32_t  iterations, accepted;
    float    initial_rms_px, final_rms_px;  /* sqrt(sum of squared pixel residuals / (4 ransac_inliers)) over the winner's
                                               inliers, both directions, at the winner's and at the refined link        */
    float    final_cost;        /* robust cost at the end                                                              */
    float    lambda;
} sfm_align_report;
typedef struct sfm_align_out {  /* DEVICE buffers of the caller; none may overlap an input or another output            */
    float   *d_sim;             /* 26, required: s, R (9, row-major), t (3) refined, then the RANSAC winner's           */
    uint8_t *d_inlier;          /* num_points of A, required: the final mask                                            */
    float   *d_err;             /* num_points of A, optional: the larger of the two pixel errors under the refined link,
                                   +inf for non-candidates and behind a camera                                          */
    int32_t *d_counts;          /* num_hypotheses, optional: every hypothesis' inlier count                             */
    sfm_align_report *d_report; /* required, DEVICE                                                                     */
} sfm_align_out;
void sfm_align_default_params(sfm_align_params *p);
/* d_index[j] = match of record j where match >= 0, score > min_score and ambiguity < max_ambiguity (the registration's gate),
 * else -1.  d_sift: DEVICE, n records of A's first view matched against A's second view; enqueue only. */
int sfm_align_index_from_matches(sfm_ctx *ctx, const sfm_sift_point *d_sift, int n, float min_score, float max_ambiguity,
                                 int32_t *d_index);
/* Needs, in both pairs: points; the refinement unless that side's d_points_* is given (SFM_E_STATE).  a and b belong to one
 * context, a != b.  d_index: DEVICE int32[num_points of A].  The work buffer belongs to pair a. */
int sfm_align_pair(sfm_pair *a, sfm_pair *b, const int32_t *d_index, const sfm_align_params *p, const sfm_align_out *out);   /* enqueue only */
/* The same for many links of ONE context in four launches: every outs[i] ends byte for byte as after
 * sfm_align_pair(as[i], bs[i], d_indices[i], p, &outs[i]), wherever the link stands in the list.  as, bs, d_indices, outs: HOST
 * arrays of num_links (0..65535) entries; the overrides in p must be NULL.  No pair may be listed twice as `a` (its work buffer
 * serves one link); a pair may be `a` of one link and `b` of another.  No output may overlap an input, another output, or a
 * buffer of another link.  Every check precedes the launches: on SFM_E_INVALID / SFM_E_STATE (the text names the first offending
 * link as links[i]) nothing is written. */
int sfm_align_pairs(sfm_pair *const *as, sfm_pair *const *bs, int num_links, const int32_t *const *d_indices,
                    const sfm_align_params *p, const sfm_align_out *outs);                           /* enqueue only */

/* ---- fusing a chain of aligned pairs: tracks and one point per track ------------------------------
 * Pairs 0 .. k-1, pair i = (view i, view i + 1), and the k - 1 links between neighbours (what sfm_align_pairs took and gave).
 * A link is valid when its report's status is not SFM_REFINE_DEGENERATE, its 13 floats are finite and s > 0; an invalid link
 * cuts the chain: pair i + 1 starts a new segment whose root frame is its own, and no track crosses the cut.  d_frames carries
 * every pair into its segment's root frame (the links' inverses composed in fp64 along the chain, rounded once), d_cams holds
 * both cameras of every pair in that frame.
 * Node (i, j) = record j of pair i, live when its point is usable (the registration's point test).  Record j of pair i is joined
 * to record d_index[j] of pair i + 1 when the link is valid, d_inlier[j] != 0, the index is in range, d_err[j] is finite and
 * both nodes are live; where several records name the same target, the smallest d_err wins, then the lowest record.  The
 * tracks are the resulting paths, numbered by their first node (by pair, then by record).  A track over pairs i .. i + L - 1
 * has L + 1 observations ordered by view: the X0 column of its record in each pair (slot 0), then the X1 column of its last
 * record (slot 1).  Its point starts at the mean of its pairs' points in the root frame and is refined by sfm_triangulate_view's
 * point Levenberg-Marquardt over all its views; it is stored when every view passes sfm_register_view's inlier test at
 * threshold_px, else the start point is.
 * The call READS the pairs and writes only the caller's buffers: no stage, buffer id or getter belongs to it.  Integer atomics
 * only: two calls give the same bytes. */
#define SFM_FUSE_REFINED 1   /* the LM result passed the test in every view of the track: stored                   */
#define SFM_FUSE_KEPT    2   /* it failed in some view: the start point (above) is stored                          */
typedef struct sfm_fuse_params {
    float   threshold_px;                                 /* acceptance, the registration's inlier test; default 4.0 */
    int32_t max_iterations;                               /* point LM, accepted + rejected, 0..50; default 5         */
    float   huber_px, min_rel_decrease, initial_lambda;   /* 1.0 / 1e-6 / 1e-3                                        */
    int32_t reserved[4];                                  /* must be zero (else SFM_E_INVALID)                        */
} sfm_fuse_params;
typedef struct sfm_fuse_pair_in {      /* HOST array, one per pair; pair i = (view i, view i + 1)                    */
    sfm_pair      *pair;
    const float   *d_points;           /* optional DEVICE 4 x n_i; NULL = refined points + the refinement's used flags */
    const uint8_t *d_valid;            /* optional, only with d_points (NULL: every point)                            */
    const float   *d_pose;             /* optional DEVICE float[12], R row-major then t: camera 2; NULL = refined pose */
} sfm_fuse_pair_in;
typedef struct sfm_fuse_link_in {      /* HOST array, one per link i: pair i -> pair i + 1; all DEVICE, all required  */
    const int32_t *d_index;            /* what sfm_align_pairs took                                                   */
    const float   *d_sim;              /* first 13 floats of sfm_align_out.d_sim                                      */
    const uint8_t *d_inlier;           /* sfm_align_out.d_inlier                                                      */
    const float   *d_err;              /* sfm_align_out.d_err                                                         */
    const sfm_align_report *d_report;
} sfm_fuse_link_in;
typedef struct sfm_fuse_out {          /* DEVICE buffers of the caller, N = sum of n_i; all required unless marked    */
    float   *d_frames;     /* 13 x k: (s, R, t) carrying pair i's frame into its segment's root frame                 */
    int32_t *d_root;       /* k: the first pair of pair i's segment                                                   */
    float   *d_cams;       /* 24 x k: [R|t] (R 9 row-major, t 3) of pair i's camera 1, then camera 2, in the root frame */
    int32_t *d_track;      /* N: track of node (pair i, record j) at offset(i) + j, -1 = none                         */
    int32_t *d_track_offset;   /* N + 1: CSR offsets, entries [0 .. T] written                                        */
    int32_t *d_obs_cam;    /* 2N: per observation 2 * pair + (0 | 1): the slot of d_cams                              */
    int32_t *d_obs_record; /* 2N: the record of that pair whose X0 (slot 0) or X1 (slot 1) column is the observation  */
    float   *d_points;     /* 4 x N, leading dimension N: column t = (X, Y, Z, 1) of track t in its segment's root frame */
    uint8_t *d_flags;      /* N: SFM_FUSE_* per track                                                                 */
    float   *d_err;        /* N, optional: largest pixel error over the track's views at the LM result                */
    int32_t *d_counts;     /* 8: tracks T, observations M, REFINED, KEPT, segments, longest track (views), 0, 0       */
} sfm_fuse_out;
void sfm_fuse_default_params(sfm_fuse_params *p);
/* pairs: HOST array of num_pairs (0..4096) entries, N at most 2^26; links: HOST array of num_pairs - 1 entries (may be NULL for
 * fewer than two pairs).  Zero pairs is SFM_OK and writes nothing.  Every pair belongs to ctx and is listed once; each needs
 * points, and the refinement unless both d_points and d_pose are given (SFM_E_STATE).  No output may overlap an input or another
 * output.  Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names pairs[i] or links[i]) nothing
 * is written.  The work buffers belong to the context. */
int  sfm_fuse_chain(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const sfm_fuse_link_in *links,
                    const sfm_fuse_params *p, const sfm_fuse_out *out);          /* enqueue only */

/* ---- one bundle adjustment over a fused chain: every camera and every track together --------------
 * Reads the pairs and what sfm_fuse_chain wrote for them.  One unknown camera per pair p: its camera 2 (view p + 1), started at
 * slot 2p + 1 of d_cams.  Camera 1 of pair p is the segment's fixed [I|0] where d_root[p] == p and the camera 2 of pair p - 1
 * otherwise (slot 2p of d_cams is not read for such a pair): one camera per view.  Per segment the root pair's camera moves with
 * sfm_refine_two_view's 5 degrees of freedom (t on the unit sphere, the start t normalised), every other camera with
 * sfm_register_view's 6.  Segments are independent Levenberg-Marquardt problems with a report each.
 * A track is used when its flag EQUALS SFM_FUSE_REFINED (a ring's seam tracks, SFM_FUSE_SEAM_*, are therefore not: their views
 * are not consecutive; sfm_adjust_ring uses them), it has at most max_track_views views, its point is finite and lies in front
 * of every one of its views under the start cameras; an unused track returns its input column.  A segment whose root camera
 * has fewer than 16 used observations, or any other camera fewer than 6, is SFM_REFINE_DEGENERATE (not an error): its cameras
 * (both input slots) and its tracks' columns are returned as they came in.
 * Residuals are pixels through the observing pair's K, Huber per view.  The reduced camera system is block-banded (a track's
 * views are consecutive) and solved by a banded Cholesky in fp64.  No float atomics: two calls give the same bytes.
 * The call READS the pairs and writes only the caller's buffers: no stage, buffer id or getter belongs to it. */
typedef struct sfm_adjust_chain_params {
    int32_t max_iterations;                               /* accepted + rejected, 0..50; default 10                    */
    float   huber_px, min_rel_decrease, initial_lambda;   /* 1.0 / 1e-6 / 1e-3                                          */
    int32_t max_track_views;                              /* W, 2..16; default 8: longer tracks are not used            */
    int32_t reserved[4];                                  /* must be zero (else SFM_E_INVALID)                          */
} sfm_adjust_chain_params;
typedef struct sfm_adjust_chain_in {   /* pairs: HOST array; the rest DEVICE, what sfm_fuse_out holds; all required   */
    sfm_pair *const *pairs;
    const int32_t *d_root;             /* k                                                                           */
    const float   *d_cams;             /* 24 x k                                                                      */
    const int32_t *d_track_offset;     /* N + 1                                                                       */
    const int32_t *d_obs_cam;          /* 2N                                                                          */
    const int32_t *d_obs_record;       /* 2N                                                                          */
    const float   *d_points;           /* 4 x N                                                                       */
    const uint8_t *d_flags;            /* N                                                                           */
    const int32_t *d_counts;           /* 8                                                                           */
} sfm_adjust_chain_in;
typedef struct sfm_adjust_chain_report {   /* entry p: all zero but `root` unless p is its segment's root             */
    int32_t root;                      /* the first pair of pair p's segment                                          */
    int32_t status;                    /* SFM_REFINE_*                                                                */
    int32_t iterations, accepted;
    int32_t num_cameras;               /* pairs of the segment                                                        */
    int32_t num_tracks, num_observations;      /* used tracks and their observations                                  */
    int32_t num_over_long;             /* tracks of the segment with more than max_track_views views                  */
    float   initial_rms_px, final_rms_px;      /* sqrt(sum of squares / (2 num_observations))                         */
    float   final_cost, lambda;
} sfm_adjust_chain_report;
typedef struct sfm_adjust_chain_out {  /* DEVICE buffers of the caller; all required unless marked                    */
    float   *d_cams;       /* 24 x k, the layout of sfm_fuse_out.d_cams: inside a segment camera 1 of pair p + 1 is the
                              bytes of camera 2 of pair p                                                             */
    float   *d_points;     /* 4 x N, leading dimension N                                                              */
    uint8_t *d_used;       /* N: 1 = the track was used                                                               */
    float   *d_err;        /* N, optional: the largest pixel error over the track's views under the final cameras,
                              +inf behind a camera; written for every track                                           */
    sfm_adjust_chain_report *d_reports;    /* k                                                                       */
} sfm_adjust_chain_out;
void sfm_adjust_chain_default_params(sfm_adjust_chain_params *p);
/* num_pairs 0..4096, N (the pairs' records in all) at most 2^26.  Zero pairs is SFM_OK and writes nothing.  Every pair belongs
 * to ctx, is listed once and needs its normalised observations and K (the points stage).  No output may overlap an input or
 * another output.  Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names pairs[i]) nothing is
 * written.  The work buffer belongs to the context. */
int  sfm_adjust_chain(sfm_ctx *ctx, const sfm_adjust_chain_in *in, int num_pairs, const sfm_adjust_chain_params *p,
                      const sfm_adjust_chain_out *out);                          /* enqueue only */

/* ---- closing a ring of aligned pairs: the drift measured and spread over the links -----------------
 * Pairs 0 .. k-1 of a ring, pair i = (view i, view i + 1 mod k), and ALL k links: link i carries pair i's frame into pair
 * (i + 1 mod k)'s, so link k - 1 is the closing one (what sfm_align_pairs gives for a = pair k - 1, b = pair 0).  The open frames
 * are sfm_fuse_chain's: F_0 = I, F_{i+1} = F_i o L_i^-1 in fp64; the drift D = F_k is the identity for a perfect ring.
 * status: SFM_RING_OPEN when some link is invalid (sfm_fuse_chain's rule), SFM_RING_REJECTED when all are valid but D's rotation
 * angle exceeds max_rotation_rad or |ln s_D| exceeds max_log_scale (gates against a wrong closing link; none on t, whose length
 * follows the gauge), else SFM_RING_CLOSED.
 * CLOSED: with (sigma, w, t_c) = (ln s, axis-angle, t) of D^-1 and alpha_0 = 0 <= alpha_1 <= ... <= alpha_k = 1 the running sums of
 * the normalised weights (1 / max(num_inliers_i, 1) from the links' reports, or `weights`), B_i = (exp(alpha_i sigma),
 * exp(alpha_i [w]x), alpha_i t_c), B_k = D^-1 itself; d_frames holds the closed frames F'_i = B_i o F_i and d_links the corrected
 * links L'_i = F'_{i+1}^-1 o F'_i, all in fp64 and rounded once.  F'_k = I: the corrected links compose to the identity, and their
 * first k - 1 go unchanged into sfm_fuse_chain.  OPEN / REJECTED: d_links is the input bit for bit, d_frames is byte for byte what
 * sfm_fuse_chain writes for the first k - 1 links (an invalid link restarts at the identity); drift_* are 0 when OPEN.
 * The seam: view 0 is the second view of pair k - 1.  Every usable record of pair k - 1 (the registration's point test) is carried
 * into pair 0's frame by the measured closing link, by the open frame F_{k-1} and by the closed frame F'_{k-1} (= the open one
 * unless CLOSED) and held against its own X1 observation through the pair's K under [I|0] (sfm_register_view's inlier test and
 * error at threshold_px).  seam_count: the records that pass under the measured link; seam_rms_*_px: the rms pixel error over
 * them under each frame, without the members whose error there is not finite -- seam_lost_* count those.
 * The call READS the pair and writes only the caller's buffers: no stage, buffer id or getter belongs to it.  No float atomics:
 * two calls give the same bytes. */
#define SFM_RING_CLOSED   0
#define SFM_RING_OPEN     1
#define SFM_RING_REJECTED 2
typedef struct sfm_ring_params {
    float   threshold_px;              /* the seam's inlier test; default 4.0                                         */
    float   max_rotation_rad;          /* in (0, pi/2]; default 0.35                                                  */
    float   max_log_scale;             /* > 0; default ln 2                                                           */
    const float *weights;              /* optional HOST float[k]: finite, >= 0, positive sum; NULL = from the reports */
    int32_t reserved[4];               /* must be zero (else SFM_E_INVALID)                                           */
} sfm_ring_params;
typedef struct sfm_ring_link_in {      /* HOST array, one per link i: pair i -> pair i + 1 mod k; DEVICE, required    */
    const float *d_sim;                /* first 13 floats of sfm_align_out.d_sim                                      */
    const sfm_align_report *d_report;
} sfm_ring_link_in;
typedef struct sfm_ring_report {
    int32_t status;                    /* SFM_RING_*                                                                  */
    int32_t num_links;
    int32_t first_invalid;             /* the first invalid link, -1 = none                                           */
    float   drift_log_scale, drift_rotation_rad, drift_t;   /* ln s, rotation angle and |t| of D                      */
    int32_t seam_count, seam_lost_open, seam_lost_closed;
    float   seam_rms_link_px, seam_rms_open_px, seam_rms_closed_px;
} sfm_ring_report;
typedef struct sfm_ring_out {          /* DEVICE buffers of the caller; all required unless marked                    */
    float   *d_links;      /* 13 x k: the corrected links                                                             */
    float   *d_frames;     /* 13 x k: the closed frames (the layout of sfm_fuse_out.d_frames)                         */
    float   *d_seam_err;   /* 3 x n of pair k - 1, optional: pixel error per record under the link, the open and the
                              closed frame; +inf where the record is not usable or the point lies behind the camera   */
    sfm_ring_report *d_report;
} sfm_ring_out;
void sfm_ring_default_params(sfm_ring_params *p);
/* links: HOST array of num_links (3..4096) entries.  last_pair: pair k - 1 with sfm_fuse_chain's overrides (d_pose is not read);
 * it belongs to ctx and needs points, and the refinement unless d_points is given (SFM_E_STATE).  No output may overlap an input
 * or another output.  Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names links[i] or
 * last_pair) nothing is written.  The work buffer belongs to the context. */
int  sfm_close_ring(sfm_ctx *ctx, const sfm_ring_link_in *links, int num_links, const sfm_fuse_pair_in *last_pair,
                    const sfm_ring_params *p, const sfm_ring_out *out);          /* enqueue only */

/* ---- fusing a closed ring: sfm_fuse_chain over k pairs and k links, the seam joined ---------------
 * Pairs 0 .. k-1 of a ring, pair i = (view i, view i + 1 mod k), and ALL k links in sfm_fuse_link_in form: link k - 1 is what
 * sfm_align_pairs took and gave for a = pair k - 1, b = pair 0; d_sim normally points into sfm_ring_out.d_links.
 * The chain part is sfm_fuse_chain's over the k pairs and the first k - 1 links: d_frames, d_root and d_cams are byte for byte
 * what it writes, and its paths are the CHAIN TRACKS.  status: SFM_RING_OPEN when one of the k links is invalid (first_invalid
 * names it); else D = the stored fp32 frame of pair k - 1 composed with the inverse of link k - 1 in fp64, and SFM_RING_REJECTED
 * when D's rotation angle exceeds max_closure_rotation_rad or |ln s_D| exceeds max_closure_log_scale (no gate on t, whose length
 * follows the gauge), else SFM_RING_CLOSED.  closure_*: ln s, the angle and |t| of D, zeros when OPEN.  Not CLOSED: every buffer
 * of sfm_fuse_out ends byte for byte as sfm_fuse_chain leaves it; only the report differs.
 * CLOSED, the seam: record j of pair k - 1 proposes to join node (0, m), m = d_index[j] of link k - 1, under sfm_fuse_chain's
 * edge test.  With A the chain track that ends in (k - 1, j), h_A its head's pair, and B the chain track headed by (0, m) over
 * len(B) pairs, the proposal is ELIGIBLE when len(B) < h_A: the joined track then sees every view at most once (views h_A ..
 * k - 1, view 0 through pair 0's X0, views 1 .. len(B)).  Eligibility comes before the contest: among the eligible proposers of
 * one target the smallest d_err wins, then the lowest record; an ineligible one never blocks an eligible one.  The winner's
 * track goes on into B: (0, m) is a head no more, B's nodes take A's track number, the joined track has len(A) + len(B) pairs and
 * one observation more: the X0 column of each record in path order, then the X1 column of B's last record (A's own slot-1
 * observation of view 0 gives way to pair 0's slot 0).  It follows that a feature followed through all k pairs back to its own
 * record (A = B, h_A = 0) stays one chain track with view 0 at both ends; a track crosses the seam at most once; no track has
 * more than k pairs; no walk can cycle; tracks stay numbered by their head (pair, then record).
 * Points and flags are sfm_fuse_chain's, but a track that crosses the seam (its first observation's pair is larger than its
 * last's) is flagged SFM_FUSE_SEAM_REFINED / SFM_FUSE_SEAM_KEPT; d_counts[2] / [3] count 1 + 3 and 2 + 4.  sfm_adjust_chain uses
 * a track only when its flag EQUALS SFM_FUSE_REFINED, so seam tracks stay out of its banded system (whose views must be
 * consecutive) and come back as they went in: the ring's table may be handed to it as it is.  sfm_adjust_ring (below) is the
 * adjustment that uses them, with one camera for view 0.
 * The call READS the pairs and writes only the caller's buffers: no stage, buffer id or getter belongs to it.  Integer atomics
 * only: two calls give the same bytes. */
#define SFM_FUSE_SEAM_REFINED 3   /* SFM_FUSE_REFINED of a track that crosses the seam of a ring                     */
#define SFM_FUSE_SEAM_KEPT    4   /* SFM_FUSE_KEPT of such a track                                                   */
typedef struct sfm_fuse_ring_params {
    sfm_fuse_params fuse;
    float   max_closure_rotation_rad;  /* in (0, pi/2]; default 1e-3                                                  */
    float   max_closure_log_scale;     /* > 0; default 1e-3                                                           */
    int32_t reserved[4];               /* must be zero (else SFM_E_INVALID)                                           */
} sfm_fuse_ring_params;
typedef struct sfm_fuse_ring_report {
    int32_t status, first_invalid;     /* SFM_RING_*; the first invalid link, -1 = none                               */
    float   closure_log_scale, closure_rotation_rad, closure_t;     /* ln s, rotation angle and |t| of D              */
    int32_t seam_proposals;            /* records of pair k - 1 that pass the edge test                               */
    int32_t seam_ineligible;           /* of them: len(B) >= h_A                                                      */
    int32_t seam_tracks;               /* joins = tracks that cross the seam                                          */
    int32_t seam_refined, seam_kept;   /* of them by flag                                                             */
} sfm_fuse_ring_report;
void sfm_fuse_ring_default_params(sfm_fuse_ring_params *p);
/* pairs: HOST array of num_pairs (3..4096) entries, N at most 2^26; links: HOST array of num_pairs entries, every field
 * required; d_report: DEVICE, required.  The contract is sfm_fuse_chain's: every pair belongs to ctx and is listed once; each
 * needs points, and the refinement unless both d_points and d_pose are given (SFM_E_STATE).  No output (d_report included) may
 * overlap an input or another output.  Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names
 * pairs[i] or links[i]) nothing is written.  The work buffers belong to the context. */
int  sfm_fuse_ring(sfm_ctx *ctx, const sfm_fuse_pair_in *pairs, int num_pairs, const sfm_fuse_link_in *links,
                   const sfm_fuse_ring_params *p, const sfm_fuse_out *out, sfm_fuse_ring_report *d_report);   /* enqueue only */

/* ---- one bundle adjustment over a closed ring: one camera per view, the seam tracks used ----------
 * Reads the k pairs of a ring (3..4096), what sfm_fuse_ring wrote for them and its report.  An observation with d_obs_cam = c is
 * of view ((c >> 1) + (c & 1)) mod k.  View 0 is the fixed [I|0] whichever pair observes it (pair 0's camera 1, pair k - 1's camera
 * 2, both ends of a track followed round the whole ring); view v >= 1 is unknown camera v - 1, started at slot 2 (v - 1) + 1 of
 * d_cams: k - 1 cameras.  Camera 0 (view 1) moves with sfm_refine_two_view's 5 degrees of freedom (t on the unit sphere, the
 * start t normalised), every other camera with sfm_register_view's 6.  Slot 2 (k - 1) + 1 of d_cams is not read; d_root is required
 * and swept for overlaps like the rest of the table, but not read (a CLOSED ring has one root).
 * A track is used when its flag is SFM_FUSE_REFINED or SFM_FUSE_SEAM_REFINED, it has at most max_track_views views, its point is
 * finite and lies in front of every one of its views under the start cameras; an unused track returns its input column.  When
 * camera 0 has fewer than 16 used observations, or any other camera fewer than 6, the status is SFM_REFINE_DEGENERATE (not an
 * error): all 24 k camera floats and all columns are returned as they came in.
 * Residuals are pixels through the observing pair's K, Huber per view, as in sfm_adjust_chain.  The reduced camera system is
 * cyclic-banded (a band and two corners); the cameras are taken in the order 0, k - 2, 1, k - 3, ..., in which it is block-banded
 * with min(2 max_track_views, k - 1) block diagonals, and solved by sfm_adjust_chain's banded Cholesky in fp64.
 * d_ring_report->status != SFM_RING_CLOSED: nothing is adjusted.  Cameras and columns are returned as they came in, d_used is all
 * zero, and the report holds ring_status and zeros.  Use sfm_adjust_chain on such a table: pair k - 1's second camera must not be
 * taken for view 0 when the closure was rejected.  The status is read on the device; the launches are the same.
 * The call READS the pairs and writes only the caller's buffers: no stage, buffer id or getter belongs to it.  No float atomics:
 * two calls give the same bytes. */
typedef struct sfm_adjust_ring_params {
    int32_t max_iterations;                               /* accepted + rejected, 0..50; default 10                    */
    float   huber_px, min_rel_decrease, initial_lambda;   /* 1.0 / 1e-6 / 1e-3                                          */
    int32_t max_track_views;                              /* W, 2..16; default 8: longer tracks are not used            */
    int32_t reserved[4];                                  /* must be zero (else SFM_E_INVALID)                          */
} sfm_adjust_ring_params;
typedef struct sfm_adjust_ring_in {    /* pairs: HOST array; the rest DEVICE, what sfm_fuse_ring wrote; all required  */
    sfm_pair *const *pairs;
    const int32_t *d_root;             /* k                                                                           */
    const float   *d_cams;             /* 24 x k                                                                      */
    const int32_t *d_track_offset;     /* N + 1                                                                       */
    const int32_t *d_obs_cam;          /* 2N                                                                          */
    const int32_t *d_obs_record;       /* 2N                                                                          */
    const float   *d_points;           /* 4 x N                                                                       */
    const uint8_t *d_flags;            /* N                                                                           */
    const int32_t *d_counts;           /* 8                                                                           */
    const sfm_fuse_ring_report *d_ring_report;
} sfm_adjust_ring_in;
typedef struct sfm_adjust_ring_report {
    int32_t ring_status;               /* SFM_RING_* of d_ring_report; the rest is zero unless it is SFM_RING_CLOSED  */
    int32_t status;                    /* SFM_REFINE_*                                                                */
    int32_t iterations, accepted;
    int32_t num_cameras;               /* k - 1                                                                       */
    int32_t num_tracks;                /* used tracks                                                                 */
    int32_t num_seam_tracks;           /* of them: SFM_FUSE_SEAM_REFINED                                              */
    int32_t num_observations;          /* the used tracks' observations                                               */
    int32_t num_over_long;             /* tracks with more than max_track_views views                                 */
    float   initial_rms_px, final_rms_px;      /* sqrt(sum of squares / (2 num_observations))                         */
    float   final_cost, lambda;
} sfm_adjust_ring_report;
typedef struct sfm_adjust_ring_out {   /* DEVICE buffers of the caller; all required unless marked                    */
    float   *d_cams;       /* 24 x k, the layout of sfm_fuse_out.d_cams: camera 1 of pair p + 1 is the bytes of camera 2 of
                              pair p, camera 1 of pair 0 is its input slot, camera 2 of pair k - 1 is the bytes of camera 1
                              of pair 0                                                                                */
    float   *d_points;     /* 4 x N, leading dimension N                                                              */
    uint8_t *d_used;       /* N: 1 = the track was used                                                               */
    float   *d_err;        /* N, optional: the largest pixel error over the track's views under the returned cameras,
                              +inf behind a camera; written for every track                                           */
    sfm_adjust_ring_report *d_report;
} sfm_adjust_ring_out;
void sfm_adjust_ring_default_params(sfm_adjust_ring_params *p);
/* num_pairs 3..4096, N (the pairs' records in all) at most 2^26.  Every pair belongs to ctx, is listed once and needs its
 * normalised observations and K (the points stage).  No output may overlap an input (d_ring_report included) or another output.
 * Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names pairs[i]) nothing is written.  The work
 * buffer belongs to the context. */
int  sfm_adjust_ring(sfm_ctx *ctx, const sfm_adjust_ring_in *in, int num_pairs, const sfm_adjust_ring_params *p,
                     const sfm_adjust_ring_out *out);                            /* enqueue only */

/* ---- every track of a fused table intersected again under a given camera table --------------------
 * Reads the pairs, a track table in sfm_fuse_out's layout (a chain, a chain with cuts or a ring) and ANY camera table in that
 * layout -- sfm_fuse_chain's, sfm_adjust_chain's or sfm_adjust_ring's: slot d_obs_cam[o] of d_cams holds the camera of
 * observation o.  An adjustment moves every camera and rewrites only the columns of the tracks it used; this call brings the
 * others (KEPT, SEAM_KEPT, over-long, seam tracks after sfm_adjust_chain, tracks that started behind a camera) into the same frame.
 * Per track t < T = d_counts[0] (the others are not touched):
 *   copied through -- its flag is not 1..4, it has fewer than two views, or d_skip[t] != 0: column and flag as they came in, d_err
 *     the largest pixel error over its views under d_cams at that column (+inf behind a camera: sfm_adjust_chain's rule).  With
 *     d_skip = sfm_adjust_*_out.d_used the jointly adjusted points stay.
 *   else two start candidates: C, the input column X / W, and L, the linear intersection of the views' rays (per view the rows
 *     (x r3 - r1) X = t1 - x t3 and (y r3 - r2) X = t2 - y t3; the 3 x 3 normal equations in fp64 in list order; a singular system
 *     gives no L).  A candidate is eligible when it is finite and in front of every view.  The start is the eligible candidate with
 *     the smaller robust cost, C on a tie; with none the column and flag come back as they came in and d_err is +inf.
 *   from the start sfm_fuse_chain's point Levenberg-Marquardt over all views and its acceptance test at threshold_px: accepted, the
 *     result is stored with SFM_FUSE_REFINED (SFM_FUSE_SEAM_REFINED where the input flag was 3 or 4), else the START with the KEPT
 *     flag of the same class; d_err is the largest pixel error at the LM result.
 * Tracks of at least wave_min_views views are intersected by one wavefront each, the others by one lane each; the bytes written do
 * not depend on that split.  The call READS the pairs and writes only the caller's buffers: no stage, buffer id or getter belongs
 * to it.  Integer atomics only: two calls give the same bytes. */
typedef struct sfm_intersect_params {
    float   threshold_px;                                 /* acceptance, the registration's inlier test; default 4.0 */
    int32_t max_iterations;                               /* point LM, accepted + rejected, 0..50; default 5         */
    float   huber_px, min_rel_decrease, initial_lambda;   /* 1.0 / 1e-6 / 1e-3                                        */
    int32_t wave_min_views;                               /* 0 = the library's default (32), else 2..INT32_MAX: a pure
                                                             performance knob                                         */
    int32_t reserved[4];                                  /* must be zero (else SFM_E_INVALID)                        */
} sfm_intersect_params;
typedef struct sfm_intersect_in {      /* pairs: HOST array; the rest DEVICE, in sfm_fuse_out's layout; all required unless marked */
    sfm_pair *const *pairs;
    const float   *d_cams;             /* 24 x k                                                                      */
    const int32_t *d_track_offset;     /* N + 1                                                                       */
    const int32_t *d_obs_cam;          /* 2N                                                                          */
    const int32_t *d_obs_record;       /* 2N                                                                          */
    const float   *d_points;           /* 4 x N, leading dimension N                                                  */
    const uint8_t *d_flags;            /* N                                                                           */
    const int32_t *d_counts;           /* 8: [0] = T and [1] = M are read, on the device                              */
    const uint8_t *d_skip;             /* N, optional: != 0 = the track is copied through                             */
} sfm_intersect_in;
typedef struct sfm_intersect_out {     /* DEVICE buffers of the caller; all required unless marked                    */
    float   *d_points;     /* 4 x N, leading dimension N                                                              */
    uint8_t *d_flags;      /* N                                                                                       */
    float   *d_err;        /* N, optional                                                                             */
    int32_t *d_counts;     /* 8: T, re-intersected, REFINED + SEAM_REFINED, KEPT + SEAM_KEPT (both of the re-intersected),
                              copied through, started from L, without an eligible start, promoted (KEPT class in, REFINED
                              class out)                                                                              */
} sfm_intersect_out;
void sfm_intersect_default_params(sfm_intersect_params *p);
/* num_pairs 0..4096, N (the pairs' records in all) at most 2^26.  Zero pairs is SFM_OK and writes nothing.  Every pair belongs
 * to ctx, is listed once and needs its normalised observations and K (the points stage).  No output may overlap an input (d_skip
 * included) or another output.  Every check precedes the first enqueue: on SFM_E_INVALID / SFM_E_STATE (the text names pairs[i])
 * nothing is written.  The table is trusted as sfm_adjust_chain trusts it.  The work buffer belongs to the context. */
int  sfm_intersect_tracks(sfm_ctx *ctx, const sfm_intersect_in *in, int num_pairs, const sfm_intersect_params *p,
                          const sfm_intersect_out *out);                         /* enqueue only */

/* ---- accessors (the reference keeps these private; needed for parity checks) ------------------ */
#define SFM_BUF_X0      0   /* float 3 x ld   normalised coords image 1 (ld = sfm_pair_ld)   */
#define SFM_BUF_X1      1
#define SFM_BUF_U0      2   /* float 3 x ld   pixel coords                                    */
#define SFM_BUF_U1      3
#define SFM_BUF_E       4   /* float 9                                                        */
#define SFM_BUF_P       5   /* float 4 x 16   candidates                                      */
#define SFM_BUF_PINV    6   /* float 4 x 16   inverses                                        */
#define SFM_BUF_POINTS  7   /* float 4 x num_points                                           */
#define SFM_BUF_COUNTS  8   /* int32 hyp_count of the last score call                         */
#define SFM_BUF_MASK    9   /* uint8 num_points                                               */
#define SFM_BUF_KEY     10  /* uint64 packed best key of the last score call                  */
#define SFM_BUF_ECAND   11  /* float 9 x hyp_count of the last score call                     */
#define SFM_BUF_PIND    12  /* int32 chosen pose index                                        */
#define SFM_BUF_REFINED_POSE   13  /* float 16 + 9  refined [R|t; 0 0 0 1], then E (sfm_refine_two_view)   */
#define SFM_BUF_REFINED_POINTS 14  /* float 4 x num_points                                          */
#define SFM_BUF_REPROJ         15  /* float num_points errors (px), then uint8 num_points used flags  */
#define SFM_BUF_VIEW_POSE      16  /* float 16 + 16  refined [R3|t3; 0 0 0 1], then the RANSAC winner's (sfm_register_view) */
#define SFM_BUF_VIEW_COUNTS    17  /* int32 num_hypotheses: per-hypothesis inlier counts             */
#define SFM_BUF_VIEW_REPROJ    18  /* float num_points errors (px), then uint8 num_points inlier flags */
/* SFM_BUF_REFINED_*, SFM_BUF_REPROJ: NULL and 0 bytes until sfm_refine_two_view has run on the current points (after a
 * fillXU, set_points or reset, as the getters' SFM_E_STATE); SFM_BUF_VIEW_* likewise until sfm_register_view has run */
int sfm_pair_device_ptr(sfm_pair *pair, int which, void **d_ptr, size_t *bytes);
int sfm_pair_ld(const sfm_pair *pair);                 /* padded leading dimension of X/U rows */
int sfm_pair_num_points(const sfm_pair *pair);
int sfm_get_XU(sfm_pair *pair, int which, float *h_out /* 3 x num_points */);
int sfm_get_E(sfm_pair *pair, float h_E[9]);
int sfm_get_best(sfm_pair *pair, uint32_t *hyp, uint32_t *count);
int sfm_get_key(sfm_pair *pair, uint64_t *key);
int sfm_get_inlier_counts(sfm_pair *pair, int32_t *h_counts, size_t capacity);
int sfm_get_inlier_mask(sfm_pair *pair, uint8_t *h_mask /* num_points */);
int sfm_get_E_candidates(sfm_pair *pair, float *h_E, size_t capacity_hyps);
int sfm_get_pose_candidates(sfm_pair *pair, float h_P[64]);
int sfm_get_pose_inverses(sfm_pair *pair, float h_Pinv[64]);
int sfm_get_pose_index(sfm_pair *pair, int *index);
int sfm_get_points(sfm_pair *pair, float *h_points /* 4 x num_points */);
/* Everything a many-pairs driver keeps of one pair, with ONE synchronisation:
 * [E (9) | chosen pose 4x4 (16): P^-1 in SFM_POSE_REFERENCE, P in SFM_POSE_CORRECT | pose index, inlier count, best hypothesis]. */
int sfm_get_result(sfm_pair *pair, float h_record[28]);
/* Many views (BASELINE configs[4]), front end: ExtractSift (src/main.cpp:258-279 per image) for the views first,
 * first + stride, ... of h_images (HOST images, width x height floats, tightly packed rows, grey values 0..255) into the
 * slots 0, 1, ... of d_block: slot s = max_pts SiftPoint records followed by the int32 feature count, slot_bytes apart.
 * Images go through pinned staging and two streams, so that upload and extraction of consecutive views overlap.
 * h_counts (optional): feature count per owned view.  A multi-GPU caller all-gathers the blocks afterwards (one
 * collective) and hands views to sfm_process_pairs.  Synchronous at the end. */
int sfm_extract_views(sfm_ctx *ctx, const float *const *h_images, int num_views, int width, int height, int first, int stride,
                      void *d_block, size_t slot_bytes, int max_pts, int num_octaves, double init_blur, float thresh,
                      float lowest_scale, int scale_up, int *h_counts);
/* The same for 8-bit grey images (what cv::imread(path, 0) hands src/main.cpp:249 before convertTo(CV_32FC1)): a quarter of
 * the bytes cross PCIe, the exact widening to float runs on the device.  Same features, bit for bit. */
int sfm_extract_views_u8(sfm_ctx *ctx, const unsigned char *const *h_images, int num_views, int width, int height, int first, int stride,
                         void *d_block, size_t slot_bytes, int max_pts, int num_octaves, double init_blur, float thresh,
                         float lowest_scale, int scale_up, int *h_counts);

/* Many view pairs (BASELINE configs[4]): the per-pair sequence of src/main.cpp:282-307 -- MatchSiftData (when d_sift2 is
 * given; it fills the match fields of d_sift1's records), fillXU, estimateE (num_hypotheses = 0: the reference's n1 / 8),
 * computePosecandidates, choosePose, linear_triangulation -- for the pairs first, first + stride, first + 2 stride, ... of
 * the list (rank r of G owns r, r + G, ...: no per-pair collective), enqueued back to back on the context's stream through
 * one pooled Image_pair, the result records assembled on the device and read back ONCE at the end.
 * h_records: 28 floats per owned pair in list order (layout of sfm_get_result; all -1 for a pair with fewer than 8
 * features); h_status (optional): SFM_OK / SFM_E_INVALID (too few features) / SFM_E_SINGULAR per owned pair -- when it
 * is NULL a singular pose makes the call return SFM_E_SINGULAR.  Synchronous at the end.
 * With SFM_POSE_REFERENCE, a K^-1 whose last row is (0 0 1) and at most 4096 hypotheses per pair the call is batched:
 * consecutive pairs that share their first view go through ONE matcher launch, fillXU / estimateE / choosePose /
 * triangulation are five launches for ALL owned pairs (fill_xu_pairs, ransac_pairs_solve, ransac_fused_pairs, choose_pose_pairs,
 * triangulate_pairs: same arithmetic, bit-identical records).  A list that holds an already matched pair (d_sift2 == NULL)
 * takes the per-pair loop; so does every call while the environment variable SFM_PAIRS_UNBATCHED is set (read on each call;
 * A/B runs, tests).  sfm_ctx_last_pairs_batched reports which path the last call took. */
typedef struct sfm_pair_desc {
    sfm_sift_point *d_sift1;        /* features of the first view (match fields are written when d_sift2 != NULL) */
    int n1;
    const sfm_sift_point *d_sift2;  /* features of the second view, or NULL when d_sift1 is already matched        */
    int n2;
} sfm_pair_desc;
#define SFM_RECORD_FLOATS 32        /* device-side record stride: 28 floats of sfm_get_result + singular flag + pad */
int sfm_process_pairs(sfm_ctx *ctx, const float h_K[9], const float h_Kinv[9], const sfm_pair_desc *pairs, int num_pairs,
                      int first, int stride, uint32_t num_hypotheses, int pose_mode, float *h_records, int *h_status);

int sfm_ctx_last_pairs_batched(sfm_ctx *ctx, int *batched);

/* Image_pair::copyBoidsToVBO (sfm.cu:374-383; kernCopyPositionsToVBO / kernCopyVelocitiesToVBO kernels.h:471-494):
 * interleaved (x, y, z, 1) * scale vertices and the constant (1, 1, 1, 1) colour buffer, written to DEVICE
 * buffers of 4 * num_points floats each (in the reference: the mapped GL buffer objects).  Either may be NULL. */
int sfm_copy_points_to_vbo(sfm_pair *pair, float *d_positions, float *d_velocities, float scale);
/* Name and launch geometry of the RANSAC scoring kernel used by the last call (for profiling). */
int sfm_ransac_last_launch(sfm_pair *pair, int *kernel, int *grid, int *block, int *lds_bytes);
/* Which form of the matrix-core pre-filter the last scoring launch ran (SFM_KERNEL_PREFILTER; 0 otherwise):
 * SFM_PREFILTER_PER_HYPOTHESIS -- operands per hypothesis, bounded over the whole views: the FIRST launch after a fillXU below 2^33
 * (hypothesis, correspondence) pairs, which would not earn back the ordering of the correspondences;
 * SFM_PREFILTER_PER_TILE -- operands per (hypothesis, tile) over a Morton-ordered copy of the correspondences, built by the first
 * launch that uses it and kept until the next fillXU.  Both give the same counts, keys and E bit for bit. */
#define SFM_PREFILTER_PER_HYPOTHESIS 2
#define SFM_PREFILTER_PER_TILE 3
int sfm_ransac_last_prefilter_rule(sfm_pair *pair, int *rule);
/* Sustained shader clock (MHz) during the last scoring launch (SFM_KERNEL_SPLIT / _PREFILTER): shader-clock ticks over
 * 100 MHz ticks across the lifetime of its first block; 0 if that kernel has not run.  Synchronises. */
int sfm_ransac_last_clock(sfm_pair *pair, double *shader_mhz);
#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SFM_AMD_H */
