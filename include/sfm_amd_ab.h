/*
 * sfm_amd_ab.h -- the LAB-BENCH additions of libsfm_amd_ab.so (make ab: the product's sources built with -DSFM_AB=1).
 *
 * NOT part of the drop-in boundary (include/sfm_amd.h is).  This flavour exists for tests/ and profiles/: it keeps the
 * recorded slower kernel variants selectable, reads the A/B switches in sfm_ransac_params.reserved[] and exports probe /
 * trace hooks into the scoring kernel.  The product library refuses non-zero reserved[] and kernel id 3 with SFM_E_INVALID
 * and exports none of the functions below.
 */
#ifndef SFM_AMD_AB_H
#define SFM_AMD_AB_H

#include "sfm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* sfm_pair_device_ptr ids of the lab-bench library: the per-hypothesis records of the last pre-filter launch (64 bytes each, 16 with the per-tile
 * rule), the pair's bound words (bound | - | eight box words, each epoch << 32 | bits) and its table of occupied cells. */
#define SFM_AB_BUF_PF_RECORDS 100
#define SFM_AB_BUF_BOUND_WORDS 101
#define SFM_AB_BUF_CELLS 102
#pragma GCC visibility push(default)

/* Scoring with E.X on the f32 matrix cores (32 hypotheses per wavefront; csrc/ab/ransac_mfma.hip): bit-exact, measured
 * slower than the vector kernel (the f32 MFMA runs at the vector rate and overlaps with nothing); never picked by AUTO. */
#define SFM_KERNEL_MFMA   3

/* sfm_ransac_params.reserved[] in this flavour (0 = the product's behaviour):
 *   [0] solve kernel: 1 generic one-hypothesis-per-lane kernel with unconstrained registers (the product runs it capped at 256
 *       for the Jacobi solver), 7 the same capped at 168, 2 packed two-per-lane (Householder or Jacobi), 3 scalar Householder,
 *       4 scattered dword gathers instead of the 16-byte point records;
 *   [1] 1 tile loop inside the scoring block instead of the tile-parallel grid (n > 4096); 2 pre-filter passes handed out by
 *       position instead of through the block's LDS counter; 5 twelve wavefronts per pre-filter block; 7 tiles of up to 1536
 *       points; 9 a 256-entry ring flushed 128 entries at a time; 11 / 12 the packed scan software-pipelined over four accumulator
 *       sets with 16 / 12 wavefronts per block (30 spills / 140 registers: profiles/r06_ab_pack_scan.txt); 13 ring entries of 16
 *       bytes that cover four steps instead of 8 bytes per two steps (half as many appends: measured 3 % slower, r06_ab_wide_entries.txt);
 *       14 / 15 s_setprio 2 around the MFMA issue / around the exact filter of a flush (level: r06_ab_prio.txt); 13-15 run the per-tile form
 *       on every call; 18 the pre-filter launch sums its counts into counts[] without waiting for an answer, keys from ransac_argmax_counts
 *       behind it, at EVERY size (the product: from 2^21 (hypothesis, tile) partial counts per launch on); 16 / 17 the same, and in the drain
 *       a lane works through up to 1 / 7 further survivors of its ring entry before the rest is re-queued (per-tile form);
 *       19 the per-tile form prepares TWO passes at once, one hypothesis per lane, at EVERY size, with the summing epilogue (the product:
 *       from 2^22 partial counts per launch on; profiles/NOTES_r11.md: the headline step 2.8 % shorter, 8 pairs per wavefront 1.2 % longer);
 *       20 the single passes it replaced, with the summing epilogue, at every size (the product: between 2^21 and 2^22 partial counts) --
 *       21 the paired passes of 19 with the survivor ring EMPTIED between a pair's two scans, as in round 11 (the product and 19 carry the
 *       first scan's leftover entries into the second scan's flushes: an entry's tag names its scan; profiles/NOTES_r12.md) --
 *       22 the paired passes of 19 with the pair's two scans run BACK TO BACK over two walks of the tile, ring carried, as in round 12 (the
 *       product and 19 interleave them over one walk: a 32-point block's fragments are read from LDS once and multiplied with both halves'
 *       operands; profiles/NOTES_r13.md) --
 *       19 .. 22 leave the choice between the per-hypothesis and the per-tile form to the product's rule (combine with [3] = 7);
 *   [2] k > 0: minimum hypothesis batches per scoring block (default 8); pre-filter kernel: grid columns;
 *   [3] 1 AUTO never picks SFM_KERNEL_PREFILTER; 2 the round-2 pre-filter kernel (csrc/ab/ransac_prefilter_r2.hip);
 *       3 per-hypothesis records from the stand-alone kernel instead of the lane-solve kernel; 4 the G rule of rounds 2-4
 *       (per-pair threshold, three MFMAs per 32 x 32 pairs) instead of the band rule; 6 the packed scan with per-hypothesis 64-byte
 *       records and whole-view boxes on EVERY call (the product: on the first call after a fillXU below 2^33 pairs); 7 round 6's
 *       per-tile band constants on every call, the first included (tiles = runs of a Morton-bucket-ordered copy of the correspondences,
 *       sigma and the coefficient slots derived per (hypothesis, tile) inside the scoring kernel from a 16-byte record:
 *       profiles/r06_ab_tile_rule_fast.txt, r06_fresh_pair_cost.txt); 5 the band rule scanned with one
 *       v_alignbit_b32 per pair (round 5) instead of the six-bit conversion of round 6 ([1] = 5, 7, 9 imply it: those variants were
 *       built on that scan); 16 + bits: recorded variants built on the G rule; 8 + bits: the pass tail of the product's two rules
 *       (profiles/NOTES_r09.md, r09_pass_tail_ab.txt) -- 1 in the drain a lane works through up to 3 further survivors of its ring entry
 *       itself before the rest is re-queued (measured: no gain), 2 a survivor's bit position is decoded by arithmetic instead of the
 *       32-byte table in LDS (measured 0.3-0.6 % slower), 4 round 4's epilogue at every size: one returning 64-bit atomic per (hypothesis,
 *       tile), the keys made inside the scoring kernel (the product: below 2^21 partial counts per launch); each on its own or together. */

/* Where block 0 of the last pre-filter scoring launch (SFM_KERNEL_PREFILTER) spent its time: ticks[0] shader-clock ticks and
 * ticks[1] 100 MHz ticks over its lifetime (as above); 100 MHz ticks since its start at: [2] tile staged, [3] first pass'
 * coefficients prepared, [4] first 32-hypothesis block scanned and drained, [5] first pass done (counts and ticket out),
 * [6] number of passes wavefront 0 ran (paired passes: pairs) in the low 32 bits; paired passes also leave in [6] >> 32 the ring entries
 * wavefront 0 held when a second scan began, summed over its pairs (0 when the ring is emptied between the scans), and in [3] >> 32 the
 * ticks from the end of its first pair's first scan to the start of that pair's second ([3]'s low 32 bits: the stamp).  With the
 * interleaved scans (the product's instance, reserved[1] = 19) no second scan begins: [6] >> 32 is the number of entries waiting in the
 * ring each time a group of the second half's rows appends (once per two 32-point blocks), summed over the wavefront's two-scan pairs,
 * and [3] >> 32 is 0.
 * Zero where the kernel that ran has no such probe.  Synchronises. */
int sfm_ransac_last_phases(sfm_pair *pair, uint64_t ticks[8]);
/* Profiling aid: when did every block / wavefront of the last pre-filter scoring launch start and finish?  20 words per
 * block (up to 1024 blocks, in blockIdx.y * gridDim.x + blockIdx.x order): [0] start and [1] end of its first wavefront,
 * [2] (XCC id << 32) | HW_ID, [3] (tile << 32) | column, [4..19] the end of each of its 16 wavefronts -- all in 100 MHz
 * ticks of one device-wide counter.  *count = words written (0 if another kernel ran).  Synchronises. */
int sfm_ransac_last_trace(sfm_pair *pair, uint64_t *words, size_t capacity, size_t *count);
/* Test probe of the matrix-core pre-filter (ransac_prefilter.hip): the fp16 operands of ONE (hypothesis, point) pair as the
 * device builds them and what the matrix cores return for them.  h_point = (x1x, x1y, x2x, x2y), bound = the tile's largest
 * |coordinate|.  h_out: coefficient slots ns[32], ts[16] | feature slots bn[32], bt[16] | nt | G | rejected (0/1) |
 * zero-divisor state.  tests/test_gpu_prefilter.py compares them with the host build of the same header.  Synchronises. */
int sfm_prefilter_probe(sfm_ctx *ctx, const float h_E[9], float threshold, float bound, const float h_point[4], int survive_all,
                        float h_out[100]);

/* The same for the band rule (round 5): h_box = the coordinate ranges (x2 lo hi, y2 lo hi, x1 lo hi, y1 lo hi), b_safe = the second
 * divisor cannot vanish.  h_out: ns[32] | (unused) | bn[32] at 48 | nt at 96 | sigma at 97 | rejected at 98 | zero-divisor state of
 * the first divisor at 99, of the second at 100.  b_safe bit 1: the packed scan of round 6 (sigma = 1.873 / W, `rejected` from the
 * six-bit conversion).  At 101: how many of the 32 (accumulator, step) slots of the packed scan come out right for the RAW value
 * h_point[0]; at 102: the conversion's reject bit for it.  Synchronises. */
int sfm_prefilter_band_probe(sfm_ctx *ctx, const float h_E[9], float threshold, float bound, const float h_box[8], int b_safe,
                             const float h_point[4], int survive_all, float h_out[104]);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SFM_AMD_AB_H */
