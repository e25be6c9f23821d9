// match_mfma.hpp -- the pieces of the exact fp32 MFMA matcher that more than one translation unit instantiates: the staging of
// descriptor rows through LDS, the resident query fragments, the MFMA loop with its top-2 epilogue and the launch plan; the
// per-split partials with the ticket merge are the fragment match_ticket_merge.inc.  match.hip (sfm_match's exact kernel, with and without the polled merge, and the
// many-matches kernel) and match_guided.hip (sfm_match_guided: the same scores behind an epipolar gate) are built from them; the
// description of the tile mapping and of the numerics is at the top of match.hip.
#pragma once
#include <stdlib.h>
#include "match_common.hpp"

namespace sfm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRowsPerStage = 64;        // database rows per LDS stage (RT = 2 MFMA row tiles)
constexpr int kLdsStride = 132;          // floats per staged row

// Stage `rows` descriptor rows (first row `row0`, zero beyond `nrows`) into buf[rows][132].  The loads are unconditional
// (from a clamped row; the zeros are selected when the values are stored): with branches around them the compiler cannot
// count the loads in flight and waits for ALL of them -- the prefetch it has just issued -- before the stage's first MFMA.
template <int W>
__device__ __forceinline__ void stage_load(const float *__restrict__ base, int ld, int row0, int nrows,
                                           float4 (&regs)[16 / W][2])
{
    const int c8 = threadIdx.x & 15;             // which 8-float chunk of the 128
    const int rr = threadIdx.x >> 4;             // 4*W rows per pass
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        const int row = min(row0 + pass * (4 * W) + rr, nrows - 1);
        const float4 *src = reinterpret_cast<const float4 *>(base + (size_t)row * ld + 8 * c8);
        regs[pass][0] = src[0];
        regs[pass][1] = src[1];
    }
}

template <int W>
__device__ __forceinline__ void stage_store(float *buf, const float4 (&regs)[16 / W][2], int row0, int nrows)
{
    const int c8 = threadIdx.x & 15;
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        float4 *dst = reinterpret_cast<float4 *>(buf + (pass * (4 * W) + rr) * kLdsStride + 8 * c8);
        const bool real = row0 + pass * (4 * W) + rr < nrows;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = real ? regs[pass][0] : z, b = real ? regs[pass][1] : z;
        dst[0] = make_float4(a.x, a.z, b.x, b.z);      // even d: k-parity 0
        dst[1] = make_float4(a.y, a.w, b.y, b.w);      // odd d : k-parity 1
    }
}

// What stands between an accumulator element and top2_push (stage_scores): gate.row(slot) is what the gate knows about the
// stage's row `slot`, gate.score(ct, s, row) the value pushed for column tile ct.  The plain matcher pushes every score as it is.
struct NoGate {
    struct Row {};
    __device__ __forceinline__ Row row(int) const { return Row{}; }
    __device__ __forceinline__ float score(int, float s, const Row &) const { return s; }
};

// The scores of one staged block of database rows (RT row tiles of 32) against the wavefront's resident queries, folded into
// the running top-2 in ascending database index.
template <int CT, int RT, class Gate>
__device__ __forceinline__ void stage_scores(const float *cur, const float (&bq)[CT][64], Top2 (&top)[CT], int stage_row0, const Gate &gate)
{
    const int lane = threadIdx.x & 63;
    const int col = lane & 31;
    const int half = lane >> 5;
    f32x16 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.0f;

    const float *a0p = cur + col * kLdsStride + 4 * half;
    const float *a1p = a0p + 32 * kLdsStride;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const float4 a0 = *reinterpret_cast<const float4 *>(a0p + 8 * m);
        const float a0v[4] = { a0.x, a0.y, a0.z, a0.w };
        float a1v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (RT == 2) {
            const float4 a1 = *reinterpret_cast<const float4 *>(a1p + 8 * m);
            a1v[0] = a1.x; a1v[1] = a1.y; a1v[2] = a1.z; a1v[3] = a1.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                acc[0][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0v[k], bq[ct][4 * m + k], acc[0][ct], 0, 0, 0);
                if (RT == 2) acc[RT - 1][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[k], bq[ct][4 * m + k], acc[RT - 1][ct], 0, 0, 0);
            }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p2 = stage_row0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const typename Gate::Row row = gate.row(rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) top2_push(top[ct], gate.score(ct, acc[rt][ct][r], row), p2);
        }
}

template <int CT, int RT>
__device__ __forceinline__ void stage_scores(const float *cur, const float (&bq)[CT][64], Top2 (&top)[CT], int stage_row0)
{
    stage_scores<CT, RT>(cur, bq, top, stage_row0, NoGate());
}


// The resident query fragments b[ct][2m + half], m = 0..63, of the block's CT * 32 * W queries (first query q0), staged through
// the two LDS buffers.  Ends with a barrier: the buffers are free afterwards.  (match.hip's match_body keeps this loop written out
// in place: as a function, with the buffers behind a reference, it compiles to other address arithmetic, and that file's kernels
// are pinned instruction for instruction.)
template <int CT, int W>
__device__ __forceinline__ void load_queries(const float *__restrict__ q, int nq, int ldq, int q0,
                                             float (&lds)[2][kRowsPerStage * kLdsStride], float (&bq)[CT][64])
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 31;
    const int half = lane >> 5;
    float4 regs[16 / W][2];
    constexpr int kChunks = CT * 32 * W / kRowsPerStage;
    // chunks alternate between the two LDS buffers and the next chunk's global loads are in flight while this one is
    // read back: one barrier per chunk, memory latency hidden behind the LDS reads
    stage_load<W>(q, ldq, q0, nq, regs);
    for (int ch = 0; ch < kChunks; ++ch) {
        float *buf = lds[ch & 1];
        stage_store<W>(buf, regs, q0 + ch * kRowsPerStage, nq);
        __syncthreads();
        if (ch + 1 < kChunks) stage_load<W>(q, ldq, q0 + (ch + 1) * kRowsPerStage, nq, regs);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int r = (wave * CT + ct) * 32 - ch * kRowsPerStage;     // first row of this column tile in the chunk
            if (r >= 0 && r < kRowsPerStage) {
                const float *src = buf + (r + col) * kLdsStride + 4 * half;
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + 8 * m);
                    bq[ct][4 * m + 0] = v.x; bq[ct][4 * m + 1] = v.y;
                    bq[ct][4 * m + 2] = v.z; bq[ct][4 * m + 3] = v.w;
                }
            }
        }
    }
    __syncthreads();
}

// The launch plan of a one-match call: one of three configurations (column tiles per wavefront, wavefronts per block), crossovers
// measured with profiles/match_cfg_probe.py
// (TFLOP/s at n x n):  n      3000   4500   5500   7000   9000   10000  12000  14000  16384
//                      (1,4)  64     79     72     79     81
//                      (1,8)  58     78     91     98     105    104    110    106    123
//                      (2,8)  42     70     84     91     103    102    112    118    127
// and the split of the database over blocks.
struct ExactMatchPlan { int ct, wv, qblocks, nsplit, rows_per_split; };

inline ExactMatchPlan exact_match_plan(int num_cus, int n1, int n2, int max_ct = 2)
{
    ExactMatchPlan p;
    static const char *cfg_env = getenv("SFM_MATCH_CFG");    // profiling only: "ct,wv"
    p.ct = n1 > 11000 ? 2 : 1;
    p.wv = n1 > 4500 ? 8 : 4;                        // wavefronts per block
    if (cfg_env && cfg_env[0] && cfg_env[1] && cfg_env[2]) { p.ct = cfg_env[0] == '2' ? 2 : 1; p.wv = cfg_env[2] == '8' ? 8 : 4; }
    if (p.ct > max_ct) { p.ct = max_ct; p.wv = 8; }  // (a kernel without the two-tile configuration: the largest one-tile block)
    const int qper = p.ct * 32 * p.wv;                      // queries per block
    p.qblocks = (n1 + qper - 1) / qper;
    // (query block, database split) pairs: as many as fit in ONE round over the CUs, not more -- rounding the split
    // count up (11 x 24 = 264 blocks on 256 CUs) costs a whole second round (12000 x 12000: 0.44 -> 0.30 ms), and two
    // blocks per CU of the small configuration only add prologues and partials (2048 x 2048: 0.026 -> 0.022 ms)
    int nsplit = num_cus / p.qblocks;
    const int max_split = (n2 + kRowsPerStage - 1) / kRowsPerStage;
    if (nsplit > max_split) nsplit = max_split;
    if (nsplit < 1) nsplit = 1;
    // a split is a whole number of 32-row tiles (its last stage runs one row tile instead of two when 32 rows or fewer are
    // left): 2155 x 2170 is 14 splits of 160 rows = 2.5 stages of matrix work per wavefront instead of 12 x 192 = 3
    int rows_per_split = (n2 + nsplit - 1) / nsplit;
    rows_per_split = round_up(rows_per_split, kRowsPerStage / 2);
    p.rows_per_split = rows_per_split;
    p.nsplit = (n2 + rows_per_split - 1) / rows_per_split;
    return p;
}

} // namespace sfm
