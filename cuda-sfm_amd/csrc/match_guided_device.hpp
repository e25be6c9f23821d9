// match_guided_device.hpp -- what the guided matcher's kernels share: the staged row's position record, the position loads and
// stores that run beside stage_load / stage_store (match_mfma.hpp), and the gate stage_scores applies.  match_guided.hip (the
// one-match kernel) and match_guided_pairs.hip (the many-matches kernel) include it; the block's schedule itself is the fragment
// match_guided_body.inc.
#pragma once
#include "match_mfma.hpp"
#include "match_guided_math.hpp"

namespace sfm {

struct GuidedRow { float x, y, lim, pad; };          // one staged database row's position and limit (16 bytes in LDS)

// positions of the rows stage_load<W> requests (same clamped rows, unconditional loads)
template <int W>
__device__ __forceinline__ void stage_load_pos(const sfm_sift_point *__restrict__ sift2, int row0, int nrows, float2 (&pos)[16 / W])
{
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        const int row = min(row0 + pass * (4 * W) + rr, nrows - 1);
        pos[pass] = *reinterpret_cast<const float2 *>(&sift2[row].xpos);        // xpos, ypos: the record's first eight bytes
    }
}

// (x2, y2, lim2) of the rows stage_store<W> writes; lim2 = 0 for rows past the end and under an F that is not finite.  Every
// thread of a row's sixteen forms the value, the one that stages the row's first descriptor chunk stores it.
template <int W>
__device__ __forceinline__ void stage_store_pos(GuidedRow *side, const float2 (&pos)[16 / W], int row0, int nrows,
                                                const float (&F)[9], const bool f_ok, const float band)
{
    const int c8 = threadIdx.x & 15;
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        const int slot = pass * (4 * W) + rr;
        const bool real = row0 + slot < nrows;
        float lt[3];
        guided_line_t(F, pos[pass].x, pos[pass].y, lt);
        const float lim2 = real && f_ok ? guided_limit(lt, band) : 0.0f;
        if (c8 == 0) side[slot] = GuidedRow{ pos[pass].x, pos[pass].y, lim2, 0.0f };
    }
}

// stage_scores' gate: the lane's lines and limits against the stage's rows
template <int CT>
struct EpipolarGate {
    typedef GuidedRow Row;
    const GuidedRow *side;
    float l[CT][3], lim1[CT];
    __device__ __forceinline__ Row row(int slot) const { return side[slot]; }
    __device__ __forceinline__ float score(int ct, float s, const Row &r) const
    {
        return guided_pass(guided_residual(l[ct], r.x, r.y), lim1[ct], r.lim) ? s : -__builtin_inff();
    }
};

} // namespace sfm
