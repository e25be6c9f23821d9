// match_guided_math.hpp -- the arithmetic of sfm_match_guided's gate and of sfm_pair_fundamental, shared by the kernels
// (match_guided.hip) and the host build (tests/hostcheck/matchguidedcheck.hip).  Single precision with explicit fmaf where a fused
// operation is meant (the build has -ffp-contract=off), so both builds produce the same bits.
//
// Convention: F is row-major, in pixel coordinates, and a true correspondence has u2^T F u1 = 0 with u1 = (xpos, ypos, 1) of a
// record of the FIRST set and u2 = (xpos, ypos, 1) of a record of the second set (what the match writes into match_xpos /
// match_ypos).  A pair (u1, u2) is in the band when u2 lies within band pixels of u1's epipolar line F u1 in view 2 AND u1 lies
// within band pixels of u2's line F^T u2 in view 1: with d = u2^T F u1 (one scalar for both directions)
//     d^2 <= band^2 (l0^2 + l1^2)   for both lines l,
// the squared point-to-line distances without a division.
#pragma once
#include "device_math.hpp"

namespace sfm {

// l = F (x, y, 1): the epipolar line in view 2 of a view-1 feature
SFM_HD void guided_line(const float *F, float x, float y, float l[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) l[r] = fmaf(F[3 * r], x, fmaf(F[3 * r + 1], y, F[3 * r + 2]));
}

// l = F^T (x, y, 1): the epipolar line in view 1 of a view-2 feature
SFM_HD void guided_line_t(const float *F, float x, float y, float l[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) l[r] = fmaf(F[r], x, fmaf(F[3 + r], y, F[6 + r]));
}

// band^2 |(l0, l1)|^2: what d^2 may reach.  0 for a feature on the epipole (its line is undefined), NaN when anything is
SFM_HD float guided_limit(const float l[3], float band) { return (band * band) * (l[0] * l[0] + l[1] * l[1]); }

// d = u2^T F u1 from u1's line (guided_line): serves both directions
SFM_HD float guided_residual(const float l[3], float x2, float y2) { return fmaf(l[0], x2, fmaf(l[1], y2, l[2])); }

// every comparison is false on a NaN; a limit of 0 (the epipole, a zero F, a row past the end) passes nothing, not even d = 0
SFM_HD bool guided_pass(float d, float lim1, float lim2)
{
    const float dd = d * d;
    return dd <= lim1 && dd <= lim2 && lim1 > 0.0f && lim2 > 0.0f;
}

// an F with an infinite entry would give infinite limits that an infinite d^2 "reaches": such an F gates everything out
// (its limits are replaced by 0), like one with a NaN
SFM_HD bool guided_finite(const float *F)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && fabsf(F[i]) < __builtin_inff();
    return ok;
}

// sfm_pair_fundamental: F = Kinv^T M Kinv in fp64, M = E (transpose == false) or E^T, scaled to unit Frobenius norm and rounded
// once; all zero where the product is zero or not finite.  Sums run left to right over k = 0, 1, 2.
SFM_HD void guided_fundamental(const float *E, const float *Kinv, bool transpose, float F[9])
{
    double M[9], T[9], G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (double)(transpose ? E[3 * c + r] : E[3 * r + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r)                      // T = M Kinv
#pragma unroll
        for (int c = 0; c < 3; ++c)
            T[3 * r + c] = (M[3 * r] * (double)Kinv[c] + M[3 * r + 1] * (double)Kinv[3 + c]) + M[3 * r + 2] * (double)Kinv[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)                      // G = Kinv^T T
#pragma unroll
        for (int c = 0; c < 3; ++c)
            G[3 * r + c] = ((double)Kinv[r] * T[c] + (double)Kinv[3 + r] * T[3 + c]) + (double)Kinv[6 + r] * T[6 + c];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = ss + G[i] * G[i];
    const double nrm = sqrt(ss);
    const bool ok = nrm > 0.0 && nrm < (double)__builtin_inff();      // (false on a NaN)
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = ok ? (float)(G[i] / nrm) : 0.0f;
}

} // namespace sfm
