// align_math.hpp -- arithmetic of the pair-to-pair alignment (align.hip): the similarity (s, R, t) with X_B = s R X_A + t that
// carries pair A's camera-1 frame into pair B's, from the points the two pairs share.
//
// A link is 13 floats: s, R (9, row-major), t (3).  A candidate is a point of A (X_A = X / W, camera-1 frame of A), the same
// feature's point of B (X_B), and the two view-1 observations (normalised, dehomogenised): o_A in A's view 1, o_B in B's.
//   forward   Y = s R X_A + t  against o_B through B's K
//   backward  Z = R^T (X_B - t) against o_A through A's K (a projection does not see the positive factor 1 / s: no division)
// Both go through register_math.hpp's division-free inlier test with the maps Pf = [s R | t] and Pb = [R^T | 0] (the latter
// applied to X_B - t): scoring, the LM's point set and the final mask share align_inlier.
//
// Everything here is fp32 with + - * /, sqrtf and fmaf only where written, fixed trip counts and no contraction (the rules of
// register_math.hpp), so the host build (tests/hostcheck/aligncheck.hip) and the gfx950 build give the same bits; the step on
// one lane (align_step) is fp64 like refine_rotate.
#pragma once
#include "device_math.hpp"
#include "refine_math.hpp"
#include "register_math.hpp"
#include "view_points_math.hpp"

namespace sfm {

constexpr int kAlignSim = 13;             // s, R (9), t (3)
constexpr int kAlignPar = 7;              // omega (3), dt (3), dsigma
constexpr int kAlignSys = 35;             // J^T W J (28 packed, symn<7>), J^T W r (7)
constexpr int kAlignMinCand = 3;          // fewer candidates: no sample
constexpr int kAlignMinInliers = 6;       // a winner with fewer inliers is SFM_REFINE_DEGENERATE (the registration's floor)

struct AlignCand { float Xa[3], Xb[3], oa[2], ob[2]; };

// Record j of A with index k: a candidate when k is a record of B and both points pass the registration's point test.  The
// caller reads B's column only where k is in range.
SFM_HD bool align_index_ok(int k, int nb) { return k >= 0 && k < nb; }
SFM_HD bool align_gate(bool valid_a, const float Xa[4], bool valid_b, const float Xb[4])
{
    return view_points_usable(valid_a, Xa) && view_points_usable(valid_b, Xb);
}

// the candidate of a gated record: X / W of both columns, both observations (x / z, y / z of the pairs' X0 columns)
SFM_HD void align_candidate(const float Xa[4], const float Xb[4], const float x0a[3], const float x0b[3], AlignCand &c)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.Xa[k] = Xa[k] / Xa[3]; c.Xb[k] = Xb[k] / Xb[3]; }
    c.oa[0] = x0a[0] / x0a[2]; c.oa[1] = x0a[1] / x0a[2];
    c.ob[0] = x0b[0] / x0b[2]; c.ob[1] = x0b[1] / x0b[2];
}

// the two maps of a link: Pf = [s R | t], Pb = [R^T | 0]
SFM_HD void align_maps(const float sim[kAlignSim], float Pf[12], float Pb[12])
{
    const float s = sim[0];
#pragma unroll
    for (int k = 0; k < 9; ++k) Pf[k] = s * sim[1 + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        Pf[9 + r] = sim[10 + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) Pb[3 * r + c] = sim[1 + 3 * c + r];
        Pb[9 + r] = 0.0f;
    }
}

// X_B - t
SFM_HD void align_back_point(const float Pf[12], const float Xb[3], float d[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = Xb[k] - Pf[9 + k];
}

// inlier iff the forward and the backward projection both pass register_inlier at thr (in front of the camera included)
SFM_HD bool align_inlier(const RefineCam &KA, const RefineCam &KB, float thr, const float Pf[12], const float Pb[12], const AlignCand &c)
{
    float d[3];
    align_back_point(Pf, c.Xb, d);
    const bool f = register_inlier(KB, thr, Pf, c.Xa, c.ob[0], c.ob[1]);
    const bool b = register_inlier(KA, thr, Pb, d, c.oa[0], c.oa[1]);
    return f && b;
}

// the larger of the two squared pixel errors (+inf behind a camera or where it is not finite)
SFM_HD float align_sq_error(const RefineCam &KA, const RefineCam &KB, const float Pf[12], const float Pb[12], const AlignCand &c)
{
    float d[3];
    align_back_point(Pf, c.Xb, d);
    const float ef = register_sq_error(KB, Pf, c.Xa, c.ob[0], c.ob[1]);
    const float eb = register_sq_error(KA, Pb, d, c.oa[0], c.oa[1]);
    return ef > eb ? ef : eb;
}

// Orthonormal triad of three points, rows of T: e1 = normalize(p2 - p1), e3 = normalize(e1 x (p3 - p1)), e2 = e3 x e1.
// False for collinear or coincident points (sin^2 of the angle at p1 below 1e-8, the registration's constant).
SFM_HD bool align_triad(const float p1[3], const float p2[3], const float p3[3], float T[9])
{
    float u[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { u[k] = p2[k] - p1[k]; v[k] = p3[k] - p1[k]; }
    const float n[3] = { u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0] };
    const float uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const float vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (!(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 1e-8f * (uu * vv))) return false;
    const float nu = sqrtf(uu);
    float e1[3], e3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = u[k] / nu;
    const float w[3] = { e1[1] * v[2] - e1[2] * v[1], e1[2] * v[0] - e1[0] * v[2], e1[0] * v[1] - e1[1] * v[0] };
    const float nw = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) e3[k] = w[k] / nw;
    const float e2[3] = { e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0] };
#pragma unroll
    for (int k = 0; k < 3; ++k) { T[k] = e1[k]; T[3 + k] = e2[k]; T[6 + k] = e3[k]; }
    return true;
}

// The minimal solver on three correspondences a[i] -> b[i]: R = T_B T_A^T from the two triads, s = sqrt(sum |b - mean b|^2 /
// sum |a - mean a|^2), t = mean b - s R mean a.  False, and the zero link (which no candidate passes: Y.z = 0), for collinear
// or coincident samples in either frame or a result that is not finite.
SFM_HD bool align_solve3(const float a[3][3], const float b[3][3], float sim[kAlignSim])
{
#pragma unroll
    for (int k = 0; k < kAlignSim; ++k) sim[k] = 0.0f;
    float Ta[9], Tb[9];
    const bool oka = align_triad(a[0], a[1], a[2], Ta);
    const bool okb = align_triad(b[0], b[1], b[2], Tb);
    if (!(oka && okb)) return false;
    float R[9], ma[3], mb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = Tb[r] * Ta[c] + Tb[3 + r] * Ta[3 + c] + Tb[6 + r] * Ta[6 + c];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ma[k] = (a[0][k] + a[1][k] + a[2][k]) / 3.0f; mb[k] = (b[0][k] + b[1][k] + b[2][k]) / 3.0f; }
    float va = 0.0f, vb = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float da = a[i][k] - ma[k], db = b[i][k] - mb[k];
            va += da * da; vb += db * db;
        }
    const float s = sqrtf(vb / va);
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = mb[r] - s * (R[3 * r] * ma[0] + R[3 * r + 1] * ma[1] + R[3 * r + 2] * ma[2]);
    bool fin = isfinite(s) && s > 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && isfinite(R[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && isfinite(t[k]);
    if (!fin) return false;
    sim[0] = s;
#pragma unroll
    for (int k = 0; k < 9; ++k) sim[1 + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) sim[10 + k] = t[k];
    return true;
}

// One RANSAC hypothesis over the m candidates: sample_distinct<3> keyed by (seed, hyp, m), align_solve3.  load(k, Xa, Xb) reads
// candidate k's two points.  The zero link for m < kAlignMinCand.
template <class Load>
SFM_HD bool align_hypothesis(uint32_t seed, uint32_t hyp, int m, Load &&load, float sim[kAlignSim])
{
    if (m < kAlignMinCand) {
#pragma unroll
        for (int k = 0; k < kAlignSim; ++k) sim[k] = 0.0f;
        return false;
    }
    int idx[3];
    sample_distinct<3>(seed, hyp, m, idx);
    float a[3][3], b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) load(idx[i], a[i], b[i]);
    return align_solve3(a, b, sim);
}

// Residuals r (forward x, y, backward x, y; pixels) and d r / d (omega, dt, dsigma) (4 x 7 row-major) of one candidate for the
// update R <- exp([omega]x) R, t <- t + dt, s <- s exp(dsigma).
//   forward:  d Y / d omega = -[q]x, d Y / d t = I, d Y / d sigma = q with q = s R X_A (register_jacobian on Pf, then the
//             sigma column);
//   backward: with d = X_B - t, Z = R^T d and g = R (d r / d Z)^T:  d r / d omega = g x d, d r / d t = -g, d r / d sigma = 0.
SFM_HD void align_jacobian(const RefineCam &KA, const RefineCam &KB, const float Pf[12], const float Pb[12], const AlignCand &c,
                           float r[4], float J[28])
{
    float Jf[12], Jb[12], q[3], d[3];
    register_jacobian(KB, Pf, c.Xa, c.ob[0], c.ob[1], r, Jf);
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = Pf[3 * a] * c.Xa[0] + Pf[3 * a + 1] * c.Xa[1] + Pf[3 * a + 2] * c.Xa[2];
    align_back_point(Pf, c.Xb, d);
    register_jacobian(KA, Pb, d, c.oa[0], c.oa[1], r + 2, Jb);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int k = 0; k < 6; ++k) J[7 * m + k] = Jf[6 * m + k];
        J[7 * m + 6] = Jf[6 * m + 3] * q[0] + Jf[6 * m + 4] * q[1] + Jf[6 * m + 5] * q[2];
        const float j0 = Jb[6 * m + 3], j1 = Jb[6 * m + 4], j2 = Jb[6 * m + 5];
        float g[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) g[cc] = Pb[cc] * j0 + Pb[3 + cc] * j1 + Pb[6 + cc] * j2;
        float *o = J + 14 + 7 * m;
        o[0] = g[1] * d[2] - g[2] * d[1];
        o[1] = g[2] * d[0] - g[0] * d[2];
        o[2] = g[0] * d[1] - g[1] * d[0];
        o[3] = -g[0]; o[4] = -g[1]; o[5] = -g[2];
        o[6] = 0.0f;
    }
}

// robust cost and squared error of one candidate: Huber per residual pair
SFM_HD void align_cost(const float r[4], float huber, float &cost, float &sq)
{
    float rf, rb;
    refine_huber(r[0], r[1], huber, rf);
    refine_huber(r[2], r[3], huber, rb);
    cost = rf + rb;
    sq = (r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]);
}

// One candidate's share of the weighted normal equations: emit(q, value) receives J^T W J (packed, symn<7>) at q = 0..27 and
// J^T W r at 28..34; wf, wb: the weights of the forward and the backward pair.
template <class Emit>
SFM_HD void align_terms(const float r[4], const float J[28], float wf, float wb, Emit &&emit)
{
#pragma unroll
    for (int i = 0; i < kAlignPar; ++i) {
#pragma unroll
        for (int k = i; k < kAlignPar; ++k)
            emit(symn<kAlignPar>(i, k), wf * (J[i] * J[k] + J[7 + i] * J[7 + k]) + wb * (J[14 + i] * J[14 + k] + J[21 + i] * J[21 + k]));
        emit(28 + i, wf * (J[i] * r[0] + J[7 + i] * r[1]) + wb * (J[14 + i] * r[2] + J[21 + i] * r[3]));
    }
}

// one lane: the link after the step d = (omega, dt, dsigma), fp64
SFM_HD void align_step(const double d[kAlignPar], const float sim[kAlignSim], float out[kAlignSim])
{
    float Rn[9];
    refine_rotate(d, sim + 1, Rn);
    out[0] = (float)((double)sim[0] * exp(d[6]));
#pragma unroll
    for (int k = 0; k < 9; ++k) out[1 + k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[10 + k] = (float)((double)sim[10 + k] + d[3 + k]);
}

// the identity link
SFM_HD void align_identity(float sim[kAlignSim])
{
#pragma unroll
    for (int k = 0; k < kAlignSim; ++k) sim[k] = (k == 0 || k == 1 || k == 5 || k == 9) ? 1.0f : 0.0f;
}

} // namespace sfm
