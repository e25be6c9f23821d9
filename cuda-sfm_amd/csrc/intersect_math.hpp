// intersect_math.hpp -- arithmetic of sfm_intersect_tracks (intersect.hip): every track of a fused table intersected over all its
// views under a given camera table.
//
// A track that is not copied through has two start candidates: C, its input column dehomogenised as chain_used does, and L, the
// linear intersection of its views' rays (two rows per view, the 3 x 3 normal equations summed in fp64 in list order, solved in
// fp64, rounded once).  A candidate is eligible when it is finite and lies in front of every view; the start is the eligible
// candidate with the smaller fuse_cost, C on a tie.  From the start the track goes through fuse_point's steps (fuse_lm, then
// fuse_accept), and its class stays its own: a seam track (flag 3 or 4) comes out SEAM_REFINED or SEAM_KEPT.
//
// Every sum over the views is a sum of PER-VIEW TERMS taken in list order, and every per-view term has a function of its own
// here (intersect_rows, intersect_cost_term, intersect_lm_terms, intersect_accept_term, intersect_depth).  The serial walk
// (intersect_track: fuse_cost, fuse_lm and fuse_accept as they are) and the wavefront kernel, where lane l forms the term of view
// l and one lane per accumulator adds them in list order, therefore give the same bytes: without contraction `V += w * (...)` is
// a rounded product and a rounded add, and 0 + term is term.  Compiled as HIP host code by tests/hostcheck/intersectcheck.hip.
#pragma once
#include "fuse_math.hpp"
#include "chain_adjust_math.hpp"
#include "view_points_math.hpp"

namespace sfm {

constexpr int kIntersectWaveMinViews = 32;        // sfm_intersect_params.wave_min_views == 0
// the normal equations are taken for singular when det A is not above this share of the product of A's diagonal: the rays of a
// track whose views share one centre meet at ~1e-14 (fp32 observations), a parallax of 1e-3 rad at ~1e-6
constexpr double kIntersectSingular = 1e-10;

constexpr int kIntersectCounts = 8;               // d_counts: T, re-intersected, REFINED class, KEPT class, copied, from L, no start, promoted

// a track is copied through: its flag is no SFM_FUSE_* class, it has fewer than two views, or the caller skips it
SFM_HD bool intersect_copied(int flag, int count, bool skip) { return flag < SFM_FUSE_REFINED || flag > SFM_FUSE_SEAM_KEPT || count < 2 || skip; }

// the class mapping: the KEPT or REFINED flag of the input flag's class (1, 2: the chain's; 3, 4: the seam's)
SFM_HD uint8_t intersect_class(int flag, bool accepted)
{
    const bool seam = flag == SFM_FUSE_SEAM_REFINED || flag == SFM_FUSE_SEAM_KEPT;
    return (uint8_t)(accepted ? (seam ? SFM_FUSE_SEAM_REFINED : SFM_FUSE_REFINED) : (seam ? SFM_FUSE_SEAM_KEPT : SFM_FUSE_KEPT));
}
SFM_HD bool intersect_promoted(int flag, bool accepted) { return accepted && (flag == SFM_FUSE_KEPT || flag == SFM_FUSE_SEAM_KEPT); }

// candidate C: the input column as chain_used takes it; false: not finite
SFM_HD bool intersect_dehom(const float Xin[4], float X[3])
{
    X[0] = Xin[0] / Xin[3]; X[1] = Xin[1] / Xin[3]; X[2] = Xin[2] / Xin[3];
    return isfinite(Xin[0]) && isfinite(Xin[1]) && isfinite(Xin[2]) && isfinite(Xin[3]) && Xin[3] != 0.0f &&
           isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

// one view's share of the normal equations: its rows u = x r3 - r1 and w = y r3 - r2 with right-hand sides t1 - x t3 and t2 - y t3;
// a = u u^T + w w^T (packed sym3), b = u rhs_u + w rhs_w
SFM_HD void intersect_rows(const FuseView &v, double a[6], double b[3])
{
    const double x = (double)v.x, y = (double)v.y;
    double u[3], w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u[c] = x * (double)v.P[6 + c] - (double)v.P[c];
        w[c] = y * (double)v.P[6 + c] - (double)v.P[3 + c];
    }
    const double ru = (double)v.P[9] - x * (double)v.P[11], rw = (double)v.P[10] - y * (double)v.P[11];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int q = p; q < 3; ++q) a[sym3(p, q)] = u[p] * u[q] + w[p] * w[q];
        b[p] = u[p] * ru + w[p] * rw;
    }
}

// A X = b by the adjugate in fp64, rounded once; a singular system (kIntersectSingular) gives NaNs
SFM_HD void intersect_solve(const double A[6], const double b[3], float L[3])
{
    const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (!(det > kIntersectSingular * ((a00 * a11) * a22))) {
        L[0] = L[1] = L[2] = __builtin_nanf("");
        return;
    }
    L[0] = (float)(((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det);
    L[1] = (float)(((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det);
    L[2] = (float)(((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det);
}

// candidate L over the list, the views' terms added in list order
template <class Views>
SFM_HD void intersect_linear(int count, Views &&view, float L[3])
{
    double A[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, b[3] = { 0.0, 0.0, 0.0 };
    for (int o = 0; o < count; ++o) {
        double a[6], c[3];
        intersect_rows(view(o), a, c);
#pragma unroll
        for (int q = 0; q < 6; ++q) A[q] += a[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) b[q] += c[q];
    }
    intersect_solve(A, b, L);
}

// the depth of X in a view (chain_used's front test reads its sign)
SFM_HD float intersect_depth(const FuseView &v, const float X[3])
{
    float Y[3];
    register_to_cam(v.P, X, Y);
    return Y[2];
}

SFM_HD bool intersect_finite(const float X[3]) { return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]); }

// X lies in front of every view
template <class Views>
SFM_HD bool intersect_front(int count, Views &&view, const float X[3])
{
    bool front = true;
    for (int o = 0; o < count; ++o) front = intersect_depth(view(o), X) > 0.0f && front;
    return front;
}

// the terms of fuse_cost, fuse_lm's system and fuse_accept for one view: what the walks add (or and, or take the larger of)
SFM_HD float intersect_cost_term(const FuseView &v, float huber, const float X[3])
{
    float Y[3], r[2], J[6], rho;
    register_to_cam(v.P, X, Y);
    refine_view(v.K, Y[0], Y[1], Y[2], v.x, v.y, r, J);
    refine_huber(r[0], r[1], huber, rho);
    return rho;
}
SFM_HD void intersect_lm_terms(const FuseView &v, float huber, const float X[3], float t[10])      // V (6), g (3), cost
{
#pragma unroll
    for (int q = 0; q < 10; ++q) t[q] = 0.0f;
    view_points_terms(v.K, v.P, X, v.x, v.y, huber, t, t + 6, t[9]);
}
SFM_HD float intersect_accept_term(const FuseView &v, float thr, const float X[3], bool &ok)
{
    ok = register_inlier(v.K, thr, v.P, X, v.x, v.y);
    return register_sq_error(v.K, v.P, X, v.x, v.y);
}

// which candidate starts the track: 0 none, 1 C, 2 L (the costs are read only where the candidate is eligible)
constexpr int kIntersectNone = 0, kIntersectC = 1, kIntersectL = 2;
SFM_HD int intersect_choose(bool c_ok, float c_cost, bool l_ok, float l_cost)
{
    if (c_ok && l_ok) return l_cost < c_cost ? kIntersectL : kIntersectC;
    return c_ok ? kIntersectC : (l_ok ? kIntersectL : kIntersectNone);
}

// the error of a column that is copied through: sfm_adjust_chain's d_err rule under the given cameras
template <class Views>
SFM_HD float intersect_error(int count, Views &&view, const float col[4])
{
    const float X[3] = { col[0] / col[3], col[1] / col[3], col[2] / col[3] };
    float e2 = 0.0f;
    for (int o = 0; o < count; ++o) {
        const FuseView v = view(o);
        e2 = fmaxf(e2, register_sq_error(v.K, v.P, X, v.x, v.y));
    }
    return sqrtf(e2);
}

// what became of one track
struct IntersectResult {
    float out[4];
    float err;
    uint8_t flag;
    int start;                            // kIntersectNone / C / L (copied through: none)
    bool copied, promoted;
};

// the finish of a track that has no eligible start, and of one that has: shared by the serial walk and the wavefront kernel
SFM_HD void intersect_no_start(int flag, const float Xin[4], IntersectResult &r)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) r.out[c] = Xin[c];
    r.err = __builtin_inff();
    r.flag = (uint8_t)flag;
    r.start = kIntersectNone; r.copied = false; r.promoted = false;
}
SFM_HD void intersect_finish(int flag, int start, const float S[3], const float X[3], bool ok, float err, IntersectResult &r)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) r.out[c] = ok ? X[c] : S[c];
    r.out[3] = 1.0f;
    r.err = err;
    r.flag = intersect_class(flag, ok);
    r.start = start; r.copied = false; r.promoted = intersect_promoted(flag, ok);
}

// One track, the list walked serially: the lane kernel's lane and the host build.  view(o): its views under the given cameras.
template <class Views>
SFM_HD void intersect_track(int flag, int count, bool skip, const float Xin[4], Views &&view, const sfm_intersect_params &p, IntersectResult &r)
{
    if (intersect_copied(flag, count, skip)) {
#pragma unroll
        for (int c = 0; c < 4; ++c) r.out[c] = Xin[c];
        r.err = intersect_error(count, view, Xin);
        r.flag = (uint8_t)flag;
        r.start = kIntersectNone; r.copied = true; r.promoted = false;
        return;
    }
    float C[3], L[3];
    bool c_ok = intersect_dehom(Xin, C);
    intersect_linear(count, view, L);
    bool l_ok = intersect_finite(L);
    c_ok = c_ok && intersect_front(count, view, C);
    l_ok = l_ok && intersect_front(count, view, L);
    const float c_cost = c_ok ? fuse_cost(count, view, p.huber_px, C) : 0.0f, l_cost = l_ok ? fuse_cost(count, view, p.huber_px, L) : 0.0f;
    const int start = intersect_choose(c_ok, c_cost, l_ok, l_cost);
    if (start == kIntersectNone) { intersect_no_start(flag, Xin, r); return; }
    const float S[3] = { start == kIntersectL ? L[0] : C[0], start == kIntersectL ? L[1] : C[1], start == kIntersectL ? L[2] : C[2] };
    float X[3] = { S[0], S[1], S[2] }, err;
    fuse_lm(count, view, p.max_iterations, p.huber_px, p.min_rel_decrease, p.initial_lambda, X);
    const bool ok = fuse_accept(count, view, p.threshold_px, X, err);
    intersect_finish(flag, start, S, X, ok, err, r);
}

} // namespace sfm
