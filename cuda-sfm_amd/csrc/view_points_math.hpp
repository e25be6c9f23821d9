// view_points_math.hpp -- arithmetic of sfm_triangulate_view (view_points.hip): one point of a pair over the pair's two cameras
// and its registered view.
//
// Cameras: 1 = [I|0], 2 = P2 = [R|t], 3 = P3 = [R3|t3] (12 floats each: R row-major, then t), all fixed.  A record that view 3 sees
// (the registration's gate) either has a usable input point -- it starts at X / W and is refined over views 1, 2 and 3 -- or has
// none -- it starts at the DLT of views 1 and 3 (tri_rows / nullvec4, the triangulation of pose.hip) and is refined over those
// two.  The refinement is a Levenberg-Marquardt on the three point coordinates: per view refine_view's pixel residual and its
// 2 x 3 Jacobian times the view's rotation, refine_huber's weights, V = sum w J^T J (packed sym3), g = sum w J^T r, the step
// -(V + lambda diag V)^-1 g by refine_damped_inverse3, LmControl's damping, accept and stop rules with one instance per point.
// The result is accepted when every view used passes register_inlier and, for a new point, the rays of cameras 1 and 3 subtend
// enough of an angle.
//
// Everything here is fp32 with + - * /, sqrtf and fmaf only where written, bounded iteration counts and no contraction, so the
// host build (tests/hostcheck/viewpointscheck.hip) and the gfx950 build give the same bits under the Makefile's flags.
#pragma once
#include <stddef.h>
#include "device_math.hpp"
#include "refine_math.hpp"
#include "register_math.hpp"

namespace sfm {

constexpr int kViewPointsSweeps = 8;      // = kSweeps4 of pose.hip: a new point starts where sfm_triangulate would put it

// One call on one pair.  Every pointer is device memory in the kernels and host memory in the host build.
struct ViewPointsArgs {
    const sfm_sift_point *sift;           // view 1's records re-matched against view 3
    const float *X0, *X1;                 // the pair's normalised observations, 3 x ld
    const float *K, *Kinv;                // 9 each
    const float *points;                  // input points, 4 x n
    const uint8_t *valid;                 // n, or null: every point
    const float *pose2, *pose3;           // pose_rows == 3: [R|t] as R (9) then t (3); 4: a 4 x 4 row-major matrix
    int pose_rows;
    int ld, n;
    float min_score, max_ambiguity;
    float thr, cos_min;                   // cos_min: cosine of the smallest accepted parallax
    int max_iter;
    float huber, min_rel, lambda0;
    float *out_points;                    // 4 x n
    uint8_t *out_flags;                   // n
    float *out_err;                       // n, or null
    int *out_counts;                      // 8, or null
};

// cosine of the smallest accepted parallax: computed once per call on the host, in double, rounded to float
inline float view_points_cos_min(float min_parallax_deg) { return (float)cos((double)min_parallax_deg * (3.14159265358979323846 / 180.0)); }

struct ViewPointsCams { RefineCam K; float Kinv[9]; float P2[12], P3[12]; };

// what one lane knows of its point before any arithmetic on it
struct ViewPointsLane {
    bool seen, usable;
    float obs[6];                         // (x, y) of views 1, 2, 3
    float Xin[4];                         // the input column
};

// bytes 24..31 and 32..47 of a record (sfm_sift_point: 576 bytes, a multiple of 16) as vector values, which the compiler neither
// splits nor merges: one 8-byte and one 16-byte load per record, issued before anything is decided from them (the record array
// must be 16-byte aligned)
typedef float vp_f32x2 __attribute__((ext_vector_type(2)));
typedef float vp_f32x4 __attribute__((ext_vector_type(4)));
static_assert(offsetof(sfm_sift_point, score) == 24 && offsetof(sfm_sift_point, match) == 32 && offsetof(sfm_sift_point, match_ypos) == 40 &&
              sizeof(sfm_sift_point) % 16 == 0, "record layout");

// [R|t] from either layout of ViewPointsArgs::pose2 / pose3
SFM_HD void view_points_pose(const float *p, int rows, float P[12])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P[3 * r + c] = rows == 4 ? p[4 * r + c] : p[3 * r + c];
        P[9 + r] = rows == 4 ? p[4 * r + 3] : p[9 + r];
    }
}

// register_gate's point test: valid flag set, finite, W != 0, in front of camera 1
SFM_HD bool view_points_usable(bool valid, const float X[4])
{
    return valid && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(X[3]) && X[3] != 0.0f && X[2] / X[3] > 0.0f;
}

// Point j of the call.  The five record fields sit at bytes 24..43 of the 576-byte record: one 8-byte load (score, ambiguity)
// and one 16-byte load (match, match_xpos, match_ypos, match_error), both aligned.
SFM_HD void view_points_load(const ViewPointsArgs &a, const float Kinv[9], int j, ViewPointsLane &L)
{
    const char *rec = reinterpret_cast<const char *>(a.sift + j);
    const vp_f32x2 sa = *reinterpret_cast<const vp_f32x2 *>(rec + 24);                    // score, ambiguity
    asm volatile("" ::: "memory");              // keeps the two apart: merged, they become 16 bytes at +24 (unaligned) and 8 at +40
    const vp_f32x4 m = *reinterpret_cast<const vp_f32x4 *>(rec + 32);                     // match (int32), match_xpos, match_ypos, match_error
    const bool matched = __builtin_bit_cast(int32_t, m.x) >= 0, scored = sa.x > a.min_score, clear = sa.y < a.max_ambiguity;
    L.seen = matched & scored & clear;                                                    // no short circuit: nothing to hang a load on
#pragma unroll
    for (int c = 0; c < 4; ++c) L.Xin[c] = a.points[(size_t)c * a.n + j];
    L.usable = view_points_usable(!a.valid || a.valid[j] != 0, L.Xin);
    const float z1 = a.X0[2 * (size_t)a.ld + j], z2 = a.X1[2 * (size_t)a.ld + j];
    L.obs[0] = a.X0[j] / z1; L.obs[1] = a.X0[(size_t)a.ld + j] / z1;
    L.obs[2] = a.X1[j] / z2; L.obs[3] = a.X1[(size_t)a.ld + j] / z2;
    const float u = m.y, v = m.z;
    float x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = fmaf(Kinv[3 * r + 2], 1.0f, fmaf(Kinv[3 * r + 1], v, Kinv[3 * r] * u));      // fill_xu_kernel's K^-1 u
    L.obs[4] = x[0] / x[2]; L.obs[5] = x[1] / x[2];
}

// the start of a new point: the null vector of the DLT rows of views 1 and 3, dehomogenised; false where w == 0 or the
// result is not finite
SFM_HD bool view_points_dlt(float x1, float y1, float x3, float y3, const float P3[12], float X[3])
{
    const float M1[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    const float M3[12] = { P3[0], P3[1], P3[2], P3[9], P3[3], P3[4], P3[5], P3[10], P3[6], P3[7], P3[8], P3[11] };
    float A[16], v[4];
    tri_rows(x1, y1, x3, y3, M1, M3, A);
    nullvec4(A, kViewPointsSweeps, v);
    const float w = v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = v[k] / w;
    return w != 0.0f && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

// One view's share of the point's normal equations at X: P null = camera 1.  Adds w J^T J to V (packed sym3), w J^T r to g and
// the robust cost to cost.
SFM_HD void view_points_terms(const RefineCam &K, const float *P, const float X[3], float x, float y, float huber, float V[6], float g[3], float &cost)
{
    float Y[3], r[2], Jy[6], J[6];
    if (P) register_to_cam(P, X, Y);
    else { Y[0] = X[0]; Y[1] = X[1]; Y[2] = X[2]; }
    refine_view(K, Y[0], Y[1], Y[2], x, y, r, Jy);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float j0 = Jy[3 * m], j1 = Jy[3 * m + 1], j2 = Jy[3 * m + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) J[3 * m + c] = P ? j0 * P[c] + j1 * P[3 + c] + j2 * P[6 + c] : Jy[3 * m + c];      // J R (refine_jacobian)
    }
    float rho;
    const float w = refine_huber(r[0], r[1], huber, rho);
    cost += rho;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int q = p; q < 3; ++q) V[sym3(p, q)] += w * (J[p] * J[q] + J[3 + p] * J[3 + q]);
        g[p] += w * (J[p] * r[0] + J[3 + p] * r[1]);
    }
}

// the robust cost of X over the views used (view 2 only with use2)
SFM_HD float view_points_cost(const ViewPointsCams &c, const float obs[6], bool use2, float huber, const float X[3])
{
    float Y[3], r[2], J[6], rho, cost = 0.0f;
    refine_view(c.K, X[0], X[1], X[2], obs[0], obs[1], r, J);
    refine_huber(r[0], r[1], huber, rho);
    cost += rho;
    if (use2) {
        register_to_cam(c.P2, X, Y);
        refine_view(c.K, Y[0], Y[1], Y[2], obs[2], obs[3], r, J);
        refine_huber(r[0], r[1], huber, rho);
        cost += rho;
    }
    register_to_cam(c.P3, X, Y);
    refine_view(c.K, Y[0], Y[1], Y[2], obs[4], obs[5], r, J);
    refine_huber(r[0], r[1], huber, rho);
    cost += rho;
    return cost;
}

// the point LM: X in / out
SFM_HD void view_points_lm(const ViewPointsCams &c, const float obs[6], bool use2, int max_iter, float huber, float min_rel, float lambda0, float X[3])
{
    const float cost0 = view_points_cost(c, obs, use2, huber, X);
    LmControl lm((double)lambda0, (double)cost0, (double)cost0, false);
    while (lm.running(max_iter)) {
        float V[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, g[3] = { 0.0f, 0.0f, 0.0f }, Vi[6], cost = 0.0f;
        view_points_terms(c.K, nullptr, X, obs[0], obs[1], huber, V, g, cost);
        if (use2) view_points_terms(c.K, c.P2, X, obs[2], obs[3], huber, V, g, cost);
        view_points_terms(c.K, c.P3, X, obs[4], obs[5], huber, V, g, cost);
        refine_damped_inverse3(V, (float)lm.lambda, Vi);
        float Xt[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) Xt[p] = X[p] - (Vi[sym3(p, 0)] * g[0] + Vi[sym3(p, 1)] * g[1] + Vi[sym3(p, 2)] * g[2]);
        if (!(isfinite(Xt[0]) && isfinite(Xt[1]) && isfinite(Xt[2]))) {      // a singular system: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        const float nc = view_points_cost(c, obs, use2, huber, Xt);
        bool stop;
        if (lm.tentative((double)nc, (double)nc, (double)min_rel, stop)) { X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2]; }
        if (stop) break;
    }
}

// The acceptance test at X and the error that is reported: every view used passes register_inlier; a new point (no view 2)
// additionally needs the rays from camera centres 1 (the origin) and 3 (-R3^T t3) to subtend at least the smallest parallax.
SFM_HD bool view_points_accept(const ViewPointsCams &c, const float obs[6], bool use2, float thr, float cos_min, const float X[3], float &err)
{
    const float P1[12] = { 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0 };
    bool ok = register_inlier(c.K, thr, P1, X, obs[0], obs[1]);
    float e2 = register_sq_error(c.K, P1, X, obs[0], obs[1]);
    if (use2) {
        ok = register_inlier(c.K, thr, c.P2, X, obs[2], obs[3]) && ok;
        e2 = fmaxf(e2, register_sq_error(c.K, c.P2, X, obs[2], obs[3]));
    }
    ok = register_inlier(c.K, thr, c.P3, X, obs[4], obs[5]) && ok;
    e2 = fmaxf(e2, register_sq_error(c.K, c.P3, X, obs[4], obs[5]));
    err = sqrtf(e2);
    if (!use2) {
        float b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = X[k] + (c.P3[k] * c.P3[9] + c.P3[3 + k] * c.P3[10] + c.P3[6 + k] * c.P3[11]);
        const float ab = X[0] * b[0] + X[1] * b[1] + X[2] * b[2];
        const float aa = X[0] * X[0] + X[1] * X[1] + X[2] * X[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
        ok = ok && ab < cos_min * sqrtf(aa * bb);
    }
    return ok;
}

// Everything behind the start point of a seen record: start (X / W of the input, or the DLT's result with start_ok), the LM,
// the acceptance test.  Returns the class, the output column and the error.
SFM_HD uint8_t view_points_finish(const ViewPointsCams &c, const ViewPointsArgs &a, const ViewPointsLane &L, bool start_ok, const float start[3],
                                  float out[4], float &err)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = L.Xin[k];
    err = __builtin_inff();
    if (!L.seen) return SFM_VP_UNSEEN;
    float X[3];
    if (L.usable) {
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = L.Xin[k] / L.Xin[3];
    } else {
        if (!start_ok) return SFM_VP_NEW_REJECTED;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = start[k];
    }
    view_points_lm(c, L.obs, L.usable, a.max_iter, a.huber, a.min_rel, a.lambda0, X);
    if (!view_points_accept(c, L.obs, L.usable, a.thr, a.cos_min, X, err)) return L.usable ? SFM_VP_KEPT : SFM_VP_NEW_REJECTED;
    out[0] = X[0]; out[1] = X[1]; out[2] = X[2]; out[3] = 1.0f;
    return L.usable ? SFM_VP_REFINED : SFM_VP_NEW;
}

// the plain form: one point from the records to its class
SFM_HD uint8_t view_points_one(const ViewPointsCams &c, const ViewPointsArgs &a, int j, float out[4], float &err)
{
    ViewPointsLane L;
    view_points_load(a, c.Kinv, j, L);
    float start[3] = { 0.0f, 0.0f, 0.0f };
    bool ok = false;
    if (L.seen && !L.usable) ok = view_points_dlt(L.obs[0], L.obs[1], L.obs[4], L.obs[5], c.P3, start);
    return view_points_finish(c, a, L, ok, start, out, err);
}

} // namespace sfm
