// adjust_math.hpp -- per-point arithmetic of the three-view bundle adjustment (adjust.hip): sfm_adjust_view / sfm_adjust_views.
//
// Cameras: 1 = [I|0] (fixed), 2 = [R|t] with |t| = 1, 3 = [R3|t3].  Parameters: the camera step dc (11) = camera 2's (omega (3),
// dt (2)) with R <- exp([omega]x) R and t <- normalize(t + b1 dt0 + b2 dt1) -- the two-view refinement's update (refine_math.hpp)
// -- then camera 3's (omega (3), dt (3)) with R3 <- exp([omega]x) R3 and t3 <- t3 + dt -- the registration's (register_math.hpp);
// and the point X (3) of every used record.  A record carries view bits (kAdjView1 / 2 / 3): view 1 always, views 2 and 3 where
// they see it.  Residuals, Jacobians and Huber weights come from refine_jacobian / refine_view / register_jacobian / refine_huber;
// a view that does not see the point contributes zeros, so every point emits the same 88 values of the reduced camera system
// (S 11 x 11 packed, b, diag U) and the block of cameras 2 x 3 is zero unless both see it.
// Everything per point is fp32; the callers sum in fp64.  Compiled as HIP host code by tests/hostcheck/adjustcheck.hip.
#pragma once
#include "device_math.hpp"
#include "refine_math.hpp"
#include "register_math.hpp"
#include "view_points_math.hpp"

namespace sfm {

constexpr int kAdjCam = 11;                       // 5 (camera 2) + 6 (camera 3)
constexpr int kAdjS = kAdjCam * (kAdjCam + 1) / 2;    // 66
constexpr int kAdjB = kAdjS;                      // b at 66..76
constexpr int kAdjU = kAdjS + kAdjCam;            // diag U at 77..87
constexpr int kAdjValues = kAdjS + 2 * kAdjCam;   // 88
constexpr int kAdjMinView2 = 16;                  // = kRefineMinPoints (refine.hip)
constexpr int kAdjMinView3 = 6;                   // the registration's smallest inlier count
constexpr int kAdjView1 = 1, kAdjView2 = 2, kAdjView3 = 4;
// the state of both cameras: R2 (9), t2 (3), b1 (3), b2 (3) -- a RefinePose -- then R3 (9), t3 (3)
constexpr int kAdjPoseWords = 30;

struct AdjustCams { RefinePose P2; float P3[12]; };

SFM_HD void adjust_load_cams(const float *s, AdjustCams &c)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) c.P2.R[k] = s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.P2.t[k] = s[9 + k]; c.P2.b1[k] = s[12 + k]; c.P2.b2[k] = s[15 + k]; }
#pragma unroll
    for (int k = 0; k < 12; ++k) c.P3[k] = s[18 + k];
}

// r: views 1, 2, 3; Jp = d r / d X (6 x 3 row-major); Jc2 = d r[2..3] / d camera 2 (2 x 5); Jc3 = d r[4..5] / d camera 3 (2 x 6)
struct AdjustJac { float r[6]; float Jp[18]; float Jc2[10]; float Jc3[12]; };

// The view bits of one record.  flag: SFM_VP_* of sfm_triangulate_view; used2: the record has an observation in view 2;
// Xin: the input column; P2, P3: the start poses as [R|t] (12).  0 = not used.
SFM_HD int adjust_view_bits(int flag, bool used2, const float Xin[4], const float P2[12], const float P3[12])
{
    const bool see3 = flag == SFM_VP_NEW || flag == SFM_VP_REFINED;
    const bool see2 = used2 && (flag == SFM_VP_UNSEEN || flag == SFM_VP_REFINED || flag == SFM_VP_KEPT);
    if (!(see2 || see3)) return 0;
    if (!view_points_usable(true, Xin)) return 0;
    const float X[3] = { Xin[0] / Xin[3], Xin[1] / Xin[3], Xin[2] / Xin[3] };
    float Y[3];
    if (see2) { register_to_cam(P2, X, Y); if (!(Y[2] > 0.0f)) return 0; }
    if (see3) { register_to_cam(P3, X, Y); if (!(Y[2] > 0.0f)) return 0; }
    return kAdjView1 | (see2 ? kAdjView2 : 0) | (see3 ? kAdjView3 : 0);
}

SFM_HD void adjust_jacobian(const RefineCam &K, const AdjustCams &c, const float obs[6], const float X[3], int bits, AdjustJac &o)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) o.r[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 18; ++k) o.Jp[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 10; ++k) o.Jc2[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; ++k) o.Jc3[k] = 0.0f;
    if (bits & kAdjView2) {
        RefineJac J;
        refine_jacobian(K, c.P2, obs, X, J);
#pragma unroll
        for (int k = 0; k < 4; ++k) o.r[k] = J.r[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) o.Jp[k] = J.Jp[k];
#pragma unroll
        for (int k = 0; k < 10; ++k) o.Jc2[k] = J.Jc[k];
    } else {
        refine_view(K, X[0], X[1], X[2], obs[0], obs[1], o.r, o.Jp);
    }
    if (bits & kAdjView3) {
        register_jacobian(K, c.P3, X, obs[4], obs[5], o.r + 4, o.Jc3);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float j0 = o.Jc3[6 * m + 3], j1 = o.Jc3[6 * m + 4], j2 = o.Jc3[6 * m + 5];     // d r / d Y: the dt columns
#pragma unroll
            for (int a = 0; a < 3; ++a) o.Jp[12 + 3 * m + a] = j0 * c.P3[a] + j1 * c.P3[3 + a] + j2 * c.P3[6 + a];      // J R3
        }
    }
}

// the Huber weights of the three views (0 for a view that does not see the point); adds the views' robust cost and squared error
SFM_HD void adjust_weights(const float r[6], int bits, float huber, float w[3], float &cost, float &sq)
{
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        w[v] = 0.0f;
        if (bits & (1 << v)) {
            float rho;
            w[v] = refine_huber(r[2 * v], r[2 * v + 1], huber, rho);
            cost += rho;
            sq += r[2 * v] * r[2 * v] + r[2 * v + 1] * r[2 * v + 1];
        }
    }
}

// residuals only (the cost passes): the robust cost and the squared error of X over its views
SFM_HD void adjust_cost(const RefineCam &K, const AdjustCams &c, const float obs[6], const float X[3], int bits, float huber, float &cost, float &sq)
{
    float r[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, J[6], Y[3], q[3], w[3];
    refine_view(K, X[0], X[1], X[2], obs[0], obs[1], r, J);
    if (bits & kAdjView2) {
        refine_to_cam2(c.P2, X, q, Y);
        refine_view(K, Y[0], Y[1], Y[2], obs[2], obs[3], r + 2, J);
    }
    if (bits & kAdjView3) {
        float J3[12];
        register_jacobian(K, c.P3, X, obs[4], obs[5], r + 4, J3);
    }
    cost = 0.0f; sq = 0.0f;
    adjust_weights(r, bits, huber, w, cost, sq);
}

// column i of the camera Jacobian in row m of its own view (camera 2: i < 5, camera 3: i >= 5)
SFM_HD float adjust_jc(const AdjustJac &J, int i, int m) { return i < 5 ? J.Jc2[5 * m + i] : J.Jc3[6 * m + (i - 5)]; }

// The point block: Vi = (V + lambda diag V)^-1 (packed 3 x 3), Wm = Jc^T W Jp (11 x 3 row-major), gp = Jp^T W r.
SFM_HD void adjust_point_block(const AdjustJac &J, const float w[3], float lambda, float Vi[6], float Wm[3 * kAdjCam], float gp[3])
{
    float V[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = a; b < 3; ++b) {
            float s = 0.0f;
#pragma unroll
            for (int v = 0; v < 3; ++v) s += w[v] * (J.Jp[6 * v + a] * J.Jp[6 * v + b] + J.Jp[6 * v + 3 + a] * J.Jp[6 * v + 3 + b]);
            V[sym3(a, b)] = s;
        }
        float g = 0.0f;
#pragma unroll
        for (int v = 0; v < 3; ++v) g += w[v] * (J.Jp[6 * v + a] * J.r[2 * v] + J.Jp[6 * v + 3 + a] * J.r[2 * v + 1]);
        gp[a] = g;
    }
    refine_damped_inverse3(V, lambda, Vi);
#pragma unroll
    for (int i = 0; i < kAdjCam; ++i) {
        const int v = i < 5 ? 1 : 2;
#pragma unroll
        for (int p = 0; p < 3; ++p) Wm[3 * i + p] = w[v] * (adjust_jc(J, i, 0) * J.Jp[6 * v + p] + adjust_jc(J, i, 1) * J.Jp[6 * v + 3 + p]);
    }
}

// One point's share of the reduced camera system (refine_schur's, 11 wide): emit(q, value) receives S = U - Wm Vi Wm^T at
// q = symn<11>(i, k), b = gc - Wm Vi gp at kAdjB + i and diag U at kAdjU + i, row by row.  U is block diagonal: a residual of
// view 2 does not depend on camera 3.
template <class Emit>
SFM_HD void adjust_schur(const AdjustJac &J, const float w[3], const float Vi[6], const float Wm[3 * kAdjCam], const float gp[3], Emit &&emit)
{
#pragma unroll
    for (int i = 0; i < kAdjCam; ++i) {
        const int v = i < 5 ? 1 : 2;
        float T[3];                                      // row i of Wm Vi
#pragma unroll
        for (int p = 0; p < 3; ++p) T[p] = Wm[3 * i] * Vi[sym3(0, p)] + Wm[3 * i + 1] * Vi[sym3(1, p)] + Wm[3 * i + 2] * Vi[sym3(2, p)];
#pragma unroll
        for (int k = i; k < kAdjCam; ++k) {
            const bool same = (k < 5) == (i < 5);
            const float u = same ? w[v] * (adjust_jc(J, i, 0) * adjust_jc(J, k, 0) + adjust_jc(J, i, 1) * adjust_jc(J, k, 1)) : 0.0f;
            if (k == i) emit(kAdjU + i, u);
            emit(symn<kAdjCam>(i, k), u - (T[0] * Wm[3 * k] + T[1] * Wm[3 * k + 1] + T[2] * Wm[3 * k + 2]));
        }
        const float gc = w[v] * (adjust_jc(J, i, 0) * J.r[2 * v] + adjust_jc(J, i, 1) * J.r[2 * v + 1]);
        emit(kAdjB + i, gc - (T[0] * gp[0] + T[1] * gp[1] + T[2] * gp[2]));
    }
}

// back substitution: dp = -Vi (gp + Wm^T dc)
SFM_HD void adjust_point_step(const float Vi[6], const float Wm[3 * kAdjCam], const float gp[3], const float dc[kAdjCam], float dp[3])
{
    float h[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < kAdjCam; ++i) s += Wm[3 * i + p] * dc[i];
        h[p] = gp[p] + s;
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) dp[p] = -(Vi[sym3(p, 0)] * h[0] + Vi[sym3(p, 1)] * h[1] + Vi[sym3(p, 2)] * h[2]);
}

// one lane: the start state from the two [R|t] (12 each; t2 as given) with camera 2's tangent basis
SFM_HD void adjust_start_state(const float P2[12], const float P3[12], float s[kAdjPoseWords])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) { s[k] = P2[k]; s[18 + k] = P3[k]; }
    const double t[3] = { s[9], s[10], s[11] };
    double b1[3], b2[3];
    refine_tangent_basis(t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[12 + k] = (float)b1[k]; s[15 + k] = (float)b2[k]; }
}

// one lane: the tentative state o of the camera step dc at the state s (fp64 updates, rounded to float once)
SFM_HD void adjust_camera_step(const double dc[kAdjCam], const float s[kAdjPoseWords], float o[kAdjPoseWords])
{
    float P2[12], P3[12];
    refine_rotate(dc, s, P2);
    double t[3], nn = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) { t[q] = (double)s[9 + q] + (double)s[12 + q] * dc[3] + (double)s[15 + q] * dc[4]; nn += t[q] * t[q]; }
    nn = sqrt(nn);
#pragma unroll
    for (int q = 0; q < 3; ++q) P2[9 + q] = (float)(t[q] / nn);
    refine_rotate(dc + 5, s + 18, P3);
#pragma unroll
    for (int q = 0; q < 3; ++q) P3[9 + q] = (float)((double)s[27 + q] + dc[8 + q]);
    adjust_start_state(P2, P3, o);
}

// the largest pixel error of X over its views, +inf where a view that sees it has it behind the camera
SFM_HD float adjust_error(const RefineCam &K, const float P2[12], const float P3[12], const float obs[6], const float X[3], int bits)
{
    const float P1[12] = { 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0 };
    float e2 = register_sq_error(K, P1, X, obs[0], obs[1]);
    bool front = X[2] > 0.0f;
    float Y[3];
    if (bits & kAdjView2) {
        register_to_cam(P2, X, Y);
        front = front && Y[2] > 0.0f;
        e2 = fmaxf(e2, register_sq_error(K, P2, X, obs[2], obs[3]));
    }
    if (bits & kAdjView3) {
        register_to_cam(P3, X, Y);
        front = front && Y[2] > 0.0f;
        e2 = fmaxf(e2, register_sq_error(K, P3, X, obs[4], obs[5]));
    }
    return front ? sqrtf(e2) : __builtin_inff();
}

} // namespace sfm
