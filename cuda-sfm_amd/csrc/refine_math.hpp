// refine_math.hpp -- per-correspondence arithmetic of the two-view bundle adjustment (refine.hip).
//
// Camera 1 is [I|0]; camera 2 is [R|t] with X2 = R X + t and |t| = 1.  Parameters per correspondence: the point X (3, camera-1
// frame); shared: the pose increment dc = (omega (3), dt (2)) with R <- exp([omega]x) R and t <- normalize(t + b1 dt0 + b2 dt1),
// where b1, b2 span the tangent plane of the unit sphere at t.  Residuals are pixels: K2x2 (pi(Y) - x / z) per view with
// K2x2 = [[fx, s], [0, fy]] (the exact pixel error for any upper-triangular K).  Everything here is fp32; refine.hip sums the
// per-point terms in fp64.  At the end: what the one-block LM kernels (refine.hip, register.hip) share beyond the per-point terms --
// LmControl (damping schedule, accept test, stop rules, bookkeeping), the rotation update and the pose store.
// Compiled as HIP host code by tests/hostcheck/refinecheck.hip and lmcheck.hip for the CPU tests.
#pragma once
#include "device_math.hpp"
#include "../../include/sfm_amd.h"

namespace sfm {

struct RefineCam { float fx, s, fy; };
struct RefinePose { float R[9]; float t[3]; float b1[3]; float b2[3]; };   // R row-major; b1, b2: tangent basis at t

// Residual and Jacobians of one correspondence: r = (view 1 x, y, view 2 x, y); Jp = dr / dX (4 x 3 row-major);
// Jc = d r[2..3] / d (omega, dt) (2 x 5 row-major: view 1 does not see the pose); z1, z2 = depths in the two views.
struct RefineJac { float r[4]; float Jp[12]; float Jc[10]; float z1, z2; };

// pixel residual of one view at the camera-frame point (a, b, c) and d r / d (a, b, c) (2 x 3 row-major)
SFM_HD void refine_view(const RefineCam &K, float a, float b, float c, float u, float v, float r[2], float J[6])
{
    const float iz = 1.0f / c;
    const float px = a * iz, py = b * iz;
    const float ex = px - u, ey = py - v;
    r[0] = K.fx * ex + K.s * ey;
    r[1] = K.fy * ey;
    const float d02 = -px * iz, d12 = -py * iz;        // d pi / d (a, b, c) = [[iz, 0, -px iz], [0, iz, -py iz]]
    J[0] = K.fx * iz; J[1] = K.s * iz; J[2] = K.fx * d02 + K.s * d12;
    J[3] = 0.0f;      J[4] = K.fy * iz; J[5] = K.fy * d12;
}

// camera-2 frame: q = R X, Y = q + t
SFM_HD void refine_to_cam2(const RefinePose &P, const float X[3], float q[3], float Y[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = P.R[3 * a] * X[0] + P.R[3 * a + 1] * X[1] + P.R[3 * a + 2] * X[2];
        Y[a] = q[a] + P.t[a];
    }
}

// residuals only (the cost passes); obs = (x1 / z1, y1 / z1, x2 / z2, y2 / z2)
SFM_HD void refine_residual(const RefineCam &K, const RefinePose &P, const float obs[4], const float X[3], float r[4], float &z1, float &z2)
{
    float q[3], Y[3], J[6];
    refine_to_cam2(P, X, q, Y);
    refine_view(K, X[0], X[1], X[2], obs[0], obs[1], r, J);
    refine_view(K, Y[0], Y[1], Y[2], obs[2], obs[3], r + 2, J);
    z1 = X[2]; z2 = Y[2];
}

SFM_HD void refine_jacobian(const RefineCam &K, const RefinePose &P, const float obs[4], const float X[3], RefineJac &o)
{
    float q[3], Y[3], J1[6], J2[6];
    refine_to_cam2(P, X, q, Y);
    refine_view(K, X[0], X[1], X[2], obs[0], obs[1], o.r, J1);
    refine_view(K, Y[0], Y[1], Y[2], obs[2], obs[3], o.r + 2, J2);
    o.z1 = X[2]; o.z2 = Y[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) o.Jp[k] = J1[k];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float j0 = J2[3 * m], j1 = J2[3 * m + 1], j2 = J2[3 * m + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) o.Jp[6 + 3 * m + c] = j0 * P.R[c] + j1 * P.R[3 + c] + j2 * P.R[6 + c];     // J2 R
        // d Y / d omega = -[q]x, so row j of J2 times it is q x j
        o.Jc[5 * m + 0] = q[1] * j2 - q[2] * j1;
        o.Jc[5 * m + 1] = q[2] * j0 - q[0] * j2;
        o.Jc[5 * m + 2] = q[0] * j1 - q[1] * j0;
        o.Jc[5 * m + 3] = j0 * P.b1[0] + j1 * P.b1[1] + j2 * P.b1[2];
        o.Jc[5 * m + 4] = j0 * P.b2[0] + j1 * P.b2[1] + j2 * P.b2[2];
    }
}

// Huber on the 2-D residual of one view: rho(e) = e^2 for e <= h, 2 h e - h^2 above; IRLS weight rho'(e^2) = 1 or h / e.
// h = 0: plain least squares.
SFM_HD float refine_huber(float rx, float ry, float h, float &rho)
{
    const float e2 = rx * rx + ry * ry;
    if (h > 0.0f && e2 > h * h) {
        const float e = sqrtf(e2);
        rho = 2.0f * h * e - h * h;
        return h / e;
    }
    rho = e2;
    return 1.0f;
}

// packed upper triangle of a symmetric N x N, row-major (N = 5: 00 01 02 03 04 11 12 13 14 22 23 24 33 34 44; N = 3: 00 01 02 11 12 22)
template <int N>
SFM_HD constexpr int symn(int i, int j) { return i <= j ? i * N - i * (i - 1) / 2 + (j - i) : j * N - j * (j - 1) / 2 + (i - j); }
SFM_HD constexpr int sym5(int i, int j) { return symn<5>(i, j); }
SFM_HD constexpr int sym3(int i, int j) { return symn<3>(i, j); }

// Vi = (V + lambda diag V)^-1 of a packed symmetric 3 x 3 by the adjugate (not finite for a singular V): the point block of the
// two-view refinement and the whole system of a point-only refinement (view_points_math.hpp)
SFM_HD void refine_damped_inverse3(const float V[6], float lambda, float Vi[6])
{
    const float d = 1.0f + lambda;
    const float a = V[0] * d, b = V[1], c = V[2], e = V[3] * d, f = V[4], g = V[5] * d;
    const float A = e * g - f * f, B = c * f - b * g, C = b * f - c * e;
    const float det = a * A + b * B + c * C;
    const float id = 1.0f / det;
    Vi[0] = A * id; Vi[1] = B * id; Vi[2] = C * id;
    Vi[3] = (a * g - c * c) * id; Vi[4] = (b * c - a * f) * id; Vi[5] = (a * e - b * b) * id;
}

// The point block of the damped normal equations: Vi = (V + lambda diag V)^-1 (packed 3 x 3), Wm = Jc^T W Jp (5 x 3 row-major),
// gp = Jp^T W r (3).  w1, w2: the per-view weights.
SFM_HD void refine_point_block(const RefineJac &J, float w1, float w2, float lambda, float Vi[6], float Wm[15], float gp[3])
{
    float V[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const float v1 = J.Jp[a] * J.Jp[b] + J.Jp[3 + a] * J.Jp[3 + b];
            const float v2 = J.Jp[6 + a] * J.Jp[6 + b] + J.Jp[9 + a] * J.Jp[9 + b];
            V[sym3(a, b)] = w1 * v1 + w2 * v2;
        }
        gp[a] = w1 * (J.Jp[a] * J.r[0] + J.Jp[3 + a] * J.r[1]) + w2 * (J.Jp[6 + a] * J.r[2] + J.Jp[9 + a] * J.r[3]);
    }
    refine_damped_inverse3(V, lambda, Vi);
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) Wm[3 * i + p] = w2 * (J.Jc[i] * J.Jp[6 + p] + J.Jc[5 + i] * J.Jp[9 + p]);
}

// One point's share of the reduced camera system: S = U - Wm Vi Wm^T (packed 5 x 5), b = gc - Wm Vi gp, dU = diag U, where
// U = Jc^T W Jc and gc = Jc^T W r.  The pose step solves (sum S + lambda diag(sum dU)) dc = -sum b.  emit(q, value) receives
// S at q = 0..14, b at 15..19 and dU at 20..24, row by row (the kernel adds each into its fp64 sums as soon as it exists, so
// that Wm Vi never has to be held whole).
template <class Emit>
SFM_HD void refine_schur(const RefineJac &J, float w2, const float Vi[6], const float Wm[15], const float gp[3], Emit &&emit)
{
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        float T[3];                                      // row i of Wm Vi
#pragma unroll
        for (int p = 0; p < 3; ++p) T[p] = Wm[3 * i] * Vi[sym3(0, p)] + Wm[3 * i + 1] * Vi[sym3(1, p)] + Wm[3 * i + 2] * Vi[sym3(2, p)];
#pragma unroll
        for (int k = i; k < 5; ++k) {
            const float u = w2 * (J.Jc[i] * J.Jc[k] + J.Jc[5 + i] * J.Jc[5 + k]);
            if (k == i) emit(20 + i, u);
            emit(sym5(i, k), u - (T[0] * Wm[3 * k] + T[1] * Wm[3 * k + 1] + T[2] * Wm[3 * k + 2]));
        }
        const float gc = w2 * (J.Jc[i] * J.r[2] + J.Jc[5 + i] * J.r[3]);
        emit(15 + i, gc - (T[0] * gp[0] + T[1] * gp[1] + T[2] * gp[2]));
    }
}

// back substitution: dp = -Vi (gp + Wm^T dc)
SFM_HD void refine_point_step(const float Vi[6], const float Wm[15], const float gp[3], const float dc[5], float dp[3])
{
    float h[3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
        h[p] = gp[p] + (Wm[p] * dc[0] + Wm[3 + p] * dc[1] + Wm[6 + p] * dc[2] + Wm[9 + p] * dc[3] + Wm[12 + p] * dc[4]);
#pragma unroll
    for (int p = 0; p < 3; ++p) dp[p] = -(Vi[sym3(p, 0)] * h[0] + Vi[sym3(p, 1)] * h[1] + Vi[sym3(p, 2)] * h[2]);
}

// Tangent basis at t (fp64, one lane): e_k for the first smallest |t_k|, b1 = normalize(t x e_k), b2 = normalize(t x b1).
SFM_HD void refine_tangent_basis(const double t[3], double b1[3], double b2[3])
{
    int k = 0;
    if (fabs(t[1]) < fabs(t[k])) k = 1;
    if (fabs(t[2]) < fabs(t[k])) k = 2;
    const double e[3] = { k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0 };
    double c[3] = { t[1] * e[2] - t[2] * e[1], t[2] * e[0] - t[0] * e[2], t[0] * e[1] - t[1] * e[0] };
    double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    #pragma unroll
    for (int a = 0; a < 3; ++a) b1[a] = c[a] / n;
    c[0] = t[1] * b1[2] - t[2] * b1[1]; c[1] = t[2] * b1[0] - t[0] * b1[2]; c[2] = t[0] * b1[1] - t[1] * b1[0];
    n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    #pragma unroll
    for (int a = 0; a < 3; ++a) b2[a] = c[a] / n;
}

// exp([w]x) (Rodrigues, fp64, row-major)
SFM_HD void refine_expso3(const double w[3], double E[9])
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    const double A = th < 1e-4 ? 1.0 - th2 / 6.0 : sin(th) / th;
    const double B = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
    // [w]x^2 = w w^T - |w|^2 I
    E[0] = 1.0 + B * (w[0] * w[0] - th2); E[1] = -A * w[2] + B * w[0] * w[1]; E[2] = A * w[1] + B * w[0] * w[2];
    E[3] = A * w[2] + B * w[1] * w[0]; E[4] = 1.0 + B * (w[1] * w[1] - th2); E[5] = -A * w[0] + B * w[1] * w[2];
    E[6] = -A * w[1] + B * w[2] * w[0]; E[7] = A * w[0] + B * w[2] * w[1]; E[8] = 1.0 + B * (w[2] * w[2] - th2);
}

// Solves the damped N x N system S x = rhs in fp64 by Cholesky, in place: S (packed, symn<N>) becomes L, rhs becomes x.
// False if S is not positive definite.  N = 5: the reduced camera system of the two-view refinement; N = 6: the pose-only
// refinement of a registered view (register.hip).
template <int N>
SFM_HD bool refine_cholesky(double S[N * (N + 1) / 2], double x[N])
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = S[symn<N>(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= S[symn<N>(j, k)] * S[symn<N>(j, k)];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        S[symn<N>(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = S[symn<N>(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= S[symn<N>(i, k)] * S[symn<N>(j, k)];
            S[symn<N>(i, j)] = s / d;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k < i; ++k) x[i] -= S[symn<N>(i, k)] * x[k];
        x[i] /= S[symn<N>(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < N; ++k) x[i] -= S[symn<N>(k, i)] * x[k];
        x[i] /= S[symn<N>(i, i)];
    }
    return true;
}

SFM_HD bool refine_solve5(double S[15], double x[5]) { return refine_cholesky<5>(S, x); }

// The control of a Levenberg-Marquardt chain, the same for every solver here: ten times the damping after a failed solve or a
// rejected step, a tenth after an accepted one; a step is accepted when it lowers the cost; the chain ends after max_iterations,
// when an accepted step lowered the cost by less than min_rel of it (CONVERGED), or when lambda has passed 1e16.  Every lane of
// the block keeps its own copy and feeds it the same block-uniform values; the report is filled from lane 0's.  No device
// intrinsics: tests/test_lm_control_host.py replays event sequences through the host build.
struct LmControl {
    double lambda, cost, sq;              // damping; cost and sum of squared residuals of the committed state
    int iters, accepted, status;          // status: SFM_REFINE_*

    SFM_HD LmControl(double lambda0, double cost0, double sq0, bool degenerate)
        : lambda(lambda0), cost(cost0), sq(sq0), iters(0), accepted(0), status(degenerate ? SFM_REFINE_DEGENERATE : SFM_REFINE_MAX_ITER) {}

    SFM_HD bool running(int max_iterations) const { return status != SFM_REFINE_DEGENERATE && iters < max_iterations; }

    // false: lambda has passed 1e16, the chain gives up
    SFM_HD bool more_damping() { lambda *= 10.0; return !(lambda > 1e16); }

    // this iteration's system was not positive definite; false: stop
    SFM_HD bool solve_failed() { ++iters; return more_damping(); }

    // this iteration's tentative state has cost nc and squared sum nsq; returns whether the caller commits it, stop: the chain ends
    // (after the commit)
    SFM_HD bool tentative(double nc, double nsq, double min_rel, bool &stop)
    {
        ++iters;
        if (nc < cost) {
            const double rel = (cost - nc) / cost;
            cost = nc; sq = nsq;
            ++accepted;
            lambda /= 10.0;
            stop = !(rel >= min_rel);
            if (stop) status = SFM_REFINE_CONVERGED;
            return true;
        }
        stop = !more_damping();
        return false;
    }
};

// one lane: Rn = exp([w]x) R, the product in fp64 (R, Rn row-major 3 x 3).  Rn is a local array that the kernels copy to LDS
// themselves: with the stores to LDS in here, refine_solve_kernel (239 of its 256 VGPRs) came out with 52 bytes of scratch.
SFM_HD void refine_rotate(const double w[3], const float R[9], float Rn[9])
{
    double E[9];
    refine_expso3(w, E);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Rn[3 * r + c] = (float)(E[3 * r] * (double)R[c] + E[3 * r + 1] * (double)R[3 + c] + E[3 * r + 2] * (double)R[6 + c]);
}

// [R|t] (R 9 row-major, then t 3) -> 4 x 4 row-major
SFM_HD void refine_store_pose(const float *P, float *o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[4 * r + c] = P[3 * r + c];
        o[4 * r + 3] = P[9 + r];
    }
    o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
}

} // namespace sfm
