// register_math.hpp -- arithmetic of the view registration (register.hip): P3P by Lambda Twist on a 4-point sample, the
// inlier test shared by the scoring kernel and the final mask, and the per-candidate terms of the pose-only refinement.
//
// The pair's gauge: camera 1 = [I|0], camera 2 = [R|t] with |t| = 1.  A registered view has the pose P = [R3|t3] (R3 row-major,
// 9 floats, then t3: 12 floats) with X3 = R3 X + t3; |t3| carries the pair's scale.  A candidate is a 3-D point X (camera-1 frame,
// fp32, X / W) and its normalised observation (x, y) in the new view.
//
// Everything here is fp32 with + - * /, sqrtf and fmaf only where written, fixed iteration counts and no contraction, so the
// host build (tests/hostcheck/registercheck.hip) and the gfx950 build give the same bits under the Makefile's flags.
//
// Lambda Twist: M. Persson, K. Nordberg, "Lambda Twist: An Accurate Fast Robust Perspective Three Point (P3P) Solver",
// ECCV 2018.
#pragma once
#include "device_math.hpp"
#include "refine_math.hpp"

namespace sfm {

constexpr int kP3PCubicIters = 12;        // Newton steps on the cubic for gamma (from the paper's start point)
constexpr int kP3PRefineIters = 5;        // Gauss-Newton steps on (lambda1, lambda2, lambda3)

// Y = R X + t in the order of refine_to_cam2
SFM_HD void register_to_cam(const float P[12], const float X[3], float Y[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) Y[a] = (P[3 * a] * X[0] + P[3 * a + 1] * X[1] + P[3 * a + 2] * X[2]) + P[9 + a];
}

// The inlier test of the registration, division-free: with Y = R X + t and e = (Y.x - x Y.z, Y.y - y Y.z),
// inlier iff Y.z > 0 and (fx e.x + s e.y)^2 + (fy e.y)^2 < (threshold_px Y.z)^2, i.e. the pixel error under K is below the
// threshold for a point in front of the camera.
SFM_HD bool register_inlier(const RefineCam &K, float thr, const float P[12], const float X[3], float x, float y)
{
    float Y[3];
    register_to_cam(P, X, Y);
    const float ex = Y[0] - x * Y[2], ey = Y[1] - y * Y[2];
    const float a = K.fx * ex + K.s * ey, b = K.fy * ey, l = thr * Y[2];
    return Y[2] > 0.0f && a * a + b * b < l * l;
}

// squared pixel error of one candidate under P (refine_view's residual), +inf behind the camera or where it is not finite
SFM_HD float register_sq_error(const RefineCam &K, const float P[12], const float X[3], float x, float y)
{
    float Y[3], r[2], J[6];
    register_to_cam(P, X, Y);
    refine_view(K, Y[0], Y[1], Y[2], x, y, r, J);
    const float e2 = r[0] * r[0] + r[1] * r[1];
    return (Y[2] > 0.0f && e2 <= 3.0e38f) ? e2 : __builtin_inff();
}

// roots of x^2 + b x + c (false, and zeros, when they are complex); the larger-magnitude root first, the other as c / r1
SFM_HD bool p3p_root2(float b, float c, float &r1, float &r2)
{
    const float v = b * b - 4.0f * c;
    if (!(v >= 0.0f)) { r1 = 0.0f; r2 = 0.0f; return false; }
    const float y = sqrtf(v);
    r1 = b < 0.0f ? 0.5f * (-b + y) : 0.5f * (-b - y);
    r2 = c / r1;
    return true;
}

// one real root of x^3 + b x^2 + c x + d: the paper's start point, then kP3PCubicIters Newton steps (a step that is not finite
// is skipped)
SFM_HD float p3p_cubic(float b, float c, float d)
{
    float r0;
    if (b * b >= 3.0f * c) {                              // two stationary points
        const float v = sqrtf(b * b - 3.0f * c);
        const float t1 = (-b - v) / 3.0f;
        const float k1 = ((t1 + b) * t1 + c) * t1 + d;
        if (k1 > 0.0f) {
            r0 = t1 - sqrtf(-k1 / (3.0f * t1 + b));       // leftmost root of the quadratic model at t1
        } else {
            const float t2 = (-b + v) / 3.0f;
            const float k2 = ((t2 + b) * t2 + c) * t2 + d;
            r0 = t2 + sqrtf(-k2 / (3.0f * t2 + b));       // rightmost root of the quadratic model at t2
        }
    } else {
        r0 = -b / 3.0f;
        if (fabsf((3.0f * r0 + 2.0f * b) * r0 + c) < 1e-4f) r0 += 1.0f;
    }
    for (int i = 0; i < kP3PCubicIters; ++i) {
        const float fx = ((r0 + b) * r0 + c) * r0 + d;
        const float fpx = (3.0f * r0 + 2.0f * b) * r0 + c;
        const float r = r0 - fx / fpx;
        if (isfinite(r)) r0 = r;
    }
    return r0;
}

// Eigen-decomposition of the symmetric 3 x 3 M (row-major) with one eigenvalue known to be 0: eigenvalues L0, L1 with
// |L0| >= |L1|; V row-major with the eigenvectors of L0, L1, 0 as its columns.
SFM_HD void p3p_eig_known0(const float M[9], float V[9], float &L0, float &L1)
{
    float v3[3] = { M[1] * M[5] - M[2] * M[4], M[2] * M[3] - M[5] * M[0], M[4] * M[0] - M[1] * M[3] };
    const float n3 = sqrtf(v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v3[k] = v3[k] / n3;
    const float x01 = M[1] * M[1];
    const float b = -M[0] - M[4] - M[8];
    const float c = -x01 - M[2] * M[2] - M[5] * M[5] + M[0] * (M[4] + M[8]) + M[4] * M[8];
    const float disc = fmaxf(b * b - 4.0f * c, 0.0f);    // real for a symmetric M; rounding may push it below 0
    const float y = sqrtf(disc);
    float e1 = b < 0.0f ? 0.5f * (-b + y) : 0.5f * (-b - y);
    float e2 = c / e1;
    if (fabsf(e1) < fabsf(e2)) { const float s = e1; e1 = e2; e2 = s; }
    L0 = e1; L1 = e2;
    const float mx0011 = -M[0] * M[4];
    const float prec0 = M[1] * M[5] - M[2] * M[4];
    const float prec1 = M[1] * M[2] - M[0] * M[5];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float e = q == 0 ? e1 : e2;
        const float tmp = 1.0f / (e * (M[0] + M[4]) + mx0011 - e * e + x01);
        float a1 = -(e * M[2] + prec0) * tmp;
        float a2 = -(e * M[5] + prec1) * tmp;
        const float rn = 1.0f / sqrtf(a1 * a1 + a2 * a2 + 1.0f);
        a1 *= rn; a2 *= rn;
        V[q] = a1; V[3 + q] = a2; V[6 + q] = rn;
    }
    V[2] = v3[0]; V[5] = v3[1]; V[8] = v3[2];
}

// inverse of a row-major 3 x 3 by the adjugate (not finite for a singular A)
SFM_HD void p3p_inv3(const float A[9], float B[9])
{
    const float c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const float det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    B[0] = c00 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
    B[3] = c01 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
    B[6] = c02 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}

// Lambda Twist P3P.  y1..y3: unit bearings, x1..x3: the 3-D points (none for collinear or coincident points).  Every solution, in a fixed order ((+v, tau1), (+v, tau2),
// (-v, tau1), (-v, tau2)), goes to emit(R[9], t[3]) after kP3PRefineIters Gauss-Newton steps on the depths.
template <class Emit>
SFM_HD void p3p_lambda_twist(const float y1[3], const float y2[3], const float y3[3],
                             const float x1[3], const float x2[3], const float x3[3], Emit &&emit)
{
    const float b12 = -2.0f * (y1[0] * y2[0] + y1[1] * y2[1] + y1[2] * y2[2]);
    const float b13 = -2.0f * (y1[0] * y3[0] + y1[1] * y3[1] + y1[2] * y3[2]);
    const float b23 = -2.0f * (y2[0] * y3[0] + y2[1] * y3[1] + y2[2] * y3[2]);
    float d12[3], d13[3], d23[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d12[k] = x1[k] - x2[k]; d13[k] = x1[k] - x3[k]; d23[k] = x2[k] - x3[k]; }
    const float nx[3] = { d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0] };
    const float a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const float a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const float a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    // collinear or coincident points (sin^2 of the angle at x1 below 1e-8): no pose
    if (!(nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2] > 1e-8f * (a12 * a13))) return;

    // the cubic in gamma: D1 - gamma D2 is degenerate (D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23)
    const float c31 = -0.5f * b13, c23 = -0.5f * b23, c12 = -0.5f * b12;
    const float blob = c12 * c23 * c31 - 1.0f;
    const float s31 = 1.0f - c31 * c31, s23 = 1.0f - c23 * c23, s12 = 1.0f - c12 * c12;
    const float p3 = a13 * (a23 * s31 - a13 * s23);
    const float p2 = 2.0f * blob * a23 * a13 + a13 * (2.0f * a12 + a13) * s23 + a23 * (a23 - a12) * s31;
    const float p1 = a23 * (a13 - a23) * s12 - a12 * a12 * s23 - 2.0f * a12 * (blob * a23 + a13 * s23);
    const float p0 = a12 * (a12 * s23 - a23 * s12);
    const float g = p3p_cubic(p2 / p3, p1 / p3, p0 / p3);

    const float A[9] = {
        a23 * (1.0f - g),             (a23 * b12) * 0.5f,             (a23 * b13 * g) * -0.5f,
        (a23 * b12) * 0.5f,           a23 - a12 + a13 * g,            b23 * (a13 * g - a12) * 0.5f,
        (a23 * b13 * g) * -0.5f,      b23 * (a13 * g - a12) * 0.5f,   g * (a13 - a23) - a12 };
    float V[9], L0, L1;
    p3p_eig_known0(A, V, L0, L1);
    const float v = sqrtf(fmaxf(0.0f, -L1 / L0));

    // pose from the depths: R [d12 d13 d12 x d13] = [yd1 yd2 yd1 x yd2], t = l1 y1 - R x1
    const float X[9] = { d12[0], d13[0], nx[0], d12[1], d13[1], nx[1], d12[2], d13[2], nx[2] };
    float Xi[9];
    p3p_inv3(X, Xi);

#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        const float s = sg == 0 ? v : -v;
        const float w2 = 1.0f / (s * V[1] - V[0]);
        const float w0 = (V[3] - s * V[4]) * w2;
        const float w1 = (V[6] - s * V[7]) * w2;
        const float a = 1.0f / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
        const float b = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0f * w0 * w1 * (a12 - a13)) * a;
        const float c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a;
        float tau1, tau2;
        const bool real = p3p_root2(b, c, tau1, tau2);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float tau = q == 0 ? tau1 : tau2;
            if (!(real && tau > 0.0f)) continue;
            const float d = a23 / (tau * (b23 + tau) + 1.0f);
            if (!(d > 0.0f)) continue;
            float l2 = sqrtf(d);
            float l3 = tau * l2;
            float l1 = w0 * l2 + w1 * l3;
            if (!(l1 >= 0.0f)) continue;
            for (int it = 0; it < kP3PRefineIters; ++it) {
                const float r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12;
                const float r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13;
                const float r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23;
                // J = [[ja, jb, 0], [jc, 0, je], [0, jf, jg]]: d (r1, r2, r3) / d (l1, l2, l3)
                const float ja = 2.0f * l1 + b12 * l2, jb = 2.0f * l2 + b12 * l1;
                const float jc = 2.0f * l1 + b13 * l3, je = 2.0f * l3 + b13 * l1;
                const float jf = 2.0f * l2 + b23 * l3, jg = 2.0f * l3 + b23 * l2;
                const float det = -ja * je * jf - jb * jc * jg;
                const float n1 = l1 - (-je * jf * r1 - jb * jg * r2 + jb * je * r3) / det;
                const float n2 = l2 - (-jc * jg * r1 + ja * jg * r2 - ja * je * r3) / det;
                const float n3 = l3 - (jc * jf * r1 - ja * jf * r2 - jb * jc * r3) / det;
                if (isfinite(n1) && isfinite(n2) && isfinite(n3)) { l1 = n1; l2 = n2; l3 = n3; }
            }
            float ry1[3], ry2[3], ry3[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { ry1[k] = y1[k] * l1; ry2[k] = y2[k] * l2; ry3[k] = y3[k] * l3; }
            float yd1[3], yd2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { yd1[k] = ry1[k] - ry2[k]; yd2[k] = ry1[k] - ry3[k]; }
            const float ny[3] = { yd1[1] * yd2[2] - yd1[2] * yd2[1], yd1[2] * yd2[0] - yd1[0] * yd2[2], yd1[0] * yd2[1] - yd1[1] * yd2[0] };
            const float Y[9] = { yd1[0], yd2[0], ny[0], yd1[1], yd2[1], ny[1], yd1[2], yd2[2], ny[2] };
            float R[9], t[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) R[3 * r + cc] = Y[3 * r] * Xi[cc] + Y[3 * r + 1] * Xi[3 + cc] + Y[3 * r + 2] * Xi[6 + cc];
#pragma unroll
            for (int r = 0; r < 3; ++r) t[r] = ry1[r] - (R[3 * r] * x1[0] + R[3 * r + 1] * x1[1] + R[3 * r + 2] * x1[2]);
            emit(R, t);
        }
    }
}

// unit bearing of a normalised observation
SFM_HD void register_bearing(float x, float y, float b[3])
{
    const float n = sqrtf(x * x + y * y + 1.0f);
    b[0] = x / n; b[1] = y / n; b[2] = 1.0f / n;
}

// One RANSAC hypothesis over the m candidates (Xc: X / W, Oc: observation): sample4, Lambda Twist on the first three samples,
// the solution with the smallest squared pixel error of the 4th (first on ties).  False, and a zero pose (which no candidate
// passes: Y.z = 0), for a degenerate sample: m < 4, collinear or coincident points, no real root, the 4th point behind every
// solution, or a pose that is not finite.
SFM_HD bool register_hypothesis(uint32_t seed, uint32_t hyp, int m, const RefineCam &K, const float4 *Xc, const float2 *Oc, float P[12])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = 0.0f;
    if (m < 4) return false;
    int idx[4];
    sample4(seed, hyp, m, idx);
    float x[4][3], y[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4 X = Xc[idx[s]];
        const float2 o = Oc[idx[s]];
        x[s][0] = X.x; x[s][1] = X.y; x[s][2] = X.z;
        if (s < 3) register_bearing(o.x, o.y, y[s]);
        else { y[3][0] = o.x; y[3][1] = o.y; y[3][2] = 1.0f; }
    }
    float best = __builtin_inff();
    p3p_lambda_twist(y[0], y[1], y[2], x[0], x[1], x[2], [&](const float R[9], const float t[3]) {
        float Q[12];
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) { Q[k] = R[k]; fin = fin && isfinite(R[k]); }
#pragma unroll
        for (int k = 0; k < 3; ++k) { Q[9 + k] = t[k]; fin = fin && isfinite(t[k]); }
        const float e2 = register_sq_error(K, Q, x[3], y[3][0], y[3][1]);
        if (fin && e2 < best) {
            best = e2;
#pragma unroll
            for (int k = 0; k < 12; ++k) P[k] = Q[k];
        }
    });
    return best < __builtin_inff();
}

// Residual r (2, pixels, refine_view's) and d r / d (omega, dt) (2 x 6 row-major) of one candidate under P, for the update
// R <- exp([omega]x) R, t <- t + dt (d Y / d omega = -[R X]x, d Y / d t = I).  Returns Y.z.
SFM_HD float register_jacobian(const RefineCam &K, const float P[12], const float X[3], float x, float y, float r[2], float J[12])
{
    float q[3], Y[3], Jy[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = P[3 * a] * X[0] + P[3 * a + 1] * X[1] + P[3 * a + 2] * X[2];
        Y[a] = q[a] + P[9 + a];
    }
    refine_view(K, Y[0], Y[1], Y[2], x, y, r, Jy);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float j0 = Jy[3 * m], j1 = Jy[3 * m + 1], j2 = Jy[3 * m + 2];
        J[6 * m + 0] = q[1] * j2 - q[2] * j1;
        J[6 * m + 1] = q[2] * j0 - q[0] * j2;
        J[6 * m + 2] = q[0] * j1 - q[1] * j0;
        J[6 * m + 3] = j0; J[6 * m + 4] = j1; J[6 * m + 5] = j2;
    }
    return Y[2];
}

// One candidate's share of the weighted normal equations: emit(q, value) receives J^T w J (packed, symn<6>) at q = 0..20 and
// J^T w r at 21..26.
template <class Emit>
SFM_HD void register_terms(const float r[2], const float J[12], float w, Emit &&emit)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = i; k < 6; ++k) emit(symn<6>(i, k), w * (J[i] * J[k] + J[6 + i] * J[6 + k]));
        emit(21 + i, w * (J[i] * r[0] + J[6 + i] * r[1]));
    }
}

} // namespace sfm
