// ring_math.hpp -- arithmetic of sfm_close_ring (ring.hip): the drift of a ring of aligned pairs measured and spread over its links.
//
// sfm_fuse_chain's conventions (fuse_math.hpp): link i = (s, R, t) carries pair i's frame into pair i + 1 mod k's, F_i carries pair
// i's frame into pair 0's, F_0 = I and F_{i+1} = F_i o L_i^-1 by fuse_invert / fuse_compose in fp64.  The drift D = F_k is what a
// point of pair 0 becomes once it has gone round the ring.  The correction is D^-1, and it is INTERPOLATED, not the links' own
// logarithms averaged: with (sigma, w, t_c) = (ln s, axis-angle, t) of D^-1 and weights alpha_0 = 0 <= ... <= alpha_k = 1,
// B_i = (exp(alpha_i sigma), exp(alpha_i [w]x), alpha_i t_c) and B_k = D^-1 ITSELF, so the closed frames F'_i = B_i o F_i end at
// F'_k = D^-1 o D = I whatever the accuracy of the logarithm: the corrected links L'_i = F'_{i+1}^-1 o F'_i close to rounding.
// (sigma, w, t_c) is not the Sim(3) logarithm -- t_c is the translation itself, not V^-1 t -- and needs not be: any path from I
// to D^-1 closes the ring; this one moves scale, rotation and translation in proportion to the weight behind each link.
//
// Everything is fp64 with + - * /, sqrt, exp, log, sin, cos and atan2, rounded to fp32 once; the host build
// (tests/hostcheck/ringcheck.hip) runs the same functions, so the two differ only where a library function of the two builds
// does, before that one rounding.
#pragma once
#include <math.h>
#include "fuse_math.hpp"
#include "register_math.hpp"

namespace sfm {

constexpr int kRingBlock = 256;           // links per round of the walk; records per block and round of the seam kernel
constexpr int kRingMaxBlocks = 1024;      // blocks of the seam kernel: block b takes the rounds b, b + blocks, ...
constexpr int kRingSums = 7;              // per frame (link, open, closed) the sum of squared errors and the number of finite ones; |S|

SFM_HD int ring_seam_blocks(int n) { const int b = (n + kRingBlock - 1) / kRingBlock; return b < 1 ? 1 : (b > kRingMaxBlocks ? kRingMaxBlocks : b); }

// One link of the ring.  The pointers are device memory in the kernels and host memory in the host build.
struct RingLink {
    const float *sim;                     // 13
    const sfm_align_report *report;
    double weight;                        // the caller's, where sfm_ring_params.weights is given
};

// what the walk leaves for the two kernels behind it
struct RingHead {
    double corr[7];                       // sigma, w (3), t_c (3) of D^-1
    double Dinv[kFuseSim];
    int32_t status, pad;
};

// the inverse of a similarity in fp64: fuse_invert's formula on doubles
SFM_HD void ring_invert(const double S[kFuseSim], double inv[kFuseSim])
{
    const double s = S[0];
    inv[0] = 1.0 / s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) inv[1 + 3 * a + b] = S[1 + 3 * b + a];
        inv[10 + a] = -((S[1 + a] * S[10] + S[4 + a] * S[11]) + S[7 + a] * S[12]) / s;
    }
}

// The rotation's axis-angle from the antisymmetric part: v = axis sin(angle), angle = atan2(|v|, (tr - 1) / 2), w = v angle / |v|.
// A vanishing |v| returns v itself (angle / |v| -> 1; the gate keeps the angle far from pi, where v vanishes again).
SFM_HD double ring_rot_log(const double R[9], double w[3])
{
    const double v[3] = { 0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1]) };
    const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double angle = atan2(nv, 0.5 * (((R[0] + R[4]) + R[8]) - 1.0));
    const double f = nv > 0.0 ? angle / nv : 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = f * v[a];
    return angle;
}

// exp([w]x) = I + a [w]x + b [w]x^2 with a = sin(th) / th, b = 2 sin^2(th / 2) / th^2 (Rodrigues); th = 0: I + [w]x
SFM_HD void ring_rot_exp(const double w[3], double R[9])
{
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(t2);
    double a = 1.0, b = 0.5;
    if (th > 0.0) {
        const double h = sin(0.5 * th);
        a = sin(th) / th;
        b = 2.0 * h * h / t2;
    }
    R[0] = 1.0 - b * (w[1] * w[1] + w[2] * w[2]);
    R[4] = 1.0 - b * (w[0] * w[0] + w[2] * w[2]);
    R[8] = 1.0 - b * (w[0] * w[0] + w[1] * w[1]);
    R[1] = b * w[0] * w[1] - a * w[2]; R[3] = b * w[0] * w[1] + a * w[2];
    R[2] = b * w[0] * w[2] + a * w[1]; R[6] = b * w[0] * w[2] - a * w[1];
    R[5] = b * w[1] * w[2] - a * w[0]; R[7] = b * w[1] * w[2] + a * w[0];
}

// B(alpha) = (exp(alpha sigma), exp(alpha [w]x), alpha t_c); alpha = 0 gives the identity exactly
SFM_HD void ring_interpolate(const double corr[7], double alpha, double B[kFuseSim])
{
    const double w[3] = { alpha * corr[1], alpha * corr[2], alpha * corr[3] };
    B[0] = exp(alpha * corr[0]);
    ring_rot_exp(w, B + 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) B[10 + a] = alpha * corr[4 + a];
}

// the weight of a link from its report
SFM_HD double ring_weight(int num_inliers) { return 1.0 / (double)(num_inliers > 1 ? num_inliers : 1); }

// alpha[0 .. k] from the k weights: normalised in fp64, summed in link order, alpha[k] = 1 exactly.  Serial.
SFM_HD void ring_alphas(const double *w, int k, double *alpha)
{
    double total = 0.0;
    for (int i = 0; i < k; ++i) total += w[i];
    double run = 0.0;
    alpha[0] = 0.0;
    for (int i = 0; i + 1 < k; ++i) { run += w[i] / total; alpha[i + 1] = run; }
    alpha[k] = 1.0;
}

// The drift D = F_k of a ring whose links are all valid: the correction's parameters, D^-1, the report's three drift numbers and
// the status.  A drift that is not finite fails the gates.
SFM_HD void ring_drift(const double D[kFuseSim], float max_rotation_rad, float max_log_scale, RingHead &h, float drift[3])
{
    ring_invert(D, h.Dinv);
    h.corr[0] = log(h.Dinv[0]);
    const double angle = ring_rot_log(h.Dinv + 1, h.corr + 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) h.corr[4 + a] = h.Dinv[10 + a];
    drift[0] = (float)-h.corr[0];
    drift[1] = (float)angle;
    drift[2] = (float)sqrt((D[10] * D[10] + D[11] * D[11]) + D[12] * D[12]);
    const bool ok = angle <= (double)max_rotation_rad && fabs(h.corr[0]) <= (double)max_log_scale;
    h.status = ok ? SFM_RING_CLOSED : SFM_RING_REJECTED;
}

// Link i of a closed ring: the closed frame F'_i = B_i o F_i and the corrected link F'_{i+1}^-1 o F'_i, rounded once.
// last: i + 1 == k, where B_{i+1} is D^-1 itself.
SFM_HD void ring_correct(const RingHead &h, double alpha0, double alpha1, bool last, const double F0[kFuseSim], const double F1[kFuseSim],
                         float link[kFuseSim], float frame[kFuseSim])
{
    double B[kFuseSim], G0[kFuseSim], G1[kFuseSim], inv[kFuseSim], L[kFuseSim];
    ring_interpolate(h.corr, alpha0, B);
    fuse_compose(B, F0, G0);
    if (last) {
#pragma unroll
        for (int q = 0; q < kFuseSim; ++q) B[q] = h.Dinv[q];
    } else ring_interpolate(h.corr, alpha1, B);
    fuse_compose(B, F1, G1);
    ring_invert(G1, inv);
    fuse_compose(inv, G0, L);
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) { link[q] = (float)L[q]; frame[q] = (float)G0[q]; }
}

// One record of pair k - 1 at the seam: its point carried into pair 0's frame by the measured closing link, the open and the closed
// frame, each held against the record's own X1 observation (view 0) through the pair's K under [I|0].  err: the three pixel
// errors (+inf: not usable, or behind the camera); v: the record's terms of the kRingSums sums.
SFM_HD void ring_seam_record(const FusePair &p, int j, float thr, const float *const frames[3], float err[3], double v[kRingSums])
{
    const float inf = __builtin_inff();
    const float P[12] = { 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int q = 0; q < kRingSums; ++q) v[q] = 0.0;
    err[0] = inf; err[1] = inf; err[2] = inf;
    float X[4];
    if (!fuse_live(p, j, X)) return;
    RefineCam K;
    K.fx = p.K[0]; K.s = p.K[1]; K.fy = p.K[4];
    const float z = p.X1[2 * (size_t)p.ld + j];
    const float x = p.X1[j] / z, y = p.X1[(size_t)p.ld + j] / z;
    float e2[3];
    bool member = false;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        float Y[3];
        fuse_carry(frames[f], X, Y);
        if (f == 0) member = register_inlier(K, thr, P, Y, x, y);
        e2[f] = register_sq_error(K, P, Y, x, y);
        err[f] = sqrtf(e2[f]);
    }
    if (!member) return;
    v[6] = 1.0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        if (isfinite(e2[f])) { v[2 * f] = (double)e2[f]; v[2 * f + 1] = 1.0; }
    }
}

// the report's seam block from the kRingSums totals
SFM_HD void ring_seam_report(const double t[kRingSums], sfm_ring_report &r)
{
    const int S = (int)t[6];
    r.seam_count = S;
    r.seam_lost_open = S - (int)t[3];
    r.seam_lost_closed = S - (int)t[5];
    r.seam_rms_link_px = t[1] > 0.0 ? (float)sqrt(t[0] / t[1]) : 0.0f;
    r.seam_rms_open_px = t[3] > 0.0 ? (float)sqrt(t[2] / t[3]) : 0.0f;
    r.seam_rms_closed_px = t[5] > 0.0 ? (float)sqrt(t[4] / t[5]) : 0.0f;
}

} // namespace sfm
