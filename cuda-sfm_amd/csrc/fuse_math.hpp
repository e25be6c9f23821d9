// fuse_math.hpp -- arithmetic of sfm_fuse_chain (fuse.hip): a chain of aligned pairs fused into tracks and one point per track.
//
// Pair i = (view i, view i + 1) lives in its own gauge; link i = (s, R, t) carries pair i's frame into pair i + 1's
// (X_{i+1} = s R X_i + t, align_math.hpp).  A valid link joins the two pairs into one segment; an invalid one cuts the chain
// and pair i + 1 becomes the root of a new segment.  Pair i's frame F_i = (s, R, t) carries its points into its segment's
// root frame: the identity for a root, else F_{i-1} composed with the inverse of link i - 1, in fp64, rounded once to fp32.
// Node (i, j) is record j of pair i; it is live when its point passes view_points_usable.  Record j of pair i proposes the
// edge (i, j) -> (i + 1, index[j]); where several propose the same target the smallest 64-bit key wins, so the tracks are
// simple paths.  A track's point starts at the mean of its path's points carried into the root frame and is refined by
// view_points_lm's Levenberg-Marquardt over the track's list of views, every view through view_points_terms with its own
// camera [R|t] of the root frame.
//
// Everything here is fp32 (the composition: fp64) with + - * /, sqrtf and fmaf only where written, bounded iteration counts
// and no contraction, so the host build (tests/hostcheck/fusecheck.hip) and the gfx950 build give the same bits under the
// Makefile's flags.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "device_math.hpp"
#include "refine_math.hpp"
#include "register_math.hpp"
#include "view_points_math.hpp"

namespace sfm {

constexpr int kFuseSim = 13;              // s, R (9, row-major), t (3)
constexpr int kFuseCams = 24;             // per pair: camera 1 [R|t] (R 9 row-major, t 3), then camera 2
constexpr int kFuseBlock = 256;           // nodes per block of the node kernels: a block never holds nodes of two pairs

// One pair of the chain and the link behind it.  Every pointer is device memory in the kernels and host memory in the host build.
struct FusePair {
    const float *points;                  // 4 x n
    const uint8_t *valid;                 // n, or null: every point
    const float *X0, *X1;                 // the pair's normalised observations, 3 x ld
    const float *K;                       // 9
    const float *pose;                    // camera 2: pose_rows == 3: R (9) then t (3); 4: a 4 x 4 row-major matrix
    int pose_rows;
    int n, ld;
    int offset;                           // nodes of the pairs before this one
    int block0;                           // node blocks of the pairs before this one
    // link i: this pair -> the next (unused in the last pair)
    const int32_t *index;                 // n
    const float *sim;                     // 13
    const uint8_t *inlier;                // n
    const float *err;                     // n
    const sfm_align_report *report;
};

SFM_HD int fuse_blocks(int n) { return (n + kFuseBlock - 1) / kFuseBlock; }

// a link joins its two pairs when it is not degenerate, all 13 floats are finite and s > 0
SFM_HD bool fuse_link_valid(int status, const float sim[kFuseSim])
{
    bool ok = status != SFM_REFINE_DEGENERATE;
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) ok = ok && isfinite(sim[q]);
    return ok && sim[0] > 0.0f;
}

SFM_HD void fuse_identity(double F[kFuseSim])
{
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) F[q] = 0.0;
    F[0] = 1.0; F[1] = 1.0; F[5] = 1.0; F[9] = 1.0;
}

// The inverse of a link, X_i = (1 / s) R^T (X_{i+1} - t), as (1 / s, R^T, -(R^T t) / s) in fp64: needs no other link, so the kernel
// takes it off the serial chain
SFM_HD void fuse_invert(const float link[kFuseSim], double inv[kFuseSim])
{
    const double s = (double)link[0];
    double R[9], t[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = (double)link[1 + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = (double)link[10 + q];
    inv[0] = 1.0 / s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) inv[1 + 3 * a + b] = R[3 * b + a];
        inv[10 + a] = -((R[a] * t[0] + R[3 + a] * t[1]) + R[6 + a] * t[2]) / s;
    }
}

// F_{i+1} = F_i o link^-1 from the inverse link (si, Ri, ti): s0 si, R0 Ri, s0 (R0 ti) + t0 -- with fuse_invert the operations of
// the host's chain composition in its order, every sum taken left to right.  Written per element, so that the kernel can give
// every element of the running frame a lane of its own: element c reads the scale, row `row` of R0 (and t0[row] for a
// translation element) and three values y of the inverse link.
SFM_HD int fuse_compose_row(int c) { return c >= 10 ? c - 10 : (c >= 1 ? (c - 1) / 3 : 0); }
SFM_HD int fuse_compose_operand(int c, int k)         // index into the inverse link of y[k], k = 0, 1, 2
{
    return c >= 10 ? 10 + k : (c >= 1 ? 1 + 3 * k + (c - 1) % 3 : 0);
}
SFM_HD double fuse_compose_element(int c, double s0, const double x[3], double t0, const double y[3])
{
    if (c == 0) return s0 * y[0];
    const double dot = (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
    return c >= 10 ? s0 * dot + t0 : dot;
}
SFM_HD void fuse_compose(const double F[kFuseSim], const double inv[kFuseSim], double out[kFuseSim])
{
#pragma unroll
    for (int c = 0; c < kFuseSim; ++c) {
        const int row = fuse_compose_row(c);
        const double x[3] = { F[1 + 3 * row], F[2 + 3 * row], F[3 + 3 * row] };
        const double y[3] = { inv[fuse_compose_operand(c, 0)], inv[fuse_compose_operand(c, 1)], inv[fuse_compose_operand(c, 2)] };
        out[c] = fuse_compose_element(c, F[0], x, F[10 + row], y);
    }
}

// The pair's two cameras in the root frame, from its rounded frame (s, R, t) and its camera 2 [R2|t2]: camera 1 = [R^T | -R^T t],
// camera 2 = [R2 R^T | s t2 - R2 R^T t] (a projection does not see the positive scale: no 1 / s)
SFM_HD void fuse_cameras(const float F[kFuseSim], const float P2[12], float cams[kFuseCams])
{
    const float s = F[0];
    const float *R = F + 1, *t = F + 10;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) cams[3 * a + b] = R[3 * b + a];
        cams[9 + a] = -((R[a] * t[0] + R[3 + a] * t[1]) + R[6 + a] * t[2]);
    }
    float *M = cams + 12;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) M[3 * a + b] = (P2[3 * a] * R[3 * b] + P2[3 * a + 1] * R[3 * b + 1]) + P2[3 * a + 2] * R[3 * b + 2];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) M[9 + a] = s * P2[9 + a] - ((M[3 * a] * t[0] + M[3 * a + 1] * t[1]) + M[3 * a + 2] * t[2]);
}

// node (pair, j) is live: its point passes the registration's point test
SFM_HD bool fuse_live(const FusePair &p, int j, float X[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) X[c] = p.points[(size_t)c * p.n + j];
    return view_points_usable(!p.valid || p.valid[j] != 0, X);
}

// record j of a pair proposes the edge to record m of the next pair (both ends are live: the caller's test)
SFM_HD bool fuse_proposes(bool link_ok, uint8_t inlier, int m, int n_next, float err)
{
    return link_ok && inlier != 0 && m >= 0 && m < n_next && isfinite(err);
}

// the smallest key wins a target: the smallest error, then the lowest record
SFM_HD unsigned long long fuse_key(float err, int j)
{
    return ((unsigned long long)__builtin_bit_cast(uint32_t, err) << 32) | (unsigned long long)(uint32_t)j;
}
constexpr unsigned long long kFuseNoKey = ~0ull;

// the target of record j's edge, or -1 where it proposes none (both ends live included); key: its key
SFM_HD int fuse_edge(const FusePair &p, const FusePair &next, bool link_ok, int j, unsigned long long &key)
{
    const int m = p.index[j];
    const float e = p.err[j];
    key = fuse_key(e, j);
    if (!fuse_proposes(link_ok, p.inlier[j], m, next.n, e)) return -1;
    float X[4];
    if (!fuse_live(p, j, X) || !fuse_live(next, m, X)) return -1;
    return m;
}

SFM_HD bool fuse_link_ok(const FusePair &p)
{
    float sim[kFuseSim];
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) sim[q] = p.sim[q];
    return fuse_link_valid(p.report->status, sim);
}

// a point of a pair carried into the root frame: X / W, then s R X + t
SFM_HD void fuse_carry(const float F[kFuseSim], const float X[4], float Y[3])
{
    const float x0 = X[0] / X[3], x1 = X[1] / X[3], x2 = X[2] / X[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) Y[a] = F[0] * ((F[1 + 3 * a] * x0 + F[2 + 3 * a] * x1) + F[3 + 3 * a] * x2) + F[10 + a];
}

// one view of a track: its intrinsics, its camera of the root frame (12 floats) and the observation
struct FuseView { RefineCam K; const float *P; float x, y; };

// observation `rec` of a pair: slot 0 = the X0 column, slot 1 = the X1 column, dehomogenised as view_points_load does
SFM_HD FuseView fuse_view(const FusePair &p, const float *cams, int pair, int slot, int rec)
{
    const float *X = slot ? p.X1 : p.X0;
    const float z = X[2 * (size_t)p.ld + rec];
    FuseView v;
    v.K.fx = p.K[0]; v.K.s = p.K[1]; v.K.fy = p.K[4];
    v.P = cams + (size_t)kFuseCams * pair + 12 * slot;
    v.x = X[rec] / z; v.y = X[(size_t)p.ld + rec] / z;
    return v;
}

// the robust cost of X over the track's views: the list is walked, nothing is kept per view
template <class Views>
SFM_HD float fuse_cost(int count, Views &&view, float huber, const float X[3])
{
    float cost = 0.0f;
    for (int o = 0; o < count; ++o) {
        const FuseView v = view(o);
        float Y[3], r[2], J[6], rho;
        register_to_cam(v.P, X, Y);
        refine_view(v.K, Y[0], Y[1], Y[2], v.x, v.y, r, J);
        refine_huber(r[0], r[1], huber, rho);
        cost += rho;
    }
    return cost;
}

// view_points_lm over a list of views: X in / out
template <class Views>
SFM_HD void fuse_lm(int count, Views &&view, int max_iter, float huber, float min_rel, float lambda0, float X[3])
{
    const float cost0 = fuse_cost(count, view, huber, X);
    LmControl lm((double)lambda0, (double)cost0, (double)cost0, false);
    while (lm.running(max_iter)) {
        float V[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, g[3] = { 0.0f, 0.0f, 0.0f }, Vi[6], cost = 0.0f;
        for (int o = 0; o < count; ++o) {
            const FuseView v = view(o);
            view_points_terms(v.K, v.P, X, v.x, v.y, huber, V, g, cost);
        }
        refine_damped_inverse3(V, (float)lm.lambda, Vi);
        float Xt[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) Xt[p] = X[p] - (Vi[sym3(p, 0)] * g[0] + Vi[sym3(p, 1)] * g[1] + Vi[sym3(p, 2)] * g[2]);
        if (!(isfinite(Xt[0]) && isfinite(Xt[1]) && isfinite(Xt[2]))) {      // a singular system: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        const float nc = fuse_cost(count, view, huber, Xt);
        bool stop;
        if (lm.tentative((double)nc, (double)nc, (double)min_rel, stop)) { X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2]; }
        if (stop) break;
    }
}

// the acceptance test at X: every view passes register_inlier; err: the square root of the largest register_sq_error
template <class Views>
SFM_HD bool fuse_accept(int count, Views &&view, float thr, const float X[3], float &err)
{
    bool ok = true;
    float e2 = 0.0f;
    for (int o = 0; o < count; ++o) {
        const FuseView v = view(o);
        ok = register_inlier(v.K, thr, v.P, X, v.x, v.y) && ok;
        e2 = fmaxf(e2, register_sq_error(v.K, v.P, X, v.x, v.y));
    }
    err = sqrtf(e2);
    return ok;
}

// one track from its start point to its class, its column and its error
template <class Views>
SFM_HD uint8_t fuse_point(int count, Views &&view, const float start[3], const sfm_fuse_params &p, float out[4], float &err)
{
    float X[3] = { start[0], start[1], start[2] };
    fuse_lm(count, view, p.max_iterations, p.huber_px, p.min_rel_decrease, p.initial_lambda, X);
    const bool ok = fuse_accept(count, view, p.threshold_px, X, err);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ok ? X[c] : start[c];
    out[3] = 1.0f;
    return ok ? SFM_FUSE_REFINED : SFM_FUSE_KEPT;
}

} // namespace sfm
