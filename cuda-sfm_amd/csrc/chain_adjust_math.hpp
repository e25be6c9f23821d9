// chain_adjust_math.hpp -- arithmetic of sfm_adjust_chain (chain_adjust.hip): one bundle adjustment over every camera and every
// track of a fused chain (the outputs of sfm_fuse_chain).
//
// Unknown cameras: one per pair p, its camera 2 (view p + 1), "block p".  Camera 1 of pair p is the segment's fixed [I|0] where
// root[p] == p and block p - 1 otherwise.  The root pair's block moves with the two-view refinement's 5 degrees of freedom
// (refine_jacobian, t on the unit sphere), every other block with the registration's 6 (register_jacobian); the 5-dof block is
// carried six wide with a zero sixth column, and the solver puts a unit row there.  A block's state is 18 floats: R (9), t (3)
// and, for a root block, the tangent basis b1, b2 at t.
// A track over the pairs h .. h + L - 1 has L + 1 consecutive views; its view v has the LOCAL block index v: block h - 1 + v (v = 0
// is the fixed camera where h is a root).  All tracks that start at head pair h therefore add into one partial band of W local
// blocks: the blocks (a, b), a <= b < W, of 36 values each, then b (6 W) and diag U (6 W).
// Per observation everything is fp32 (the rules of adjust_point_block and adjust_schur over a list of views); the sums over the
// tracks, the banded Cholesky and the steps are fp64.  Compiled as HIP host code by tests/hostcheck/chainadjustcheck.hip.
#pragma once
#include "adjust_math.hpp"                // kAdjMinView2 / kAdjMinView3: the smallest blocks
#include "fuse_math.hpp"

namespace sfm {

constexpr int kChainState = 18;
constexpr int kChainMaxViews = 16;                // the largest max_track_views
constexpr int kChainFixed = 0, kChainRoot = 1, kChainFree = 2;     // what a view's camera is

// the block of an observation: its pair's camera 2 is block `pair`; its camera 1 is block pair - 1, or the fixed root (-1)
SFM_HD int chain_block(int obs_cam, int root_of_pair)
{
    const int q = obs_cam >> 1;
    return (obs_cam & 1) ? q : (root_of_pair == q ? -1 : q - 1);
}

// the values of a head pair's partial band for tracks of at most W views
SFM_HD int chain_part_block(int W, int a, int b) { return 36 * (a * W - a * (a - 1) / 2 + (b - a)); }      // a <= b
SFM_HD int chain_part_b(int W) { return 36 * (W * (W + 1) / 2); }
SFM_HD int chain_part_u(int W) { return chain_part_b(W) + 6 * W; }
SFM_HD int chain_part_values(int W) { return chain_part_b(W) + 12 * W; }
// The wavefronts that share a head pair's tracks in the system pass, each with a partial band of its own in LDS: as many as fit
// 64 KiB, four at the most.  Wavefront w takes the rounds (of 64 tracks) w, w + waves, ...; the bands are added in wave order.
SFM_HD int chain_system_waves(int W) { const int w = 65536 / (8 * chain_part_values(W)); return w < 1 ? 1 : (w > 4 ? 4 : w); }

// one view of a track: its intrinsics, what its camera is, the camera's state (not read for the fixed one) and the observation
struct ChainView { RefineCam K; int kind; const float *S; float x, y; };

// r (2), Jp = d r / d X (2 x 3), Jc = d r / d camera (2 x 6; the fixed camera: zeros; a root block: column 5 is zero)
struct ChainJac { float r[2]; float Jp[6]; float Jc[12]; };

SFM_HD void chain_jacobian(const ChainView &v, const float X[3], ChainJac &o)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) o.Jc[k] = 0.0f;
    if (v.kind == kChainFixed) {
        refine_view(v.K, X[0], X[1], X[2], v.x, v.y, o.r, o.Jp);
    } else if (v.kind == kChainRoot) {
        RefinePose P;
#pragma unroll
        for (int k = 0; k < 9; ++k) P.R[k] = v.S[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { P.t[k] = v.S[9 + k]; P.b1[k] = v.S[12 + k]; P.b2[k] = v.S[15 + k]; }
        const float obs[4] = { 0.0f, 0.0f, v.x, v.y };     // (view 1 of refine_jacobian is not this view: its half is dropped)
        RefineJac J;
        refine_jacobian(v.K, P, obs, X, J);
        o.r[0] = J.r[2]; o.r[1] = J.r[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) o.Jp[k] = J.Jp[6 + k];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 5; ++i) o.Jc[6 * m + i] = J.Jc[5 * m + i];
    } else {
        register_jacobian(v.K, v.S, X, v.x, v.y, o.r, o.Jc);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float j0 = o.Jc[6 * m + 3], j1 = o.Jc[6 * m + 4], j2 = o.Jc[6 * m + 5];     // d r / d Y: the dt columns
#pragma unroll
            for (int a = 0; a < 3; ++a) o.Jp[3 * m + a] = j0 * v.S[a] + j1 * v.S[3 + a] + j2 * v.S[6 + a];      // J R
        }
    }
}

// residual only; returns the depth of X in the view
SFM_HD float chain_residual(const ChainView &v, const float X[3], float r[2])
{
    float Y[3] = { X[0], X[1], X[2] }, J[6];
    if (v.kind != kChainFixed) register_to_cam(v.S, X, Y);
    refine_view(v.K, Y[0], Y[1], Y[2], v.x, v.y, r, J);
    return Y[2];
}

// The used test of one track.  flag: its SFM_FUSE_*; count: its views; Xin: its input column; view(o): its views under the
// unified start cameras.  X: the start point X / W where used.
template <class Views>
SFM_HD bool chain_used(int flag, int count, int W, const float Xin[4], Views &&view, float X[3])
{
    if (flag != SFM_FUSE_REFINED || count > W || count < 2) return false;
    if (!(isfinite(Xin[0]) && isfinite(Xin[1]) && isfinite(Xin[2]) && isfinite(Xin[3]) && Xin[3] != 0.0f)) return false;
    X[0] = Xin[0] / Xin[3]; X[1] = Xin[1] / Xin[3]; X[2] = Xin[2] / Xin[3];
    if (!(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]))) return false;
    bool front = true;
    for (int o = 0; o < count; ++o) {
        const ChainView v = view(o);
        float r[2];
        front = chain_residual(v, X, r) > 0.0f && front;
    }
    return front;
}

// the robust cost and the squared error of X over the track's views
template <class Views>
SFM_HD void chain_cost(int count, Views &&view, float huber, const float X[3], float &cost, float &sq)
{
    cost = 0.0f; sq = 0.0f;
    for (int o = 0; o < count; ++o) {
        const ChainView v = view(o);
        float r[2], rho;
        chain_residual(v, X, r);
        refine_huber(r[0], r[1], huber, rho);
        cost += rho;
        sq += r[0] * r[0] + r[1] * r[1];
    }
}

// The point block over the list (adjust_point_block's sums, the views in order): Vi = (V + lambda diag V)^-1, gp = Jp^T W r
template <class Views>
SFM_HD void chain_point_block(int count, Views &&view, float huber, float lambda, const float X[3], float Vi[6], float gp[3])
{
    float V[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
    for (int o = 0; o < count; ++o) {
        const ChainView v = view(o);
        ChainJac J;
        chain_jacobian(v, X, J);
        float rho;
        const float w = refine_huber(J.r[0], J.r[1], huber, rho);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) V[sym3(a, b)] += w * (J.Jp[a] * J.Jp[b] + J.Jp[3 + a] * J.Jp[3 + b]);
            gp[a] += w * (J.Jp[a] * J.r[0] + J.Jp[3 + a] * J.r[1]);
        }
    }
    refine_damped_inverse3(V, lambda, Vi);
}

// one view's Wm = Jc^T W Jp (6 x 3 row-major) and its weight
SFM_HD float chain_view_w(const ChainJac &J, float huber, float Wm[18])
{
    float rho;
    const float w = refine_huber(J.r[0], J.r[1], huber, rho);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) Wm[3 * i + p] = w * (J.Jc[i] * J.Jp[p] + J.Jc[6 + i] * J.Jp[3 + p]);
    return w;
}

// view a's rows of adjust_schur: T = Wm Vi (6 x 3), bu = b (6: gc - T gp) then diag U (6)
SFM_HD void chain_row_terms(const ChainJac &J, float w, const float Wm[18], const float Vi[6], const float gp[3], float T[18], float bu[12])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int p = 0; p < 3; ++p) T[3 * i + p] = Wm[3 * i] * Vi[sym3(0, p)] + Wm[3 * i + 1] * Vi[sym3(1, p)] + Wm[3 * i + 2] * Vi[sym3(2, p)];
        const float gc = w * (J.Jc[i] * J.r[0] + J.Jc[6 + i] * J.r[1]);
        bu[i] = gc - (T[3 * i] * gp[0] + T[3 * i + 1] * gp[1] + T[3 * i + 2] * gp[2]);
        bu[6 + i] = w * (J.Jc[i] * J.Jc[i] + J.Jc[6 + i] * J.Jc[6 + i]);
    }
}

// the 6 x 6 block (view a's rows, view b's columns, row-major) of S = U - Wm Vi Wm^T; same: a == b (U is block diagonal)
SFM_HD void chain_block_terms(const ChainJac &Ja, float wa, const float Ta[18], const float Wb[18], bool same, float S[36])
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float u = same ? wa * (Ja.Jc[i] * Ja.Jc[k] + Ja.Jc[6 + i] * Ja.Jc[6 + k]) : 0.0f;
            S[6 * i + k] = u - (Ta[3 * i] * Wb[3 * k] + Ta[3 * i + 1] * Wb[3 * k + 1] + Ta[3 * i + 2] * Wb[3 * k + 2]);
        }
}

// Back substitution over the list: dp = -Vi (gp + sum over the views of Wm^T dc).  dc(o): the six floats of view o's block
// (not called for the fixed camera).
template <class Views, class Steps>
SFM_HD void chain_point_step(int count, Views &&view, Steps &&dc, float huber, const float X[3], const float Vi[6], const float gp[3], float dp[3])
{
    float s[3] = { 0.0f, 0.0f, 0.0f };
    for (int o = 0; o < count; ++o) {
        const ChainView v = view(o);
        if (v.kind == kChainFixed) continue;
        ChainJac J;
        float Wm[18];
        chain_jacobian(v, X, J);
        chain_view_w(J, huber, Wm);
        const float *d = dc(o);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) s[p] += Wm[3 * i + p] * d[i];
    }
    const float h[3] = { gp[0] + s[0], gp[1] + s[1], gp[2] + s[2] };
#pragma unroll
    for (int p = 0; p < 3; ++p) dp[p] = -(Vi[sym3(p, 0)] * h[0] + Vi[sym3(p, 1)] * h[1] + Vi[sym3(p, 2)] * h[2]);
}

// the largest pixel error of X over the views, +inf behind a camera.  P(o): the view's [R|t] (12), null for [I|0]
template <class Views, class Cams>
SFM_HD float chain_error(int count, Views &&view, Cams &&P, const float X[3])
{
    const float P1[12] = { 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0 };
    float e2 = 0.0f;
    for (int o = 0; o < count; ++o) {
        const ChainView v = view(o);
        const float *p = P(o);
        e2 = fmaxf(e2, register_sq_error(v.K, p ? p : P1, X, v.x, v.y));
    }
    return sqrtf(e2);
}

// a block's start state from its [R|t]: a root block's t is normalised (fp64) and gets its tangent basis
SFM_HD void chain_start_state(int kind, const float P[12], float s[kChainState])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = P[k];
#pragma unroll
    for (int k = 12; k < kChainState; ++k) s[k] = 0.0f;
    if (kind != kChainRoot) return;
    double t[3] = { P[9], P[10], P[11] }, b1[3], b2[3];
    const double nn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[9 + k] = (float)(t[k] / nn); t[k] = (double)s[9 + k]; }
    refine_tangent_basis(t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[12 + k] = (float)b1[k]; s[15 + k] = (float)b2[k]; }
}

// the tentative state o of the step dc (6; a root block reads 5) at the state s: fp64 updates, rounded once
SFM_HD void chain_camera_step(int kind, const double dc[6], const float s[kChainState], float o[kChainState])
{
    float P[12];
    refine_rotate(dc, s, P);
    if (kind == kChainRoot) {
        double t[3], nn = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) { t[q] = (double)s[9 + q] + (double)s[12 + q] * dc[3] + (double)s[15 + q] * dc[4]; nn += t[q] * t[q]; }
        nn = sqrt(nn);
#pragma unroll
        for (int q = 0; q < 3; ++q) P[9 + q] = (float)(t[q] / nn);
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) P[9 + q] = (float)((double)s[9 + q] + dc[3 + q]);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = P[k];
#pragma unroll
    for (int k = 12; k < kChainState; ++k) o[k] = 0.0f;
    if (kind == kChainRoot) {
        const double t[3] = { o[9], o[10], o[11] };
        double b1[3], b2[3];
        refine_tangent_basis(t, b1, b2);
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[12 + k] = (float)b1[k]; o[15 + k] = (float)b2[k]; }
    }
}

// ---- the block-banded system of one segment -------------------------------------------------------------------------------
// nb camera blocks, N = 6 nb scalar rows; block (p, q), p <= q < p + W, row-major 6 x 6 at B + 36 (p W + q - p).  The scalar
// Cholesky factor L (lower) is kept in place: L[r][j], r >= j, is the element (j, r) of the upper band.  Every sum is taken left
// to right over the columns; a pivot that is not > 0 is a failure, as in refine_cholesky.
SFM_HD size_t chain_band_at(int W, int r, int j)         // r >= j, r / 6 - j / 6 < W
{
    const int p = j / 6, q = r / 6;
    return 36 * ((size_t)p * W + (q - p)) + 6 * (j - 6 * p) + (r - 6 * q);
}
// the first column that can be non-zero in row r, the last row that can be non-zero in column j
SFM_HD int chain_band_first(int W, int r) { const int q = r / 6 - (W - 1); return q > 0 ? 6 * q : 0; }
SFM_HD int chain_band_last(int W, int N, int j) { const int r = 6 * (j / 6 + W) - 1; return r < N - 1 ? r : N - 1; }

// A[r][j] - sum over k < j of L[r][k] L[j][k], k ascending (r >= j)
SFM_HD double chain_band_dot(const double *B, int W, int r, int j)
{
    double s = B[chain_band_at(W, r, j)];
    for (int k = chain_band_first(W, r); k < j; ++k) s -= B[chain_band_at(W, r, k)] * B[chain_band_at(W, j, k)];
    return s;
}

// serial factorisation in place; false: not positive definite
SFM_HD bool chain_band_factor(double *B, int W, int N)
{
    for (int j = 0; j < N; ++j) {
        double d = chain_band_dot(B, W, j, j);
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        const int last = chain_band_last(W, N, j);
        for (int r = j + 1; r <= last; ++r) B[chain_band_at(W, r, j)] = chain_band_dot(B, W, r, j) / d;
        B[chain_band_at(W, j, j)] = d;
    }
    return true;
}

// L L^T x = rhs in place, column by column: forward with ascending columns, backward with descending ones
SFM_HD void chain_band_solve(const double *B, int W, int N, double *x)
{
    for (int j = 0; j < N; ++j) {
        x[j] /= B[chain_band_at(W, j, j)];
        const int last = chain_band_last(W, N, j);
        for (int r = j + 1; r <= last; ++r) x[r] -= B[chain_band_at(W, r, j)] * x[j];
    }
    for (int j = N - 1; j >= 0; --j) {
        x[j] /= B[chain_band_at(W, j, j)];
        for (int i = chain_band_first(W, j); i < j; ++i) x[i] -= B[chain_band_at(W, j, i)] * x[j];
    }
}

// The segment's band, right-hand side and diag U from the partial bands of its head pairs (part: chain_part_values(W) doubles per
// pair), head pairs in ascending order.  p0 .. p1 - 1: the segment's pairs.  One element each, so that the kernel can give every
// element a thread of its own.
SFM_HD double chain_reduce_block(const double *part, int W, int p0, int p1, int pl, int d, int e)      // block (pl, pl + d) local, value e
{
    const size_t stride = (size_t)chain_part_values(W);
    double s = 0.0;
    for (int a = W - 1 - d; a >= 0; --a) {
        const int h = p0 + pl + 1 - a;
        if (h < p0 || h >= p1) continue;
        s += part[stride * h + chain_part_block(W, a, a + d) + e];
    }
    return s;
}
SFM_HD double chain_reduce_row(const double *part, int W, int p0, int p1, int pl, int i, bool diag_u)
{
    const size_t stride = (size_t)chain_part_values(W);
    double s = 0.0;
    for (int a = W - 1; a >= 0; --a) {
        const int h = p0 + pl + 1 - a;
        if (h < p0 || h >= p1) continue;
        s += part[stride * h + (diag_u ? chain_part_u(W) : chain_part_b(W)) + 6 * a + i];
    }
    return s;
}

// the per-segment bookkeeping of the fixed launch sequence: what a block needs to know to fall through
struct ChainSeg {
    LmControl lm;
    int end;                              // one past the segment's last pair
    int stopped, go, cur;                 // the chain has ended; this iteration's solve succeeded; which state / point buffer is committed
    int tracks, obs, over;                // used tracks, their observations, tracks longer than W
    float initial_rms;
    SFM_HD ChainSeg() : lm(0.0, 0.0, 0.0, true), end(0), stopped(0), go(0), cur(0), tracks(0), obs(0), over(0), initial_rms(0.0f) {}
};

SFM_HD bool chain_running(const ChainSeg &s, int max_iter) { return !s.stopped && s.lm.running(max_iter); }

} // namespace sfm
