// tests/hostcheck/adjustcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_adjust_view (cuda-sfm_amd/csrc/adjust_math.hpp) as HIP *host* code: the per-point terms for the
// Jacobian and Schur tests, and a serial driver of the whole chain -- the same header functions and LmControl as adjust.hip, the
// fp64 sums taken in compact order -- that the CPU tests hold to the fp64 twin (tests/adjust_reference.py) and the GPU tests
// compare the device's outputs with.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/adjust_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

extern "C" {

// state: kAdjPoseWords (R2, t2, b1, b2, R3, t3).  out: r (6), Jp (18), Jc2 (10), Jc3 (12)
void adj_jacobian(const float cam[3], const float state[30], const float obs[6], const float X[3], int bits, float out[46])
{
    const RefineCam K = { cam[0], cam[1], cam[2] };
    AdjustCams c;
    adjust_load_cams(state, c);
    AdjustJac J;
    adjust_jacobian(K, c, obs, X, bits, J);
    memcpy(out, J.r, 6 * 4); memcpy(out + 6, J.Jp, 18 * 4); memcpy(out + 24, J.Jc2, 10 * 4); memcpy(out + 34, J.Jc3, 12 * 4);
}

// the cost pass of one point: cost, squared error
void adj_cost(const float cam[3], const float state[30], const float obs[6], const float X[3], int bits, float huber, float out[2])
{
    const RefineCam K = { cam[0], cam[1], cam[2] };
    AdjustCams c;
    adjust_load_cams(state, c);
    adjust_cost(K, c, obs, X, bits, huber, out[0], out[1]);
}

// w (3), Vi (6), Wm (33), gp (3), then the 88 system values; dc (11) -> dp (3) behind them: 136 floats
void adj_terms(const float cam[3], const float state[30], const float obs[6], const float X[3], int bits, float huber, float lambda,
               const float dc[11], float out[136])
{
    const RefineCam K = { cam[0], cam[1], cam[2] };
    AdjustCams c;
    adjust_load_cams(state, c);
    AdjustJac J;
    adjust_jacobian(K, c, obs, X, bits, J);
    float cost = 0.0f, sq = 0.0f;
    adjust_weights(J.r, bits, huber, out, cost, sq);
    adjust_point_block(J, out, lambda, out + 3, out + 9, out + 42);
    float *sys = out + 45;
    adjust_schur(J, out, out + 3, out + 9, out + 42, [&](int q, float v) { sys[q] = v; });
    adjust_point_step(out + 3, out + 9, out + 42, dc, out + 133);
}

// one camera step: state (30), dc (11, double) -> state (30)
void adj_camera_step(const double dc[11], const float state[30], float out[30]) { adjust_camera_step(dc, state, out); }

// What sfm_adjust_view computes, serially.  sift: n records; X0, X1: 3 x ld; points: 4 x n; flags, used2: n; poses: 24; p: the
// call's parameters (its pointers are not read).  Outputs as sfm_adjust_out.
void adj_run(int n, int ld, const sfm_sift_point *sift, const float *X0, const float *X1, const float Kf[9], const float Kinv[9],
             const float *points, const uint8_t *flags, const uint8_t *used2, const float poses[24], const sfm_adjust_params *p,
             float *out_poses, float *out_points, uint8_t *out_views, float *out_err, sfm_adjust_report *rep)
{
    const RefineCam K = { Kf[0], Kf[1], Kf[4] };
    const float *P2s = poses, *P3s = poses + 12;
    struct Pt { float obs[6]; float X[3]; int bits; int j; };
    std::vector<Pt> pts;
    std::vector<float> obs_all((size_t)6 * n);
    for (int j = 0; j < n; ++j) {
        float Xin[4];
        for (int c = 0; c < 4; ++c) Xin[c] = points[(size_t)c * n + j];
        const int bits = adjust_view_bits(flags[j], used2[j] != 0, Xin, P2s, P3s);
        out_views[j] = (uint8_t)bits;
        const float z1 = X0[2 * (size_t)ld + j], z2 = X1[2 * (size_t)ld + j];
        float *o = &obs_all[(size_t)6 * j];
        o[0] = X0[j] / z1; o[1] = X0[(size_t)ld + j] / z1; o[2] = X1[j] / z2; o[3] = X1[(size_t)ld + j] / z2;
        const float u = sift[j].match_xpos, v = sift[j].match_ypos;
        float x[3];
        for (int r = 0; r < 3; ++r) x[r] = fmaf(Kinv[3 * r + 2], 1.0f, fmaf(Kinv[3 * r + 1], v, Kinv[3 * r] * u));
        o[4] = x[0] / x[2]; o[5] = x[1] / x[2];
        if (bits) {
            Pt q;
            memcpy(q.obs, o, sizeof(q.obs));
            for (int c = 0; c < 3; ++c) q.X[c] = Xin[c] / Xin[3];
            q.bits = bits; q.j = j;
            pts.push_back(q);
        }
    }
    const int m = (int)pts.size();
    float state[kAdjPoseWords], trial[kAdjPoseWords];
    adjust_start_state(P2s, P3s, state);
    AdjustCams P;
    adjust_load_cams(state, P);
    int n2 = 0, n3 = 0;
    double c0 = 0.0, q0 = 0.0;
    for (const Pt &q : pts) {
        float cost, sq;
        adjust_cost(K, P, q.obs, q.X, q.bits, p->huber_px, cost, sq);
        c0 += (double)cost; q0 += (double)sq;
        n2 += (q.bits & kAdjView2) ? 1 : 0; n3 += (q.bits & kAdjView3) ? 1 : 0;
    }
    const double terms = 2.0 * ((double)m + (double)n2 + (double)n3);
    LmControl lm(p->initial_lambda, c0, q0, n2 < kAdjMinView2 || n3 < kAdjMinView3);
    rep->initial_rms_px = m > 0 ? (float)sqrt(lm.sq / terms) : 0.0f;
    std::vector<float> Xn((size_t)3 * m);
    while (lm.running(p->max_iterations)) {
        const float lam = (float)lm.lambda;
        double sys[kAdjValues];
        for (int q = 0; q < kAdjValues; ++q) sys[q] = 0.0;
        for (const Pt &q : pts) {
            AdjustJac J;
            adjust_jacobian(K, P, q.obs, q.X, q.bits, J);
            float w[3], cost = 0.0f, sq = 0.0f, Vi[6], Wm[3 * kAdjCam], gp[3];
            adjust_weights(J.r, q.bits, p->huber_px, w, cost, sq);
            adjust_point_block(J, w, lam, Vi, Wm, gp);
            adjust_schur(J, w, Vi, Wm, gp, [&](int i, float v) { sys[i] += (double)v; });
        }
        double S[kAdjS], dc[kAdjCam];
        for (int q = 0; q < kAdjS; ++q) S[q] = sys[q];
        for (int q = 0; q < kAdjCam; ++q) { S[symn<kAdjCam>(q, q)] += lm.lambda * sys[kAdjU + q]; dc[q] = -sys[kAdjB + q]; }
        if (!refine_cholesky<kAdjCam>(S, dc)) {
            if (!lm.solve_failed()) break;
            continue;
        }
        float dcf[kAdjCam];
        for (int q = 0; q < kAdjCam; ++q) dcf[q] = (float)dc[q];
        adjust_camera_step(dc, state, trial);
        AdjustCams Pt_;
        adjust_load_cams(trial, Pt_);
        double nc = 0.0, nsq = 0.0;
        for (int k = 0; k < m; ++k) {
            const Pt &q = pts[(size_t)k];
            AdjustJac J;
            adjust_jacobian(K, P, q.obs, q.X, q.bits, J);
            float w[3], cost = 0.0f, sq = 0.0f, Vi[6], Wm[3 * kAdjCam], gp[3], dp[3];
            adjust_weights(J.r, q.bits, p->huber_px, w, cost, sq);
            adjust_point_block(J, w, lam, Vi, Wm, gp);
            adjust_point_step(Vi, Wm, gp, dcf, dp);
            float *Xt = &Xn[(size_t)3 * k];
            for (int c = 0; c < 3; ++c) Xt[c] = q.X[c] + dp[c];
            adjust_cost(K, Pt_, q.obs, Xt, q.bits, p->huber_px, cost, sq);
            nc += (double)cost; nsq += (double)sq;
        }
        bool stop;
        if (lm.tentative(nc, nsq, (double)p->min_rel_decrease, stop)) {
            memcpy(state, trial, sizeof(state));
            P = Pt_;
            for (int k = 0; k < m; ++k) memcpy(pts[(size_t)k].X, &Xn[(size_t)3 * k], 3 * sizeof(float));
        }
        if (stop) break;
    }
    for (int q = 0; q < 12; ++q) { out_poses[q] = state[q]; out_poses[12 + q] = state[18 + q]; }
    rep->status = lm.status; rep->iterations = lm.iters; rep->accepted = lm.accepted;
    rep->num_points = m; rep->num_view2 = n2; rep->num_view3 = n3;
    rep->final_rms_px = m > 0 ? (float)sqrt(lm.sq / terms) : 0.0f;
    rep->final_cost = (float)lm.cost;
    rep->lambda = (float)lm.lambda;
    const bool degenerate = lm.status == SFM_REFINE_DEGENERATE;
    for (int j = 0; j < n; ++j) {
        for (int c = 0; c < 4; ++c) out_points[(size_t)c * n + j] = points[(size_t)c * n + j];
        out_err[j] = __builtin_inff();
    }
    for (const Pt &q : pts) {
        if (!degenerate) {
            for (int c = 0; c < 3; ++c) out_points[(size_t)c * n + q.j] = q.X[c];
            out_points[(size_t)3 * n + q.j] = 1.0f;
        }
        out_err[q.j] = adjust_error(K, out_poses, out_poses + 12, q.obs, q.X, q.bits);
    }
}

// ctypes layout check: sizeof, then the offset of every field in declaration order
int adj_layout(int which, int64_t *out)
{
    int n = 0;
#define F(T, f) out[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        out[0] = sizeof(sfm_adjust_params);
        F(sfm_adjust_params, max_iterations); F(sfm_adjust_params, huber_px); F(sfm_adjust_params, min_rel_decrease);
        F(sfm_adjust_params, initial_lambda); F(sfm_adjust_params, d_used2); F(sfm_adjust_params, d_poses); F(sfm_adjust_params, reserved);
    } else if (which == 1) {
        out[0] = sizeof(sfm_adjust_in);
        F(sfm_adjust_in, d_sift); F(sfm_adjust_in, d_points); F(sfm_adjust_in, d_flags);
    } else if (which == 2) {
        out[0] = sizeof(sfm_adjust_report);
        F(sfm_adjust_report, status); F(sfm_adjust_report, iterations); F(sfm_adjust_report, accepted); F(sfm_adjust_report, num_points);
        F(sfm_adjust_report, num_view2); F(sfm_adjust_report, num_view3); F(sfm_adjust_report, initial_rms_px);
        F(sfm_adjust_report, final_rms_px); F(sfm_adjust_report, final_cost); F(sfm_adjust_report, lambda);
    } else {
        out[0] = sizeof(sfm_adjust_out);
        F(sfm_adjust_out, d_poses); F(sfm_adjust_out, d_points); F(sfm_adjust_out, d_views); F(sfm_adjust_out, d_err); F(sfm_adjust_out, d_report);
    }
#undef F
    return n;
}

}
