// tests/hostcheck/refineruncheck.hip -- TEST HARNESS ONLY.
// A serial driver of the whole of sfm_refine_two_view (rc_run), compiled as HIP *host* code into librefinecheck.so next to
// refinecheck.hip's per-point functions: the three kernel bodies of cuda-sfm_amd/csrc/refine.hip through the same header functions
// (device_math.hpp, refine_math.hpp) and LmControl, the fp64 sums taken in the solve block's own order (per-thread strided sums,
// wave butterflies, wave partials in wave order).  The CPU tests hold it to the fp64 twin (tests/refine_reference.py) and the GPU
// tests compare the device's outputs with it, byte for byte.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/refine_math.hpp"
#include <math.h>
#include <algorithm>
#include <vector>

using namespace sfm;

static RefinePose pose_of(const float *p /* R 9, t 3, b1 3, b2 3 */)
{
    RefinePose P;
    for (int k = 0; k < 9; ++k) P.R[k] = p[k];
    for (int k = 0; k < 3; ++k) { P.t[k] = p[9 + k]; P.b1[k] = p[12 + k]; P.b2[k] = p[15 + k]; }
    return P;
}

// ---- the whole call, serially (rc_run) ----
// refine.hip's constants, restated: the kernels are device code and cannot be included here
constexpr int kRcSweeps = 8, kRcThreads = 512, kRcWaves = kRcThreads / 64, kRcMinPoints = 16, kRcSys = 25;

// block_sum (block_ops.hpp) over kRcThreads per-thread values, on the host: in every wave of 64 lanes what lane 0 holds after
// x += shfl_xor(x, off) for off = 32 .. 1 -- a[i] += a[i + off] for i < off, the addition being commutative -- then the wave
// partials in wave order.
static double rc_block_sum(const double *v /* kRcThreads values, stride `stride` */, int stride)
{
    double part[kRcWaves];
    for (int w = 0; w < kRcWaves; ++w) {
        double a[64];
        for (int l = 0; l < 64; ++l) a[l] = v[(size_t)(64 * w + l) * stride];
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) a[l] = a[l] + a[l + off];
        part[w] = a[0];
    }
    double s = part[0];
    for (int w = 1; w < kRcWaves; ++w) s += part[w];
    return s;
}

// N sums of a block: acc[tid][q] are the per-thread sums (thread tid added records tid, tid + 512, ... in rising order)
template <int N>
static void rc_block_sums(const std::vector<double> &acc, double out[N])
{
    for (int q = 0; q < N; ++q) out[q] = rc_block_sum(acc.data() + q, N);
}

// refine.hip's set_basis: the tangent basis of the pose in s (R 9, t 3) into s[12..17]
static void rc_set_basis(float *s)
{
    const double t[3] = { s[9], s[10], s[11] };
    double b1[3], b2[3];
    refine_tangent_basis(t, b1, b2);
    for (int k = 0; k < 3; ++k) { s[12 + k] = (float)b1[k]; s[15 + k] = (float)b2[k]; }
}

extern "C" {

// The block sum alone, for the test of its order: v[512] -> the total
double rc_sum512(const double *v) { return rc_block_sum(v, 1); }

// What sfm_refine_two_view computes, serially, the three kernel bodies of refine.hip in turn.  X0, X1: 3 x ld; E, Kf: 9; mask: n
// (the caller's, or the pair's inlier mask); p: the call's parameters (its pointer is not read).  Outputs as the getters hand them
// out: pose (16) + E (9), points 4 x n, err n, used n, the report; trace (8): which of Xa / Xb held the committed points at the
// end, failed solves, rejected steps, 0, the four candidates' votes.
void rc_run(int n, int ld, const float *X0, const float *X1, const float *E, const float *Kf, const uint8_t *mask,
            const sfm_refine_params *p, float *out_pose, float *out_points, float *out_err, uint8_t *out_used, sfm_refine_report *rep,
            int *trace)
{
    struct F4 { float x, y, z, w; };
    const RefineCam K = { Kf[0], Kf[1], Kf[4] };
    // ---- refine_start_block: candidates, start points, votes ----
    float e[9], cands[64];
    for (int k = 0; k < 9; ++k) e[k] = E[k];
    pose_candidates(e, SFM_POSE_CORRECT, cands);
    std::vector<F4> cand((size_t)4 * n);
    int votes[4] = { 0, 0, 0, 0 };
    for (int j = 0; j < n; ++j) {
        if (!mask[j]) continue;
        for (int i = 0; i < 4; ++i) {
            const float *Pm = cands + 16 * i;
            float pt[4];
            const float z0 = X0[2 * (size_t)ld + j], z1 = X1[2 * (size_t)ld + j];
            triangulate_point(X0[j] / z0, X0[(size_t)ld + j] / z0, X1[j] / z1, X1[(size_t)ld + j] / z1, Pm, kRcSweeps, pt);
            float z2 = Pm[8] * pt[0];
            for (int k = 1; k < 4; ++k) z2 = fmaf(Pm[8 + k], pt[k], z2);
            if ((pt[2] > 0.0f) && (z2 > 0.0f)) ++votes[i];
            cand[(size_t)i * n + j] = F4{ pt[0], pt[1], pt[2], pt[3] };
        }
    }
    // ---- refine_solve_block ----
    int best = votes[0], pi = 0;                          // first maximum
    for (int i = 1; i < 4; ++i) if (votes[i] > best) { best = votes[i]; pi = i; }
    float s_pose[18], s_try[18], s_dc[5];
    {
        const float *P = cands + 16 * pi;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) s_pose[3 * r + c] = P[4 * r + c];
            s_pose[9 + r] = P[4 * r + 3];
        }
        rc_set_basis(s_pose);
    }
    RefinePose P = pose_of(s_pose);
    std::vector<int> slot((size_t)n), idx;
    std::vector<F4> obs, Xa, Xb;
    for (int j = 0; j < n; ++j) {                         // record order is the order of the rounds and of the lanes inside one
        bool use = false;
        F4 X = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (mask[j]) {
            X = cand[(size_t)pi * n + j];
            const float Xv[3] = { X.x, X.y, X.z };
            float q[3], Y[3];
            refine_to_cam2(P, Xv, q, Y);
            use = isfinite(X.x) && isfinite(X.y) && isfinite(X.z) && X.z > 0.0f && Y[2] > 0.0f;
        }
        slot[(size_t)j] = use ? (int)idx.size() : -1;
        if (use) {
            const float z1 = X0[2 * (size_t)ld + j], z2 = X1[2 * (size_t)ld + j];
            obs.push_back(F4{ X0[j] / z1, X0[(size_t)ld + j] / z1, X1[j] / z2, X1[(size_t)ld + j] / z2 });
            Xa.push_back(X);
            idx.push_back(j);
        }
    }
    const int m = (int)idx.size();
    Xb.resize((size_t)m);
    const float huber = p->huber_px;
    std::vector<double> acc2((size_t)kRcThreads * 2), accs((size_t)kRcThreads * kRcSys);
    double tot2[2], tot[kRcSys];
    // the cost of the start
    std::fill(acc2.begin(), acc2.end(), 0.0);
    for (int k = 0; k < m; ++k) {
        double *v = &acc2[(size_t)(k % kRcThreads) * 2];
        const F4 o4 = obs[(size_t)k], X4 = Xa[(size_t)k];
        const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
        float r[4], z1, z2, rho1, rho2;
        refine_residual(K, P, o, X, r, z1, z2);
        refine_huber(r[0], r[1], huber, rho1);
        refine_huber(r[2], r[3], huber, rho2);
        v[0] += (double)rho1 + (double)rho2;
        v[1] += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
    }
    rc_block_sums<2>(acc2, tot2);
    LmControl lm(p->initial_lambda, tot2[0], tot2[1], m < kRcMinPoints);
    const float initial_rms = m > 0 ? (float)sqrt(lm.sq / (4.0 * m)) : 0.0f;
    int cur = 0, failed = 0, rejected = 0;
    while (lm.running(p->max_iterations)) {
        const float lam = (float)lm.lambda;
        const std::vector<F4> &Xc = cur ? Xb : Xa;
        std::vector<F4> &Xn = cur ? Xa : Xb;
        // pass A
        std::fill(accs.begin(), accs.end(), 0.0);
        for (int k = 0; k < m; ++k) {
            double *sys = &accs[(size_t)(k % kRcThreads) * kRcSys];
            const F4 o4 = obs[(size_t)k], X4 = Xc[(size_t)k];
            const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
            RefineJac J;
            refine_jacobian(K, P, o, X, J);
            float rho, Vi[6], Wm[15], gp[3];
            const float w1 = refine_huber(J.r[0], J.r[1], huber, rho), w2 = refine_huber(J.r[2], J.r[3], huber, rho);
            refine_point_block(J, w1, w2, lam, Vi, Wm, gp);
            refine_schur(J, w2, Vi, Wm, gp, [&](int q, float v) { sys[q] += (double)v; });
        }
        rc_block_sums<kRcSys>(accs, tot);
        // the pose step
        bool ok;
        {
            double Sd[15], dc[5];
            for (int q = 0; q < 15; ++q) Sd[q] = tot[q];
            for (int q = 0; q < 5; ++q) { Sd[sym5(q, q)] += lm.lambda * tot[20 + q]; dc[q] = -tot[15 + q]; }
            ok = refine_solve5(Sd, dc);
            if (ok) {
                double t[3], nn = 0.0;
                float Rn[9];
                refine_rotate(dc, s_pose, Rn);
                for (int q = 0; q < 9; ++q) s_try[q] = Rn[q];
                for (int q = 0; q < 3; ++q) { t[q] = (double)s_pose[9 + q] + (double)s_pose[12 + q] * dc[3] + (double)s_pose[15 + q] * dc[4]; nn += t[q] * t[q]; }
                nn = sqrt(nn);
                for (int q = 0; q < 3; ++q) s_try[9 + q] = (float)(t[q] / nn);
                for (int q = 0; q < 5; ++q) s_dc[q] = (float)dc[q];
                rc_set_basis(s_try);
            }
        }
        if (!ok) {
            ++failed;
            if (!lm.solve_failed()) break;
            continue;
        }
        // pass B
        const RefinePose Pt = pose_of(s_try);
        const float dc[5] = { s_dc[0], s_dc[1], s_dc[2], s_dc[3], s_dc[4] };
        std::fill(acc2.begin(), acc2.end(), 0.0);
        for (int k = 0; k < m; ++k) {
            double *v = &acc2[(size_t)(k % kRcThreads) * 2];
            const F4 o4 = obs[(size_t)k], X4 = Xc[(size_t)k];
            const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
            RefineJac J;
            refine_jacobian(K, P, o, X, J);
            float rho1, rho2, Vi[6], Wm[15], gp[3], dp[3];
            const float w1 = refine_huber(J.r[0], J.r[1], huber, rho1), w2 = refine_huber(J.r[2], J.r[3], huber, rho2);
            refine_point_block(J, w1, w2, lam, Vi, Wm, gp);
            refine_point_step(Vi, Wm, gp, dc, dp);
            const float Xt[3] = { X[0] + dp[0], X[1] + dp[1], X[2] + dp[2] };
            Xn[(size_t)k] = F4{ Xt[0], Xt[1], Xt[2], 1.0f };
            float r[4], z1, z2;
            refine_residual(K, Pt, o, Xt, r, z1, z2);
            refine_huber(r[0], r[1], huber, rho1);
            refine_huber(r[2], r[3], huber, rho2);
            v[0] += (double)rho1 + (double)rho2;
            v[1] += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
        }
        rc_block_sums<2>(acc2, tot2);
        bool stop;
        if (lm.tentative(tot2[0], tot2[1], (double)p->min_rel_decrease, stop)) {
            cur ^= 1;
            P = Pt;
            for (int q = 0; q < 18; ++q) s_pose[q] = s_try[q];
        } else {
            ++rejected;
        }
        if (stop) break;
    }
    {
        float *Po = out_pose;
        const float *R = s_pose, *t = s_pose + 9;
        refine_store_pose(s_pose, Po);
        const float tx[9] = { 0.0f, -t[2], t[1], t[2], 0.0f, -t[0], -t[1], t[0], 0.0f };
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Po[16 + 3 * r + c] = tx[3 * r] * R[c] + tx[3 * r + 1] * R[3 + c] + tx[3 * r + 2] * R[6 + c];
        rep->status = lm.status; rep->iterations = lm.iters; rep->accepted = lm.accepted; rep->num_used = m; rep->pose_index = pi;
        rep->initial_rms_px = initial_rms;
        rep->final_rms_px = m > 0 ? (float)sqrt(lm.sq / (4.0 * m)) : 0.0f;
        rep->final_cost = (float)lm.cost;
        rep->lambda = (float)lm.lambda;
    }
    if (cur) {                                            // the finish body reads the committed points from Xa
        for (int k = 0; k < m; ++k) Xa[(size_t)k] = Xb[(size_t)k];
    }
    trace[0] = cur; trace[1] = failed; trace[2] = rejected; trace[3] = 0;
    for (int i = 0; i < 4; ++i) trace[4 + i] = votes[i];
    // ---- refine_finish_block ----
    for (int j = 0; j < n; ++j) {
        float Pm[16];
        for (int k = 0; k < 16; ++k) Pm[k] = out_pose[k];
        const int k = slot[(size_t)j];
        const float z1 = X0[2 * (size_t)ld + j], z2 = X1[2 * (size_t)ld + j];
        const float o[4] = { X0[j] / z1, X0[(size_t)ld + j] / z1, X1[j] / z2, X1[(size_t)ld + j] / z2 };
        float pt[4];
        if (k >= 0) {
            const F4 X = Xa[(size_t)k];
            pt[0] = X.x; pt[1] = X.y; pt[2] = X.z; pt[3] = 1.0f;
        } else {
            triangulate_point(o[0], o[1], o[2], o[3], Pm, kRcSweeps, pt);
        }
        for (int c = 0; c < 4; ++c) out_points[(size_t)c * n + j] = pt[c];
        RefinePose Pf;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Pf.R[3 * r + c] = Pm[4 * r + c];
            Pf.t[r] = Pm[4 * r + 3];
            Pf.b1[r] = 0.0f; Pf.b2[r] = 0.0f;
        }
        float r[4], d1, d2;
        refine_residual(K, Pf, o, pt, r, d1, d2);
        const float err = fmaxf(sqrtf(r[0] * r[0] + r[1] * r[1]), sqrtf(r[2] * r[2] + r[3] * r[3]));
        out_err[j] = (d1 > 0.0f && d2 > 0.0f) ? err : __builtin_inff();
        out_used[j] = k >= 0 ? 1 : 0;
    }
}

}
