// tests/hostcheck/registercheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of the view registration (cuda-sfm_amd/csrc/register_math.hpp) as HIP *host* code, so that CPU tests
// can check the P3P solver, the sampler, the inlier test and the pose Jacobian without a GPU, and GPU tests can compare every
// RANSAC count of the device with the same arithmetic on the host.  Nothing in the product loads this library; it is not a
// CPU fallback.
#include "../../cuda-sfm_amd/csrc/register_math.hpp"
#include "../../include/sfm_amd.h"

using namespace sfm;

static RefineCam cam_of(const float c[3]) { return RefineCam{ c[0], c[1], c[2] }; }

extern "C" {

void rg_sample4(uint32_t seed, uint32_t hyp, int m, int idx[4]) { sample4(seed, hyp, m, idx); }

// every solution of Lambda Twist for unit bearings y (3 x 3, row i = bearing i) and points X (3 x 3): R (9) + t (3) each
int rg_p3p(const float y[9], const float X[9], float out[48])
{
    int n = 0;
    p3p_lambda_twist(y, y + 3, y + 6, X, X + 3, X + 6, [&](const float R[9], const float t[3]) {
        for (int k = 0; k < 9; ++k) out[12 * n + k] = R[k];
        for (int k = 0; k < 3; ++k) out[12 * n + 9 + k] = t[k];
        ++n;
    });
    return n;
}

float rg_cubic(float b, float c, float d) { return p3p_cubic(b, c, d); }

int rg_inlier(const float cam[3], float thr, const float P[12], const float X[3], float x, float y)
{
    return register_inlier(cam_of(cam), thr, P, X, x, y) ? 1 : 0;
}

float rg_sq_error(const float cam[3], const float P[12], const float X[3], float x, float y)
{
    return register_sq_error(cam_of(cam), P, X, x, y);
}

// one hypothesis: the pose (12) and whether the sample was usable
int rg_hypothesis(uint32_t seed, uint32_t hyp, int m, const float cam[3], const float *Xc /* m x 4 */, const float *Oc /* m x 2 */, float P[12])
{
    return register_hypothesis(seed, hyp, m, cam_of(cam), reinterpret_cast<const float4 *>(Xc), reinterpret_cast<const float2 *>(Oc), P) ? 1 : 0;
}

// what the device's solve + score kernels compute: every hypothesis' pose (12 x H, as the device stores them) and inlier count,
// and the packed arg-max key (count << 32) | (0xFFFFFFFF - hyp)
uint64_t rg_ransac(uint32_t seed, uint32_t H, int m, const float cam[3], float thr, const float *Xc, const float *Oc,
                   int32_t *counts, float *poses)
{
    const RefineCam K = cam_of(cam);
    const float4 *X4 = reinterpret_cast<const float4 *>(Xc);
    const float2 *O2 = reinterpret_cast<const float2 *>(Oc);
    uint64_t best = 0;
    for (uint32_t h = 0; h < H; ++h) {
        float P[12];
        register_hypothesis(seed, h, m, K, X4, O2, P);
        int c = 0;
        for (int k = 0; k < m; ++k) {
            const float X[3] = { X4[k].x, X4[k].y, X4[k].z };
            c += register_inlier(K, thr, P, X, O2[k].x, O2[k].y) ? 1 : 0;
        }
        counts[h] = c;
        if (poses)
            for (int q = 0; q < 12; ++q) poses[(size_t)q * H + h] = P[q];
        const uint64_t key = pack_key((uint32_t)c, h);
        best = key > best ? key : best;
    }
    return best;
}

// r (2), J (12), Y.z
void rg_jacobian(const float cam[3], const float P[12], const float X[3], float x, float y, float out[15])
{
    out[14] = register_jacobian(cam_of(cam), P, X, x, y, out, out + 2);
}

int rg_solve6(double S[21], double x[6]) { return refine_cholesky<6>(S, x) ? 1 : 0; }

// ctypes layout check: sizeof, then the offset of every field in declaration order
int rg_layout(int which, int64_t *out)
{
    int n = 0;
#define F(T, f) out[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        out[0] = sizeof(sfm_register_params);
        F(sfm_register_params, num_hypotheses); F(sfm_register_params, seed); F(sfm_register_params, threshold_px);
        F(sfm_register_params, min_score); F(sfm_register_params, max_ambiguity); F(sfm_register_params, max_iterations);
        F(sfm_register_params, huber_px); F(sfm_register_params, min_rel_decrease); F(sfm_register_params, initial_lambda);
        F(sfm_register_params, d_points); F(sfm_register_params, d_valid); F(sfm_register_params, reserved);
    } else {
        out[0] = sizeof(sfm_register_report);
        F(sfm_register_report, status); F(sfm_register_report, num_candidates); F(sfm_register_report, ransac_inliers);
        F(sfm_register_report, num_inliers); F(sfm_register_report, best_hypothesis); F(sfm_register_report, iterations);
        F(sfm_register_report, accepted); F(sfm_register_report, initial_rms_px); F(sfm_register_report, final_rms_px);
        F(sfm_register_report, final_cost); F(sfm_register_report, lambda);
    }
#undef F
    return n;
}

}
