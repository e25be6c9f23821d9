// tests/hostcheck/viewpointscheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_triangulate_view (cuda-sfm_amd/csrc/view_points_math.hpp) as HIP *host* code and runs it over
// arrays on the CPU: the CPU tests compare it with the fp64 twin (tests/view_points_reference.py), the GPU tests compare the
// device's bytes with it.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/view_points_math.hpp"
#include "../../include/sfm_amd.h"
#include <string.h>

using namespace sfm;

extern "C" {

// What the kernel does for every point, in point order.  sift: n records; X0, X1: 3 x ld; points: 4 x n; valid: n or null;
// poses: [R|t] of camera 2 then camera 3 (24); p: the call's parameters (its pointers are not read).  counts: 8.
void vp_run(int n, int ld, const sfm_sift_point *sift, const float *X0, const float *X1, const float K[9], const float Kinv[9],
            const float *points, const uint8_t *valid, const float poses[24], const sfm_view_points_params *p,
            float *out_points, uint8_t *out_flags, float *out_err, int32_t *out_counts)
{
    ViewPointsArgs a;
    a.sift = sift; a.X0 = X0; a.X1 = X1; a.K = K; a.Kinv = Kinv; a.points = points; a.valid = valid;
    a.pose2 = poses; a.pose3 = poses + 12; a.pose_rows = 3;
    a.ld = ld; a.n = n;
    a.min_score = p->min_score; a.max_ambiguity = p->max_ambiguity;
    a.thr = p->threshold_px; a.cos_min = view_points_cos_min(p->min_parallax_deg);
    a.max_iter = p->max_iterations; a.huber = p->huber_px; a.min_rel = p->min_rel_decrease; a.lambda0 = p->initial_lambda;
    a.out_points = out_points; a.out_flags = out_flags; a.out_err = out_err; a.out_counts = out_counts;
    ViewPointsCams c;
    c.K = RefineCam{ K[0], K[1], K[4] };
    for (int q = 0; q < 9; ++q) c.Kinv[q] = Kinv[q];
    view_points_pose(a.pose2, a.pose_rows, c.P2);
    view_points_pose(a.pose3, a.pose_rows, c.P3);
    memset(out_counts, 0, 8 * sizeof(int32_t));
    for (int j = 0; j < n; ++j) {
        float out[4], err;
        const uint8_t cls = view_points_one(c, a, j, out, err);
        for (int q = 0; q < 4; ++q) out_points[(size_t)q * n + j] = out[q];
        out_flags[j] = cls;
        out_err[j] = err;
        ++out_counts[cls];
    }
}

// ctypes layout check: sizeof, then the offset of every field in declaration order
int vp_layout(int which, int64_t *out)
{
    int n = 0;
#define F(T, f) out[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        out[0] = sizeof(sfm_view_points_params);
        F(sfm_view_points_params, threshold_px); F(sfm_view_points_params, min_score); F(sfm_view_points_params, max_ambiguity);
        F(sfm_view_points_params, min_parallax_deg); F(sfm_view_points_params, max_iterations); F(sfm_view_points_params, huber_px);
        F(sfm_view_points_params, min_rel_decrease); F(sfm_view_points_params, initial_lambda); F(sfm_view_points_params, d_points);
        F(sfm_view_points_params, d_valid); F(sfm_view_points_params, d_poses); F(sfm_view_points_params, reserved);
    } else {
        out[0] = sizeof(sfm_view_points_out);
        F(sfm_view_points_out, d_points); F(sfm_view_points_out, d_flags); F(sfm_view_points_out, d_err); F(sfm_view_points_out, d_counts);
    }
#undef F
    return n;
}

}
