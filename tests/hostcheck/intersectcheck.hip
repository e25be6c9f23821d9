// tests/hostcheck/intersectcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_intersect_tracks (cuda-sfm_amd/csrc/intersect_math.hpp) as HIP *host* code: a serial driver of the
// whole call that walks every track's list in order -- intersect_track, what a lane of intersect.hip's lane kernel runs; the
// wavefront kernel's ordered sums of per-view terms must give the same bytes -- and the header's pieces one by one.  The CPU tests
// hold it to the fp64 twin (tests/intersect_reference.py), the GPU tests compare the device's outputs with it byte for byte.
// Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/intersect_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

extern "C" {

// What sfm_intersect_tracks computes, serially.  Per pair (arrays of k): n, ld, X0, X1 (3 x ld), K (9).  in / out: the structs over
// host memory (in->pairs is not read).  starts (N bytes, or null): per track 0 no eligible start, 1 started from C, 2 from L, 3
// copied through.
void intersect_run(int k, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
                   const sfm_intersect_in *in, const sfm_intersect_params *p, const sfm_intersect_out *out, uint8_t *starts)
{
    if (k <= 0) return;
    std::vector<FusePair> pairs((size_t)k);
    int N = 0;
    for (int i = 0; i < k; ++i) {
        FusePair &f = pairs[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = X0[i]; f.X1 = X1[i]; f.K = K[i]; f.n = n[i]; f.ld = ld[i]; f.offset = N;
        N += n[i];
    }
    const int T = in->d_counts[0] < N ? in->d_counts[0] : N;
    int32_t counts[kIntersectCounts] = { T, 0, 0, 0, 0, 0, 0, 0 };
    for (int t = 0; t < T; ++t) {
        const int o0 = in->d_track_offset[t], count = in->d_track_offset[t + 1] - o0;
        const int32_t *cam = in->d_obs_cam + o0, *rec = in->d_obs_record + o0;
        auto view = [&](int o) { return fuse_view(pairs[(size_t)(cam[o] >> 1)], in->d_cams, cam[o] >> 1, cam[o] & 1, rec[o]); };
        float Xin[4];
        for (int c = 0; c < 4; ++c) Xin[c] = in->d_points[(size_t)c * N + t];
        IntersectResult r;
        intersect_track(in->d_flags[t], count, in->d_skip && in->d_skip[t] != 0, Xin, view, *p, r);
        for (int c = 0; c < 4; ++c) out->d_points[(size_t)c * N + t] = r.out[c];
        out->d_flags[t] = r.flag;
        if (out->d_err) out->d_err[t] = r.err;
        if (starts) starts[t] = r.copied ? 3 : (uint8_t)r.start;
        if (r.copied) { ++counts[4]; continue; }
        ++counts[1];
        if (r.start == kIntersectNone) { ++counts[6]; continue; }
        ++counts[(r.flag == SFM_FUSE_REFINED || r.flag == SFM_FUSE_SEAM_REFINED) ? 2 : 3];
        if (r.start == kIntersectL) ++counts[5];
        if (r.promoted) ++counts[7];
    }
    for (int q = 0; q < kIntersectCounts; ++q) out->d_counts[q] = counts[q];
}

// ---- the header's pieces one by one ----
// candidate L of `count` views: Ps (12 each), xy (2 each); returns 1 where it is finite
int intersect_check_linear(int count, const float *Ps, const float *xy, float *L)
{
    auto view = [&](int o) {
        FuseView v;
        v.K.fx = 1.0f; v.K.s = 0.0f; v.K.fy = 1.0f;
        v.P = Ps + 12 * o; v.x = xy[2 * o]; v.y = xy[2 * o + 1];
        return v;
    };
    intersect_linear(count, view, L);
    return intersect_finite(L) ? 1 : 0;
}
int intersect_check_choose(int c_ok, float c_cost, int l_ok, float l_cost) { return intersect_choose(c_ok != 0, c_cost, l_ok != 0, l_cost); }
int intersect_check_class(int flag, int accepted) { return intersect_class(flag, accepted != 0); }
int intersect_check_copied(int flag, int count, int skip) { return intersect_copied(flag, count, skip != 0) ? 1 : 0; }
int intersect_check_wave_min_views(void) { return kIntersectWaveMinViews; }

// ctypes layout check: sizeof, then the offset of every field in declaration order
int intersect_layout(int which, int64_t *o)
{
    int n = 0;
#define F(T, f) o[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        o[0] = sizeof(sfm_intersect_params);
        F(sfm_intersect_params, threshold_px); F(sfm_intersect_params, max_iterations); F(sfm_intersect_params, huber_px);
        F(sfm_intersect_params, min_rel_decrease); F(sfm_intersect_params, initial_lambda); F(sfm_intersect_params, wave_min_views);
        F(sfm_intersect_params, reserved);
    } else if (which == 1) {
        o[0] = sizeof(sfm_intersect_in);
        F(sfm_intersect_in, pairs); F(sfm_intersect_in, d_cams); F(sfm_intersect_in, d_track_offset); F(sfm_intersect_in, d_obs_cam);
        F(sfm_intersect_in, d_obs_record); F(sfm_intersect_in, d_points); F(sfm_intersect_in, d_flags); F(sfm_intersect_in, d_counts);
        F(sfm_intersect_in, d_skip);
    } else {
        o[0] = sizeof(sfm_intersect_out);
        F(sfm_intersect_out, d_points); F(sfm_intersect_out, d_flags); F(sfm_intersect_out, d_err); F(sfm_intersect_out, d_counts);
    }
#undef F
    return n;
}

}
