// tests/hostcheck/ringcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_close_ring (cuda-sfm_amd/csrc/ring_math.hpp) as HIP *host* code: a serial driver of the whole
// call -- the same header functions as ring.hip, the links and records visited in order, the seam's sums taken in the order
// block_sum and the fold take them -- that the CPU tests hold to the fp64 twin (tests/ring_reference.py) and the GPU tests compare
// the device's outputs with.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../include/sfm_amd.h"
#include "../../cuda-sfm_amd/csrc/ring_math.hpp"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

// block_sum (block_ops.hpp) over the 256 threads' values: per wavefront the xor butterfly, then the wave partials in wave order
static void block_sum_order(const double v[kRingBlock][kRingSums], double out[kRingSums])
{
    for (int q = 0; q < kRingSums; ++q) {
        double part[kRingBlock / 64];
        for (int w = 0; w < kRingBlock / 64; ++w) {
            double x[64], y[64];
            for (int l = 0; l < 64; ++l) x[l] = v[64 * w + l][q];
            for (int off = 32; off > 0; off >>= 1) {
                for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ off];
                memcpy(x, y, sizeof(x));
            }
            part[w] = x[0];
        }
        double s = part[0];
        for (int w = 1; w < kRingBlock / 64; ++w) s += part[w];
        out[q] = s;
    }
}

extern "C" {

// What sfm_close_ring computes, serially.  sims: 13 x k, status / num_inliers: k (the links' reports); the last pair: n, ld, points
// (4 x n), valid (n or null), X1 (3 x ld), K (9).  p->weights: host, as in the call.  links / frames: 13 x k, seam_err: 3 x n or null.
void ring_run(int k, const float *sims, const int32_t *status, const int32_t *num_inliers, int n, int ld, const float *points, const uint8_t *valid,
              const float *X1, const float *K, const sfm_ring_params *p, float *links, float *frames, float *seam_err, sfm_ring_report *report)
{
    // ---- the walk: F_0 .. F_k, the weights ----
    std::vector<double> F((size_t)(k + 1) * kFuseSim), w((size_t)k), alpha((size_t)k + 1);
    fuse_identity(F.data());
    int first_invalid = -1;
    for (int i = 0; i < k; ++i) {
        float link[kFuseSim];
        memcpy(link, sims + (size_t)kFuseSim * i, sizeof(link));
        double *next = F.data() + (size_t)kFuseSim * (i + 1);
        if (!fuse_link_valid(status[i], link)) {
            fuse_identity(next);
            if (first_invalid < 0) first_invalid = i;
        } else {
            double inv[kFuseSim];
            fuse_invert(link, inv);
            fuse_compose(F.data() + (size_t)kFuseSim * i, inv, next);
        }
        w[(size_t)i] = p->weights ? (double)p->weights[i] : ring_weight(num_inliers[i]);
    }
    RingHead h;
    float drift[3] = { 0.0f, 0.0f, 0.0f };
    for (int q = 0; q < 7; ++q) h.corr[q] = 0.0;
    fuse_identity(h.Dinv);
    h.status = SFM_RING_OPEN; h.pad = 0;
    if (first_invalid < 0) ring_drift(F.data() + (size_t)kFuseSim * k, p->max_rotation_rad, p->max_log_scale, h, drift);
    if (h.status == SFM_RING_CLOSED) ring_alphas(w.data(), k, alpha.data());
    report->status = h.status; report->num_links = k; report->first_invalid = first_invalid;
    report->drift_log_scale = drift[0]; report->drift_rotation_rad = drift[1]; report->drift_t = drift[2];
    // ---- the corrected links and the closed frames ----
    for (int i = 0; i < k; ++i) {
        const double *F0 = F.data() + (size_t)kFuseSim * i;
        float link[kFuseSim], frame[kFuseSim];
        if (h.status != SFM_RING_CLOSED) {
            memcpy(link, sims + (size_t)kFuseSim * i, sizeof(link));
            for (int q = 0; q < kFuseSim; ++q) frame[q] = (float)F0[q];
        } else ring_correct(h, alpha[(size_t)i], alpha[(size_t)i + 1], i + 1 == k, F0, F0 + kFuseSim, link, frame);
        memcpy(links + (size_t)kFuseSim * i, link, sizeof(link));
        memcpy(frames + (size_t)kFuseSim * i, frame, sizeof(frame));
    }
    // ---- the seam: ring_seam_kernel's blocks, rounds and sums in its order ----
    FusePair pr;
    memset(&pr, 0, sizeof(pr));
    pr.points = points; pr.valid = valid; pr.X1 = X1; pr.K = K; pr.n = n; pr.ld = ld;
    float open[kFuseSim];
    for (int q = 0; q < kFuseSim; ++q) open[q] = (float)F[(size_t)kFuseSim * (k - 1) + q];
    const float *const three[3] = { sims + (size_t)kFuseSim * (k - 1), open, frames + (size_t)kFuseSim * (k - 1) };
    const int blocks = ring_seam_blocks(n);
    std::vector<double> partial((size_t)blocks * kRingSums);
    static double v[kRingBlock][kRingSums];
    for (int b = 0; b < blocks; ++b) {
        memset(v, 0, sizeof(v));
        for (int base = b * kRingBlock; base < n; base += blocks * kRingBlock) {
            for (int tid = 0; tid < kRingBlock && base + tid < n; ++tid) {
                float err[3];
                double t[kRingSums];
                ring_seam_record(pr, base + tid, p->threshold_px, three, err, t);
                for (int q = 0; q < kRingSums; ++q) v[tid][q] += t[q];
                if (seam_err) for (int f = 0; f < 3; ++f) seam_err[(size_t)f * n + base + tid] = err[f];
            }
        }
        block_sum_order(v, partial.data() + (size_t)kRingSums * b);
    }
    memset(v, 0, sizeof(v));
    for (int tid = 0; tid < kRingBlock; ++tid)
        for (int b = tid; b < blocks; b += kRingBlock)
            for (int q = 0; q < kRingSums; ++q) v[tid][q] += partial[(size_t)kRingSums * b + q];
    double total[kRingSums];
    block_sum_order(v, total);
    ring_seam_report(total, *report);
}

// the rotation's logarithm and exponential on their own (tests/test_ring_host.py: round trip)
double ring_log(const double R[9], double w[3]) { return ring_rot_log(R, w); }
void ring_exp(const double w[3], double R[9]) { ring_rot_exp(w, R); }
int ring_blocks(int n) { return ring_seam_blocks(n); }

// ctypes layout check: sizeof, then the offset of every field in declaration order
int ring_layout(int which, int64_t *o)
{
    int n = 0;
#define F(T, f) o[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        o[0] = sizeof(sfm_ring_params);
        F(sfm_ring_params, threshold_px); F(sfm_ring_params, max_rotation_rad); F(sfm_ring_params, max_log_scale); F(sfm_ring_params, weights);
        F(sfm_ring_params, reserved);
    } else if (which == 1) {
        o[0] = sizeof(sfm_ring_link_in);
        F(sfm_ring_link_in, d_sim); F(sfm_ring_link_in, d_report);
    } else if (which == 2) {
        o[0] = sizeof(sfm_ring_report);
        F(sfm_ring_report, status); F(sfm_ring_report, num_links); F(sfm_ring_report, first_invalid); F(sfm_ring_report, drift_log_scale);
        F(sfm_ring_report, drift_rotation_rad); F(sfm_ring_report, drift_t); F(sfm_ring_report, seam_count); F(sfm_ring_report, seam_lost_open);
        F(sfm_ring_report, seam_lost_closed); F(sfm_ring_report, seam_rms_link_px); F(sfm_ring_report, seam_rms_open_px);
        F(sfm_ring_report, seam_rms_closed_px);
    } else {
        o[0] = sizeof(sfm_ring_out);
        F(sfm_ring_out, d_links); F(sfm_ring_out, d_frames); F(sfm_ring_out, d_seam_err); F(sfm_ring_out, d_report);
    }
#undef F
    return n;
}

}
