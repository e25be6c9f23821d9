// tests/hostcheck/fuseringcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_fuse_ring (cuda-sfm_amd/csrc/fuse_ring_math.hpp over fuse_math.hpp and ring_math.hpp) as HIP
// *host* code: a serial driver of the whole call -- the same header functions and LmControl as fuse.hip and fuse_ring.hip, the
// nodes visited in order instead of scanned -- that the CPU tests hold to the fp64 twin (tests/fuse_ring_reference.py) and the GPU
// tests compare the device's outputs with.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/fuse_ring_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

extern "C" {

// What sfm_fuse_ring computes, serially.  Per pair (arrays of k): n, ld, points (4 x n), valid (n or null), X0, X1 (3 x ld), K (9),
// pose (12: R then t).  Per link (arrays of k: link k - 1 is pair k - 1's, onto pair 0): index, sim (13), inlier, err, status.
// out: sfm_fuse_out over host memory; report: host memory.
void fuse_ring_run(int k, const int32_t *n, const int32_t *ld, const float *const *points, const uint8_t *const *valid, const float *const *X0,
                   const float *const *X1, const float *const *K, const float *const *pose, const int32_t *const *index, const float *const *sim,
                   const uint8_t *const *inlier, const float *const *err, const int32_t *status, const sfm_fuse_ring_params *p,
                   const sfm_fuse_out *out, sfm_fuse_ring_report *report)
{
    if (k < 3) return;
    std::vector<FusePair> pr((size_t)k);
    std::vector<sfm_align_report> rep((size_t)k);
    int N = 0;
    for (int i = 0; i < k; ++i) {
        FusePair &f = pr[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.points = points[i]; f.valid = valid[i]; f.X0 = X0[i]; f.X1 = X1[i]; f.K = K[i]; f.pose = pose[i]; f.pose_rows = 3;
        f.n = n[i]; f.ld = ld[i]; f.offset = N;
        N += n[i];
        memset(&rep[(size_t)i], 0, sizeof(sfm_align_report));
        rep[(size_t)i].status = status[i];
        f.index = index[i]; f.sim = sim[i]; f.inlier = inlier[i]; f.err = err[i]; f.report = &rep[(size_t)i];
    }
    for (int c = 0; c < 8; ++c) out->d_counts[c] = 0;
    // ---- the chain part: frames, roots, cameras over links 0 .. k - 2 ----
    double F[kFuseSim];
    int root = 0, segs = 0;
    for (int i = 0; i < k; ++i) {
        if (i == 0 || !fuse_link_ok(pr[(size_t)i - 1])) { fuse_identity(F); root = i; ++segs; }
        else {
            float link[kFuseSim];
            double inv[kFuseSim], G[kFuseSim];
            memcpy(link, pr[(size_t)i - 1].sim, sizeof(link));
            fuse_invert(link, inv);
            fuse_compose(F, inv, G);
            memcpy(F, G, sizeof(F));
        }
        float Ff[kFuseSim], P2[12], cams[kFuseCams];
        for (int c = 0; c < kFuseSim; ++c) { Ff[c] = (float)F[c]; out->d_frames[(size_t)kFuseSim * i + c] = Ff[c]; }
        out->d_root[i] = root;
        view_points_pose(pr[(size_t)i].pose, 3, P2);
        fuse_cameras(Ff, P2, cams);
        memcpy(out->d_cams + (size_t)kFuseCams * i, cams, sizeof(cams));
    }
    out->d_counts[4] = segs;
    // ---- the chain's edges, successors, classes and lengths ----
    std::vector<unsigned long long> keys((size_t)N, kFuseNoKey);
    for (int i = 0; i + 1 < k; ++i) {
        const bool ok = fuse_link_ok(pr[(size_t)i]);
        for (int j = 0; j < pr[(size_t)i].n; ++j) {
            unsigned long long key;
            const int m = fuse_edge(pr[(size_t)i], pr[(size_t)i + 1], ok, j, key);
            if (m >= 0 && key < keys[(size_t)pr[(size_t)i + 1].offset + m]) keys[(size_t)pr[(size_t)i + 1].offset + m] = key;
        }
    }
    std::vector<int> succ((size_t)N, -1), len((size_t)N, 0);
    std::vector<uint8_t> kind((size_t)N, 0);
    for (int i = 0; i < k; ++i) {
        const bool ok = i + 1 < k && fuse_link_ok(pr[(size_t)i]);
        for (int j = 0; j < pr[(size_t)i].n; ++j) {
            const size_t g = (size_t)pr[(size_t)i].offset + j;
            float X[4];
            const bool live = fuse_live(pr[(size_t)i], j, X);
            kind[g] = !live ? 0 : (keys[g] == kFuseNoKey ? 2 : 1);
            if (i + 1 < k) {
                unsigned long long key;
                const int m = fuse_edge(pr[(size_t)i], pr[(size_t)i + 1], ok, j, key);
                if (m >= 0 && keys[(size_t)pr[(size_t)i + 1].offset + m] == key) succ[g] = pr[(size_t)i + 1].offset + m;
            }
        }
    }
    for (int g0 = 0; g0 < N; ++g0) {
        if (kind[(size_t)g0] != 2) continue;
        int L = 0;
        for (int g = g0; g >= 0 && L < k; g = succ[(size_t)g]) ++L;
        len[(size_t)g0] = L;
    }
    // ---- closure and status ----
    memset(report, 0, sizeof(*report));
    const int bad = fuse_ring_first_invalid(pr.data(), k, 0, 1);
    report->status = SFM_RING_OPEN;
    report->first_invalid = bad < k ? bad : -1;
    if (bad == k) {
        float closure[3];
        report->status = fuse_ring_closure(out->d_frames + (size_t)kFuseSim * (k - 1), pr[(size_t)k - 1].sim, p->max_closure_rotation_rad,
                                           p->max_closure_log_scale, closure);
        report->closure_log_scale = closure[0]; report->closure_rotation_rad = closure[1]; report->closure_t = closure[2];
    }
    // ---- the seam: eligible proposals, the smallest key per target, the winners' joins ----
    if (report->status == SFM_RING_CLOSED) {
        const FusePair &last = pr[(size_t)k - 1], &first = pr[0];
        const bool ok = fuse_link_ok(last);
        std::vector<int> head((size_t)last.n, kFuseRingNoHead);
        for (int j = 0; j < last.n; ++j) {
            unsigned long long key;
            int h;
            bool eligible;
            const int m = fuse_ring_proposal(pr.data(), k, last, first, ok, keys.data(), len.data(), j, key, h, eligible);
            if (m < 0) continue;
            report->seam_proposals += 1;
            if (!eligible) { report->seam_ineligible += 1; continue; }
            head[(size_t)j] = h;
            if (key < keys[(size_t)first.offset + m]) keys[(size_t)first.offset + m] = key;
        }
        for (int j = 0; j < last.n; ++j) {
            if (head[(size_t)j] == kFuseRingNoHead) continue;
            const size_t target = (size_t)first.offset + last.index[j];
            if (keys[target] != fuse_key(last.err[j], j)) continue;
            succ[(size_t)last.offset + j] = (int)target;
            kind[target] = 1;
            len[(size_t)head[(size_t)j]] += len[target];
            report->seam_tracks += 1;
        }
    }
    // ---- tracks in the order of their heads, observations in path order: counted by the stored length ----
    int T = 0, M = 0, longest = 0;
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < pr[(size_t)i].n; ++j) {
            const int g0 = pr[(size_t)i].offset + j;
            if (kind[(size_t)g0] == 0) out->d_track[g0] = -1;
            if (kind[(size_t)g0] != 2) continue;
            out->d_track_offset[T] = M;
            const int L = len[(size_t)g0];
            int pair = i, g = g0, rec = j;
            for (int s = 0; s < L; ++s) {
                out->d_track[g] = T;
                out->d_obs_cam[M] = 2 * pair; out->d_obs_record[M] = rec;
                ++M;
                if (s + 1 == L) break;
                const int nx = succ[(size_t)g];
                if (nx < 0) break;                        // not reached (fuse_ring_fill_kernel's note): the length is the path's
                pair = fuse_ring_next(pair, k);
                g = nx; rec = nx - pr[(size_t)pair].offset;
            }
            out->d_obs_cam[M] = 2 * pair + 1; out->d_obs_record[M] = rec;
            ++M;
            if (L + 1 > longest) longest = L + 1;
            ++T;
        }
    }
    out->d_track_offset[T] = M;
    out->d_counts[0] = T; out->d_counts[1] = M; out->d_counts[5] = longest;
    // ---- one point per track ----
    for (int t = 0; t < T; ++t) {
        const int o0 = out->d_track_offset[t], count = out->d_track_offset[t + 1] - o0;
        const int32_t *cam = out->d_obs_cam + o0, *recs = out->d_obs_record + o0;
        float sum[3] = { 0.0f, 0.0f, 0.0f };
        for (int o = 0; o + 1 < count; ++o) {
            const int pair = cam[o] >> 1;
            float X[4], Y[3];
            fuse_live(pr[(size_t)pair], recs[o], X);
            fuse_carry(out->d_frames + (size_t)kFuseSim * pair, X, Y);
            sum[0] += Y[0]; sum[1] += Y[1]; sum[2] += Y[2];
        }
        const float L = (float)(count - 1);
        const float start[3] = { sum[0] / L, sum[1] / L, sum[2] / L };
        auto view = [&](int o) { return fuse_view(pr[(size_t)(cam[o] >> 1)], out->d_cams, cam[o] >> 1, cam[o] & 1, recs[o]); };
        float X[4], e;
        const uint8_t flag = fuse_ring_flag(fuse_point(count, view, start, p->fuse, X, e), cam[0], cam[count - 1]);
        for (int c = 0; c < 4; ++c) out->d_points[(size_t)c * N + t] = X[c];
        out->d_flags[t] = flag;
        if (out->d_err) out->d_err[t] = e;
        const bool refined = flag == SFM_FUSE_REFINED || flag == SFM_FUSE_SEAM_REFINED;
        out->d_counts[refined ? 2 : 3] += 1;
        if (flag == SFM_FUSE_SEAM_REFINED) report->seam_refined += 1;
        if (flag == SFM_FUSE_SEAM_KEPT) report->seam_kept += 1;
    }
}

// ctypes layout check: sizeof, then the offset of every field in declaration order
int fuse_ring_layout(int which, int64_t *o)
{
    int n = 0;
#define F(T, f) o[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        o[0] = sizeof(sfm_fuse_ring_params);
        F(sfm_fuse_ring_params, fuse); F(sfm_fuse_ring_params, max_closure_rotation_rad); F(sfm_fuse_ring_params, max_closure_log_scale);
        F(sfm_fuse_ring_params, reserved);
    } else {
        o[0] = sizeof(sfm_fuse_ring_report);
        F(sfm_fuse_ring_report, status); F(sfm_fuse_ring_report, first_invalid); F(sfm_fuse_ring_report, closure_log_scale);
        F(sfm_fuse_ring_report, closure_rotation_rad); F(sfm_fuse_ring_report, closure_t); F(sfm_fuse_ring_report, seam_proposals);
        F(sfm_fuse_ring_report, seam_ineligible); F(sfm_fuse_ring_report, seam_tracks); F(sfm_fuse_ring_report, seam_refined);
        F(sfm_fuse_ring_report, seam_kept);
    }
#undef F
    return n;
}

}
