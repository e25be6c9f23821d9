// tests/hostcheck/chainadjustcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_adjust_chain (cuda-sfm_amd/csrc/chain_adjust_math.hpp) as HIP *host* code: the header's functions
// one by one and a serial driver of the whole call -- the same functions, LmControl and sum orders as chain_adjust.hip (a head
// pair's rounds of 64 tracks dealt to chain_system_waves(W) partial bands that are added in order), except that inside a partial
// band the tracks are added one by one instead of 64 at a time -- that the CPU tests hold to the fp64
// twin (tests/chain_adjust_reference.py) and the GPU tests compare the device's outputs with.  Nothing in the product loads this
// library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/chain_adjust_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

namespace {

struct HostChain {
    std::vector<FusePair> pairs;
    int k, N, W;
    const int32_t *root, *track_offset, *obs_cam, *obs_record;
    const float *cams;
};

struct HostViews {
    const HostChain &c;
    const float *S;
    const int32_t *cam, *rec;
    int block(int o) const { return chain_block(cam[o], c.root[cam[o] >> 1]); }
    ChainView operator()(int o) const
    {
        const int cc = cam[o], q = cc >> 1;
        const FuseView f = fuse_view(c.pairs[(size_t)q], c.cams, q, cc & 1, rec[o]);
        const int b = chain_block(cc, c.root[q]);
        ChainView v;
        v.K = f.K; v.x = f.x; v.y = f.y;
        v.kind = b < 0 ? kChainFixed : (c.root[b] == b ? kChainRoot : kChainFree);
        v.S = S + (size_t)kChainState * (b < 0 ? 0 : b);
        return v;
    }
};

// one track's terms into its head pair's partial band (chain_system_kernel's lane, the values added one track at a time)
void track_terms(const HostViews &view, int count, int first, float huber, float lambda, const float X[3], int W, double *part)
{
    float Vi[6], gp[3];
    chain_point_block(count, view, huber, lambda, X, Vi, gp);
    for (int va = first; va < count; ++va) {
        ChainJac Ja;
        float Wa[18], Ta[18], bu[12], blk[36];
        chain_jacobian(view(va), X, Ja);
        const float wa = chain_view_w(Ja, huber, Wa);
        chain_row_terms(Ja, wa, Wa, Vi, gp, Ta, bu);
        for (int i = 0; i < 6; ++i) { part[chain_part_b(W) + 6 * va + i] += (double)bu[i]; part[chain_part_u(W) + 6 * va + i] += (double)bu[6 + i]; }
        for (int vb = va; vb < count; ++vb) {
            if (vb == va) chain_block_terms(Ja, wa, Ta, Wa, true, blk);
            else {
                ChainJac Jb;
                float Wb[18];
                chain_jacobian(view(vb), X, Jb);
                chain_view_w(Jb, huber, Wb);
                chain_block_terms(Ja, wa, Ta, Wb, false, blk);
            }
            for (int e = 0; e < 36; ++e) part[chain_part_block(W, va, vb) + e] += (double)blk[e];
        }
    }
}

} // namespace

extern "C" {

// What sfm_adjust_chain computes, serially.  Per pair (arrays of k): n, ld, X0, X1 (3 x ld), K (9).  in / out: the structs over
// host memory (in->pairs is not read).  accepts (k x 64 bytes, or null): per segment root the commit decision of every iteration
// (1 accepted, 2 rejected, 3 solve failed), for the accept sequences of the tests.
void chain_adjust_run(int k, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
                      const sfm_adjust_chain_in *in, const sfm_adjust_chain_params *p, const sfm_adjust_chain_out *out, uint8_t *accepts)
{
    if (k <= 0) return;
    HostChain c;
    c.pairs.resize((size_t)k);
    c.k = k; c.N = 0; c.W = p->max_track_views;
    for (int i = 0; i < k; ++i) {
        FusePair &f = c.pairs[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = X0[i]; f.X1 = X1[i]; f.K = K[i]; f.n = n[i]; f.ld = ld[i]; f.offset = c.N;
        c.N += n[i];
    }
    c.root = in->d_root; c.track_offset = in->d_track_offset; c.obs_cam = in->d_obs_cam; c.obs_record = in->d_obs_record; c.cams = in->d_cams;
    const int N = c.N, W = c.W, T = in->d_counts[0] < N ? in->d_counts[0] : N;
    const int values = chain_part_values(W);
    const float huber = p->huber_px;
    std::vector<float> state[2] = { std::vector<float>((size_t)kChainState * k), std::vector<float>((size_t)kChainState * k) };
    std::vector<float> Xs[2] = { std::vector<float>((size_t)4 * (N + 1)), std::vector<float>((size_t)4 * (N + 1)) };
    std::vector<ChainSeg> seg((size_t)k);
    std::vector<int> head((size_t)k + 1), blockobs((size_t)k, 0);
    std::vector<double> part((size_t)values * k), pcost((size_t)2 * k), band((size_t)36 * W * k), x((size_t)6 * k), du((size_t)6 * k);
    std::vector<float> dcf((size_t)6 * k);
    if (accepts) memset(accepts, 0, (size_t)64 * k);
    // ---- start states, head ranges ----
    for (int q = 0; q <= k; ++q) {
        int lo = 0;
        while (lo < T && (c.obs_cam[c.track_offset[lo]] >> 1) < q) ++lo;
        head[(size_t)q] = lo;
    }
    for (int q = 0; q < k; ++q) chain_start_state(c.root[q] == q ? kChainRoot : kChainFree, c.cams + (size_t)kFuseCams * q + 12, &state[0][(size_t)kChainState * q]);
    // ---- used tracks ----
    for (int t = 0; t < T; ++t) {
        const int o0 = c.track_offset[t], count = c.track_offset[t + 1] - o0;
        const HostViews view = { c, state[0].data(), c.obs_cam + o0, c.obs_record + o0 };
        float Xin[4], X[3] = { 0.0f, 0.0f, 1.0f };
        for (int a = 0; a < 4; ++a) Xin[a] = in->d_points[(size_t)a * N + t];
        const bool used = chain_used(in->d_flags[t], count, W, Xin, view, X);
        out->d_used[t] = used ? 1 : 0;
        for (int a = 0; a < 3; ++a) Xs[0][(size_t)4 * t + a] = X[a];
        ChainSeg &s = seg[(size_t)c.root[view.cam[0] >> 1]];
        if (count > W) ++s.over;
        if (!used) continue;
        ++s.tracks; s.obs += count;
        for (int o = 0; o < count; ++o) if (view.block(o) >= 0) ++blockobs[(size_t)view.block(o)];
    }
    // the cost of head pair h's used tracks: chain_cost_kernel (256 threads, thread i its tracks in order; the butterfly of block_sum
    // over a wavefront, then the wavefronts in order)
    auto head_cost = [&](int h, int cur, int mode, float lam) {
        double v[256][2];
        memset(v, 0, sizeof(v));
        for (int t = head[(size_t)h]; t < head[(size_t)h + 1]; ++t) {
            if (!out->d_used[t]) continue;
            const int o0 = c.track_offset[t], count = c.track_offset[t + 1] - o0;
            float X[3] = { Xs[cur][(size_t)4 * t], Xs[cur][(size_t)4 * t + 1], Xs[cur][(size_t)4 * t + 2] }, cost, sq;
            if (mode) {
                const HostViews view = { c, state[cur].data(), c.obs_cam + o0, c.obs_record + o0 };
                float Vi[6], gp[3], dp[3];
                chain_point_block(count, view, huber, lam, X, Vi, gp);
                chain_point_step(count, view, [&](int o) { return dcf.data() + 6 * (size_t)view.block(o); }, huber, X, Vi, gp, dp);
                X[0] += dp[0]; X[1] += dp[1]; X[2] += dp[2];
                for (int a = 0; a < 3; ++a) Xs[cur ^ 1][(size_t)4 * t + a] = X[a];
            }
            const HostViews trial = { c, state[mode ? cur ^ 1 : cur].data(), c.obs_cam + o0, c.obs_record + o0 };
            chain_cost(count, trial, huber, X, cost, sq);
            const int lane = (t - head[(size_t)h]) % 256;
            v[lane][0] += (double)cost; v[lane][1] += (double)sq;
        }
        for (int q = 0; q < 2; ++q) {
            double total = 0.0;
            for (int w = 0; w < 4; ++w) {
                double b[64];
                for (int l = 0; l < 64; ++l) b[l] = v[64 * w + l][q];
                for (int off = 32; off > 0; off >>= 1) {
                    double nb[64];
                    for (int l = 0; l < 64; ++l) nb[l] = b[l] + b[l ^ off];
                    memcpy(b, nb, sizeof(b));
                }
                total = w == 0 ? b[0] : total + b[0];
            }
            pcost[2 * (size_t)h + q] = total;
        }
    };
    for (int h = 0; h < k; ++h) head_cost(h, 0, 0, 0.0f);
    // ---- the segments, one after the other ----
    for (int p0 = 0; p0 < k; ++p0) {
        if (c.root[p0] != p0) continue;
        ChainSeg &s = seg[(size_t)p0];
        int p1 = p0 + 1;
        while (p1 < k && c.root[p1] == p0) ++p1;
        bool degenerate = blockobs[(size_t)p0] < kAdjMinView2;
        for (int q = p0 + 1; q < p1; ++q) degenerate = degenerate || blockobs[(size_t)q] < kAdjMinView3;
        double cost = 0.0, sq = 0.0;
        for (int h = p0; h < p1; ++h) { cost += pcost[2 * (size_t)h]; sq += pcost[2 * (size_t)h + 1]; }
        s.end = p1;
        s.lm = LmControl((double)p->initial_lambda, cost, sq, degenerate);
        s.initial_rms = s.obs > 0 ? (float)sqrt(sq / (2.0 * (double)s.obs)) : 0.0f;
        const int nb = p1 - p0, Nn = 6 * nb;
        double *B = band.data() + (size_t)36 * W * p0, *xs = x.data() + (size_t)6 * p0, *dus = du.data() + (size_t)6 * p0;
        while (chain_running(s, p->max_iterations)) {
            const int it = s.lm.iters;
            const float lam = (float)s.lm.lambda;
            // the system
            const int waves = chain_system_waves(W);
            std::vector<double> pw((size_t)values * waves);
            for (int h = p0; h < p1; ++h) {
                double *ph = part.data() + (size_t)values * h;
                for (double &v : pw) v = 0.0;
                for (int t = head[(size_t)h]; t < head[(size_t)h + 1]; ++t) {
                    if (!out->d_used[t]) continue;
                    const int o0 = c.track_offset[t], count = c.track_offset[t + 1] - o0;
                    const HostViews view = { c, state[s.cur].data(), c.obs_cam + o0, c.obs_record + o0 };
                    const int wave = ((t - head[(size_t)h]) / 64) % waves;
                    track_terms(view, count, h == p0 ? 1 : 0, huber, lam, &Xs[s.cur][(size_t)4 * t], W, pw.data() + (size_t)values * wave);
                }
                for (int q = 0; q < values; ++q) {
                    double v = pw[(size_t)q];
                    for (int w = 1; w < waves; ++w) v += pw[(size_t)values * w + q];
                    ph[q] = v;
                }
            }
            for (int idx = 0; idx < nb * W * 36; ++idx) {
                const int e = idx % 36, d = (idx / 36) % W, pl = idx / (36 * W);
                B[idx] = pl + d < nb ? chain_reduce_block(part.data(), W, p0, p1, pl, d, e) : 0.0;
            }
            for (int idx = 0; idx < Nn; ++idx) {
                xs[idx] = -chain_reduce_row(part.data(), W, p0, p1, idx / 6, idx % 6, false);
                dus[idx] = chain_reduce_row(part.data(), W, p0, p1, idx / 6, idx % 6, true);
            }
            for (int idx = 0; idx < Nn; ++idx) {
                const size_t at = chain_band_at(W, idx, idx);
                B[at] = idx == 5 ? 1.0 : B[at] + s.lm.lambda * dus[idx];
            }
            if (!chain_band_factor(B, W, Nn)) {
                if (accepts && it < 64) accepts[(size_t)64 * p0 + it] = 3;
                if (!s.lm.solve_failed()) s.stopped = 1;
                continue;
            }
            chain_band_solve(B, W, Nn, xs);
            for (int pl = 0; pl < nb; ++pl) {
                double dc[6];
                for (int q = 0; q < 6; ++q) { dc[q] = xs[6 * pl + q]; dcf[6 * (size_t)(p0 + pl) + q] = (float)dc[q]; }
                chain_camera_step(pl == 0 ? kChainRoot : kChainFree, dc, &state[s.cur][(size_t)kChainState * (p0 + pl)],
                                  &state[s.cur ^ 1][(size_t)kChainState * (p0 + pl)]);
            }
            for (int h = p0; h < p1; ++h) head_cost(h, s.cur, 1, lam);
            cost = 0.0; sq = 0.0;
            for (int h = p0; h < p1; ++h) { cost += pcost[2 * (size_t)h]; sq += pcost[2 * (size_t)h + 1]; }
            bool stop;
            const bool commit = s.lm.tentative(cost, sq, (double)p->min_rel_decrease, stop);
            if (accepts && it < 64) accepts[(size_t)64 * p0 + it] = commit ? 1 : 2;
            if (commit) s.cur ^= 1;
            if (stop) s.stopped = 1;
        }
    }
    // ---- cameras, reports, columns, errors ----
    for (int q = 0; q < k; ++q) {
        const int r = c.root[q];
        const ChainSeg &s = seg[(size_t)r];
        const bool degenerate = s.lm.status == SFM_REFINE_DEGENERATE;
        float *o = out->d_cams + (size_t)kFuseCams * q;
        const float *ci = c.cams + (size_t)kFuseCams * q, *S = state[s.cur].data();
        for (int e = 0; e < 12; ++e) {
            o[e] = (degenerate || r == q) ? ci[e] : S[(size_t)kChainState * (q - 1) + e];
            o[12 + e] = degenerate ? ci[12 + e] : S[(size_t)kChainState * q + e];
        }
        sfm_adjust_chain_report rep;
        memset(&rep, 0, sizeof(rep));
        rep.root = r;
        if (r == q) {
            rep.status = s.lm.status; rep.iterations = s.lm.iters; rep.accepted = s.lm.accepted;
            rep.num_cameras = s.end - q; rep.num_tracks = s.tracks; rep.num_observations = s.obs; rep.num_over_long = s.over;
            rep.initial_rms_px = s.initial_rms;
            rep.final_rms_px = s.obs > 0 ? (float)sqrt(s.lm.sq / (2.0 * (double)s.obs)) : 0.0f;
            rep.final_cost = (float)s.lm.cost;
            rep.lambda = (float)s.lm.lambda;
        }
        out->d_reports[q] = rep;
    }
    for (int t = 0; t < T; ++t) {
        const int o0 = c.track_offset[t], count = c.track_offset[t + 1] - o0;
        const ChainSeg &s = seg[(size_t)c.root[c.obs_cam[o0] >> 1]];
        const bool degenerate = s.lm.status == SFM_REFINE_DEGENERATE;
        float o[4];
        for (int a = 0; a < 4; ++a) o[a] = in->d_points[(size_t)a * N + t];
        if (out->d_used[t] && !degenerate) { for (int a = 0; a < 3; ++a) o[a] = Xs[s.cur][(size_t)4 * t + a]; o[3] = 1.0f; }
        for (int a = 0; a < 4; ++a) out->d_points[(size_t)a * N + t] = o[a];
        if (out->d_err) {
            const float X[3] = { o[0] / o[3], o[1] / o[3], o[2] / o[3] };
            const float *S = state[s.cur].data();
            const HostViews view = { c, S, c.obs_cam + o0, c.obs_record + o0 };
            out->d_err[t] = chain_error(count, view, [&](int ob) -> const float * {
                if (degenerate) return c.cams + 12 * (size_t)view.cam[ob];
                const int b = view.block(ob);
                return b < 0 ? nullptr : S + (size_t)kChainState * b;
            }, X);
        }
    }
}

// ---- the header's functions one by one ----
// kind: kChainFixed / Root / Free; S: 18 floats; out: r (2), Jp (6), Jc (12)
void chain_adjust_jacobian(int kind, const float *K, const float *S, float x, float y, const float *X, float *out)
{
    ChainView v = { { K[0], K[1], K[4] }, kind, S, x, y };
    ChainJac J;
    chain_jacobian(v, X, J);
    memcpy(out, J.r, 8); memcpy(out + 2, J.Jp, 24); memcpy(out + 8, J.Jc, 48);
}
void chain_adjust_residual(int kind, const float *K, const float *S, float x, float y, const float *X, float *r)
{
    ChainView v = { { K[0], K[1], K[4] }, kind, S, x, y };
    chain_residual(v, X, r);
}
void chain_adjust_start_state(int kind, const float *P, float *s) { chain_start_state(kind, P, s); }
void chain_adjust_camera_step(int kind, const double *dc, const float *s, float *o) { chain_camera_step(kind, dc, s, o); }

// One track's terms: count views with kinds[], Ks (9 each), states (18 each), xy (2 each); the partial band of a head pair that
// holds this track alone (chain_part_values(W) doubles); first: 1 where view 0 is the fixed camera
void chain_adjust_track_terms(int count, int first, int W, const int32_t *kinds, const float *Ks, const float *states, const float *xy, const float *X,
                              float huber, float lambda, double *part)
{
    auto view = [&](int o) {
        ChainView v = { { Ks[9 * o], Ks[9 * o + 1], Ks[9 * o + 4] }, kinds[o], states + kChainState * o, xy[2 * o], xy[2 * o + 1] };
        return v;
    };
    for (int q = 0; q < chain_part_values(W); ++q) part[q] = 0.0;
    float Vi[6], gp[3];
    chain_point_block(count, view, huber, lambda, X, Vi, gp);
    for (int va = first; va < count; ++va) {
        ChainJac Ja;
        float Wa[18], Ta[18], bu[12], blk[36];
        chain_jacobian(view(va), X, Ja);
        const float wa = chain_view_w(Ja, huber, Wa);
        chain_row_terms(Ja, wa, Wa, Vi, gp, Ta, bu);
        for (int i = 0; i < 6; ++i) { part[chain_part_b(W) + 6 * va + i] += (double)bu[i]; part[chain_part_u(W) + 6 * va + i] += (double)bu[6 + i]; }
        for (int vb = va; vb < count; ++vb) {
            ChainJac Jb;
            float Wb[18];
            chain_jacobian(view(vb), X, Jb);
            chain_view_w(Jb, huber, Wb);
            chain_block_terms(Ja, wa, Ta, Wb, vb == va, blk);
            for (int e = 0; e < 36; ++e) part[chain_part_block(W, va, vb) + e] += (double)blk[e];
        }
    }
}

int chain_adjust_part_values(int W) { return chain_part_values(W); }
int chain_adjust_part_block(int W, int a, int b) { return chain_part_block(W, a, b); }
int64_t chain_adjust_band_at(int W, int r, int j) { return (int64_t)chain_band_at(W, r, j); }
int chain_adjust_block(int obs_cam, int root_of_pair) { return chain_block(obs_cam, root_of_pair); }

// the banded factor and solve on a band of nb blocks (36 W nb doubles, in place) and a right-hand side (6 nb); 0: not positive definite
int chain_adjust_band_solve(double *B, int W, int nb, double *x)
{
    if (!chain_band_factor(B, W, 6 * nb)) return 0;
    chain_band_solve(B, W, 6 * nb, x);
    return 1;
}

// ctypes layout check: sizeof, then the offset of every field in declaration order
int chain_adjust_layout(int which, int64_t *o)
{
    int n = 0;
#define F(T, f) o[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        o[0] = sizeof(sfm_adjust_chain_params);
        F(sfm_adjust_chain_params, max_iterations); F(sfm_adjust_chain_params, huber_px); F(sfm_adjust_chain_params, min_rel_decrease);
        F(sfm_adjust_chain_params, initial_lambda); F(sfm_adjust_chain_params, max_track_views); F(sfm_adjust_chain_params, reserved);
    } else if (which == 1) {
        o[0] = sizeof(sfm_adjust_chain_in);
        F(sfm_adjust_chain_in, pairs); F(sfm_adjust_chain_in, d_root); F(sfm_adjust_chain_in, d_cams); F(sfm_adjust_chain_in, d_track_offset);
        F(sfm_adjust_chain_in, d_obs_cam); F(sfm_adjust_chain_in, d_obs_record); F(sfm_adjust_chain_in, d_points); F(sfm_adjust_chain_in, d_flags);
        F(sfm_adjust_chain_in, d_counts);
    } else if (which == 2) {
        o[0] = sizeof(sfm_adjust_chain_report);
        F(sfm_adjust_chain_report, root); F(sfm_adjust_chain_report, status); F(sfm_adjust_chain_report, iterations); F(sfm_adjust_chain_report, accepted);
        F(sfm_adjust_chain_report, num_cameras); F(sfm_adjust_chain_report, num_tracks); F(sfm_adjust_chain_report, num_observations);
        F(sfm_adjust_chain_report, num_over_long); F(sfm_adjust_chain_report, initial_rms_px); F(sfm_adjust_chain_report, final_rms_px);
        F(sfm_adjust_chain_report, final_cost); F(sfm_adjust_chain_report, lambda);
    } else {
        o[0] = sizeof(sfm_adjust_chain_out);
        F(sfm_adjust_chain_out, d_cams); F(sfm_adjust_chain_out, d_points); F(sfm_adjust_chain_out, d_used); F(sfm_adjust_chain_out, d_err);
        F(sfm_adjust_chain_out, d_reports);
    }
#undef F
    return n;
}

}
