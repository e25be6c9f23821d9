// tests/hostcheck/ringadjustcheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_adjust_ring (cuda-sfm_amd/csrc/ring_adjust_math.hpp over chain_adjust_math.hpp) as HIP *host*
// code: a serial driver of the whole call -- the same functions, LmControl and sum orders as ring_adjust.hip (a head pair's rounds
// of 64 tracks dealt to chain_system_waves(W) partial bands that are added in order, the head pairs reduced in ascending order into
// the folded band), except that inside a partial band the tracks are added one by one instead of 64 at a time -- and the pieces
// the CPU tests hold to the fp64 twin (tests/ring_adjust_reference.py).  The GPU tests compare the device's outputs with the
// driver's.  Every system the driver forms is checked against the band claim: a block of the dense reduced system that lies
// outside the folded band must be exactly zero.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/ring_adjust_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

namespace {

struct HostViews;

struct HostRing {
    std::vector<FusePair> pairs;
    int k, N, W, Wf, nb, T;
    const int32_t *track_offset, *obs_cam, *obs_record;
    const float *cams, *points;
    const uint8_t *flags;
    float huber;
    std::vector<float> state[2], Xs[2], dcf;
    std::vector<int> head, rcnt;
    std::vector<double> part, pcost, band, x, du;
    std::vector<uint8_t> used;
    RingSeg rs;

    void setup(int k_, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
               const sfm_adjust_ring_in *in, const sfm_adjust_ring_params *p);
    void start();
    void head_cost(int h, int cur, int mode, float lam);
    void system(int cur, float lam);
    void reduce(double lambda);
    bool band_holds() const;
};

struct HostViews {
    const HostRing &c;
    const float *S;
    const int32_t *cam, *rec;
    int block(int o) const { return ring_block(cam[o], c.k); }
    ChainView operator()(int o) const
    {
        const int cc = cam[o], q = cc >> 1;
        const FuseView f = fuse_view(c.pairs[(size_t)q], c.cams, q, cc & 1, rec[o]);
        const int b = ring_block(cc, c.k);
        ChainView v;
        v.K = f.K; v.x = f.x; v.y = f.y;
        v.kind = ring_kind(b);
        v.S = S + (size_t)kChainState * (b < 0 ? 0 : b);
        return v;
    }
};

// one track's terms into its head pair's partial band (ring_system_kernel's lane, the values added one track at a time): a fixed
// view, wherever it sits, is passed over
template <class Views>
void track_terms(Views &&view, int count, int h, int k, float huber, float lambda, const float X[3], int W, double *part)
{
    float Vi[6], gp[3];
    chain_point_block(count, view, huber, lambda, X, Vi, gp);
    for (int va = 0; va < count; ++va) {
        if (ring_local_block(h, va, k) < 0) continue;
        ChainJac Ja;
        float Wa[18], Ta[18], bu[12], blk[36];
        chain_jacobian(view(va), X, Ja);
        const float wa = chain_view_w(Ja, huber, Wa);
        chain_row_terms(Ja, wa, Wa, Vi, gp, Ta, bu);
        for (int i = 0; i < 6; ++i) { part[chain_part_b(W) + 6 * va + i] += (double)bu[i]; part[chain_part_u(W) + 6 * va + i] += (double)bu[6 + i]; }
        for (int vb = va; vb < count; ++vb) {
            if (ring_local_block(h, vb, k) < 0) continue;
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

void HostRing::setup(int k_, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
                     const sfm_adjust_ring_in *in, const sfm_adjust_ring_params *p)
{
    k = k_; N = 0; W = p->max_track_views; nb = k - 1; Wf = ring_band_width(W, nb);
    pairs.resize((size_t)k);
    for (int i = 0; i < k; ++i) {
        FusePair &f = pairs[(size_t)i];
        memset(&f, 0, sizeof(f));
        f.X0 = X0[i]; f.X1 = X1[i]; f.K = K[i]; f.n = n[i]; f.ld = ld[i]; f.offset = N;
        N += n[i];
    }
    track_offset = in->d_track_offset; obs_cam = in->d_obs_cam; obs_record = in->d_obs_record; cams = in->d_cams; points = in->d_points;
    flags = in->d_flags;
    T = in->d_counts[0] < N ? in->d_counts[0] : N;
    huber = p->huber_px;
    for (int b = 0; b < 2; ++b) { state[b].assign((size_t)kChainState * k, 0.0f); Xs[b].assign((size_t)4 * (N + 1), 0.0f); }
    dcf.assign((size_t)6 * k, 0.0f);
    head.assign((size_t)k + 1, 0); rcnt.assign((size_t)kRingCounts * k, 0);
    part.assign((size_t)chain_part_values(W) * k, 0.0); pcost.assign((size_t)2 * k, 0.0); band.assign((size_t)36 * Wf * k, 0.0);
    x.assign((size_t)6 * k, 0.0); du.assign((size_t)6 * k, 0.0);
    used.assign((size_t)N + 1, 0);
    rs = RingSeg();
}

// init, used, cost (mode 0) and open
void HostRing::start()
{
    for (int q = 0; q <= k; ++q) {
        int lo = 0;
        while (lo < T && (obs_cam[track_offset[lo]] >> 1) < q) ++lo;
        head[(size_t)q] = lo;
    }
    for (int q = 0; q < nb; ++q) chain_start_state(ring_kind(q), cams + (size_t)kFuseCams * q + 12, &state[0][(size_t)kChainState * q]);
    for (int t = 0; t < T; ++t) {
        const int o0 = track_offset[t], count = track_offset[t + 1] - o0;
        const HostViews view = { *this, state[0].data(), obs_cam + o0, obs_record + o0 };
        float Xin[4], X[3] = { 0.0f, 0.0f, 1.0f };
        for (int a = 0; a < 4; ++a) Xin[a] = points[(size_t)a * N + t];
        const bool u = chain_used(ring_flag(flags[t]), count, W, Xin, view, X);
        used[(size_t)t] = u ? 1 : 0;
        for (int a = 0; a < 3; ++a) Xs[0][(size_t)4 * t + a] = X[a];
        int *c = rcnt.data() + (size_t)kRingCounts * (view.cam[0] >> 1);
        if (count > W) ++c[2];
        if (!u) continue;
        ++c[0]; c[1] += count;
        if (flags[t] == SFM_FUSE_SEAM_REFINED) ++c[3];
        for (int o = 0; o < count; ++o) ++c[4 + o];
    }
    for (int h = 0; h < k; ++h) head_cost(h, 0, 0, 0.0f);
    for (int h = 0; h < k; ++h) {
        const int *c = rcnt.data() + (size_t)kRingCounts * h;
        rs.s.tracks += c[0]; rs.s.obs += c[1]; rs.s.over += c[2]; rs.seam += c[3];
    }
    rs.s.end = nb;
}

// the cost of head pair h's used tracks: ring_cost_kernel (256 threads, thread i its tracks in order; the butterfly of block_sum
// over a wavefront, then the wavefronts in order)
void HostRing::head_cost(int h, int cur, int mode, float lam)
{
    static thread_local double v[256][2];
    memset(v, 0, sizeof(v));
    for (int t = head[(size_t)h]; t < head[(size_t)h + 1]; ++t) {
        if (!used[(size_t)t]) continue;
        const int o0 = track_offset[t], count = track_offset[t + 1] - o0;
        float X[3] = { Xs[cur][(size_t)4 * t], Xs[cur][(size_t)4 * t + 1], Xs[cur][(size_t)4 * t + 2] }, cost, sq;
        if (mode) {
            const HostViews view = { *this, state[cur].data(), obs_cam + o0, obs_record + o0 };
            float Vi[6], gp[3], dp[3];
            chain_point_block(count, view, huber, lam, X, Vi, gp);
            chain_point_step(count, view, [&](int o) { return dcf.data() + 6 * (size_t)view.block(o); }, huber, X, Vi, gp, dp);
            X[0] += dp[0]; X[1] += dp[1]; X[2] += dp[2];
            for (int a = 0; a < 3; ++a) Xs[cur ^ 1][(size_t)4 * t + a] = X[a];
        }
        const HostViews trial = { *this, state[mode ? cur ^ 1 : cur].data(), obs_cam + o0, obs_record + o0 };
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
                double nbv[64];
                for (int l = 0; l < 64; ++l) nbv[l] = b[l] + b[l ^ off];
                memcpy(b, nbv, sizeof(b));
            }
            total = w == 0 ? b[0] : total + b[0];
        }
        pcost[2 * (size_t)h + q] = total;
    }
}

// the head pairs' partial bands at the committed state
void HostRing::system(int cur, float lam)
{
    const int values = chain_part_values(W), waves = chain_system_waves(W);
    std::vector<double> pw((size_t)values * waves);
    for (int h = 0; h < k; ++h) {
        double *ph = part.data() + (size_t)values * h;
        for (double &v : pw) v = 0.0;
        for (int t = head[(size_t)h]; t < head[(size_t)h + 1]; ++t) {
            if (!used[(size_t)t]) continue;
            const int o0 = track_offset[t], count = track_offset[t + 1] - o0;
            const HostViews view = { *this, state[cur].data(), obs_cam + o0, obs_record + o0 };
            const int wave = ((t - head[(size_t)h]) / 64) % waves;
            track_terms(view, count, h, k, huber, lam, &Xs[cur][(size_t)4 * t], W, pw.data() + (size_t)values * wave);
        }
        for (int q = 0; q < values; ++q) {
            double v = pw[(size_t)q];
            for (int w = 1; w < waves; ++w) v += pw[(size_t)values * w + q];
            ph[q] = v;
        }
    }
}

// the folded band, right-hand side and diag U, damped, the unit row in place
void HostRing::reduce(double lambda)
{
    const int Nn = 6 * nb;
    for (int idx = 0; idx < nb * Wf * 36; ++idx) {
        const int e = idx % 36, d = (idx / 36) % Wf, pl = idx / (36 * Wf);
        band[(size_t)idx] = pl + d < nb ? ring_reduce_block(part.data(), W, k, ring_fold_block(pl, nb), ring_fold_block(pl + d, nb), e) : 0.0;
    }
    for (int idx = 0; idx < Nn; ++idx) {
        const int P = ring_fold_block(idx / 6, nb);
        x[(size_t)idx] = -ring_reduce_row(part.data(), W, k, P, idx % 6, false);
        du[(size_t)idx] = ring_reduce_row(part.data(), W, k, P, idx % 6, true);
    }
    for (int idx = 0; idx < Nn; ++idx) {
        const size_t at = chain_band_at(Wf, idx, idx);
        band[at] = idx == 5 ? 1.0 : band[at] + lambda * du[(size_t)idx];
    }
}

// the band claim: every block (P, Q) whose folded positions lie Wf or more apart is exactly zero
bool HostRing::band_holds() const
{
    for (int P = 0; P < nb; ++P)
        for (int Q = 0; Q < nb; ++Q) {
            const int d = ring_fold_pos(P, nb) - ring_fold_pos(Q, nb);
            if ((d < 0 ? -d : d) < Wf) continue;
            for (int e = 0; e < 36; ++e)
                if (ring_reduce_block(part.data(), W, k, P, Q, e) != 0.0) return false;
        }
    return true;
}

} // namespace

extern "C" {

// What sfm_adjust_ring computes, serially.  Per pair (arrays of k): n, ld, X0, X1 (3 x ld), K (9).  in / out: the structs over
// host memory (in->pairs is not read).  accepts (64 bytes, or null): the commit decision of every iteration (1 accepted, 2
// rejected, 3 solve failed).  Returns 1, or 0 where some system it formed had a non-zero block outside the folded band.
int ring_adjust_run(int k, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
                    const sfm_adjust_ring_in *in, const sfm_adjust_ring_params *p, const sfm_adjust_ring_out *out, uint8_t *accepts)
{
    if (k < 3) return 1;
    HostRing c;
    c.setup(k, n, ld, X0, X1, K, in, p);
    const int N = c.N, T = c.T, W = c.W, nb = c.nb, Nn = 6 * nb;
    if (accepts) memset(accepts, 0, 64);
    const int ring_status = in->d_ring_report->status;
    const bool closed = ring_status == SFM_RING_CLOSED;
    int band_ok = 1;
    RingSeg &rs = c.rs;
    if (closed) {
        c.start();
        bool degenerate = false;
        for (int P = 0; P < nb; ++P) degenerate = degenerate || ring_block_obs(c.rcnt.data(), W, k, P) < (P == 0 ? kAdjMinView2 : kAdjMinView3);
        double cost = 0.0, sq = 0.0;
        for (int h = 0; h < k; ++h) { cost += c.pcost[2 * (size_t)h]; sq += c.pcost[2 * (size_t)h + 1]; }
        ChainSeg &s = rs.s;
        s.lm = LmControl((double)p->initial_lambda, cost, sq, degenerate);
        s.initial_rms = s.obs > 0 ? (float)sqrt(sq / (2.0 * (double)s.obs)) : 0.0f;
        while (chain_running(s, p->max_iterations)) {
            const int it = s.lm.iters;
            const float lam = (float)s.lm.lambda;
            c.system(s.cur, lam);
            if (!c.band_holds()) band_ok = 0;
            c.reduce(s.lm.lambda);
            if (!chain_band_factor(c.band.data(), c.Wf, Nn)) {
                if (accepts && it < 64) accepts[it] = 3;
                if (!s.lm.solve_failed()) s.stopped = 1;
                continue;
            }
            chain_band_solve(c.band.data(), c.Wf, Nn, c.x.data());
            for (int P = 0; P < nb; ++P) {
                const int pos = ring_fold_pos(P, nb);
                double dc[6];
                for (int q = 0; q < 6; ++q) { dc[q] = c.x[6 * (size_t)pos + q]; c.dcf[6 * (size_t)P + q] = (float)dc[q]; }
                chain_camera_step(ring_kind(P), dc, &c.state[s.cur][(size_t)kChainState * P], &c.state[s.cur ^ 1][(size_t)kChainState * P]);
            }
            for (int h = 0; h < k; ++h) c.head_cost(h, s.cur, 1, lam);
            cost = 0.0; sq = 0.0;
            for (int h = 0; h < k; ++h) { cost += c.pcost[2 * (size_t)h]; sq += c.pcost[2 * (size_t)h + 1]; }
            bool stop;
            const bool commit = s.lm.tentative(cost, sq, (double)p->min_rel_decrease, stop);
            if (accepts && it < 64) accepts[it] = commit ? 1 : 2;
            if (commit) s.cur ^= 1;
            if (stop) s.stopped = 1;
        }
    }
    // ---- cameras, report, columns, errors ----
    const bool through = !closed || rs.s.lm.status == SFM_REFINE_DEGENERATE;
    const float *S = c.state[closed ? rs.s.cur : 0].data();
    for (int q = 0; q < k; ++q) {
        float *o = out->d_cams + (size_t)kFuseCams * q;
        const float *ci = c.cams + (size_t)kFuseCams * q;
        for (int e = 0; e < 12; ++e) {
            o[e] = (through || q == 0) ? ci[e] : S[(size_t)kChainState * (q - 1) + e];
            o[12 + e] = through ? ci[12 + e] : (q == k - 1 ? c.cams[e] : S[(size_t)kChainState * q + e]);
        }
    }
    sfm_adjust_ring_report rep;
    memset(&rep, 0, sizeof(rep));
    rep.ring_status = ring_status;
    if (closed) {
        rep.status = rs.s.lm.status; rep.iterations = rs.s.lm.iters; rep.accepted = rs.s.lm.accepted;
        rep.num_cameras = nb; rep.num_tracks = rs.s.tracks; rep.num_seam_tracks = rs.seam; rep.num_observations = rs.s.obs;
        rep.num_over_long = rs.s.over;
        rep.initial_rms_px = rs.s.initial_rms;
        rep.final_rms_px = rs.s.obs > 0 ? (float)sqrt(rs.s.lm.sq / (2.0 * (double)rs.s.obs)) : 0.0f;
        rep.final_cost = (float)rs.s.lm.cost;
        rep.lambda = (float)rs.s.lm.lambda;
    }
    *out->d_report = rep;
    for (int t = 0; t < T; ++t) {
        const int o0 = c.track_offset[t], count = c.track_offset[t + 1] - o0;
        const bool used = closed && c.used[(size_t)t] != 0;
        out->d_used[t] = used ? 1 : 0;
        float o[4];
        for (int a = 0; a < 4; ++a) o[a] = c.points[(size_t)a * N + t];
        if (used && !through) { for (int a = 0; a < 3; ++a) o[a] = c.Xs[rs.s.cur][(size_t)4 * t + a]; o[3] = 1.0f; }
        for (int a = 0; a < 4; ++a) out->d_points[(size_t)a * N + t] = o[a];
        if (out->d_err) {
            const float X[3] = { o[0] / o[3], o[1] / o[3], o[2] / o[3] };
            const HostViews view = { c, S, c.obs_cam + o0, c.obs_record + o0 };
            out->d_err[t] = chain_error(count, view, [&](int ob) -> const float * {
                if (through) return c.cams + 12 * (size_t)view.cam[ob];
                const int b = view.block(ob);
                return b < 0 ? nullptr : S + (size_t)kChainState * b;
            }, X);
        }
    }
    return band_ok;
}

// The first system of the call (the start state, damping `lambda`) in full: dense (6 nb x 6 nb, block order, damped, the unit row
// in place, every block through ring_reduce_block: no band assumed), rhs (6 nb: -b, row 5 as the solver sees it), and x (6 nb,
// block order): the folded band's factor and solve.  info[0]: the band claim holds; info[1]: positive definite; info[2]: the
// folded band's block diagonals; info[3]: used tracks.
void ring_adjust_first_system(int k, const int32_t *n, const int32_t *ld, const float *const *X0, const float *const *X1, const float *const *K,
                              const sfm_adjust_ring_in *in, const sfm_adjust_ring_params *p, double lambda, double *dense, double *rhs, double *x,
                              int32_t *info)
{
    HostRing c;
    c.setup(k, n, ld, X0, X1, K, in, p);
    c.start();
    c.system(0, (float)lambda);
    const int nb = c.nb, Nn = 6 * nb;
    info[0] = c.band_holds() ? 1 : 0;
    c.reduce(lambda);
    for (int P = 0; P < nb; ++P)
        for (int Q = 0; Q < nb; ++Q)
            for (int e = 0; e < 36; ++e)
                dense[(size_t)(6 * P + e / 6) * Nn + 6 * Q + e % 6] = ring_reduce_block(c.part.data(), c.W, k, P, Q, e);
    for (int P = 0; P < nb; ++P)
        for (int i = 0; i < 6; ++i) {
            const int r = 6 * P + i, f = 6 * ring_fold_pos(P, nb) + i;
            dense[(size_t)r * Nn + r] = r == 5 ? 1.0 : dense[(size_t)r * Nn + r] + lambda * c.du[(size_t)f];
            rhs[r] = c.x[(size_t)f];
        }
    info[1] = chain_band_factor(c.band.data(), c.Wf, Nn) ? 1 : 0;
    if (info[1]) chain_band_solve(c.band.data(), c.Wf, Nn, c.x.data());
    for (int P = 0; P < nb; ++P)
        for (int i = 0; i < 6; ++i) x[6 * P + i] = c.x[6 * (size_t)ring_fold_pos(P, nb) + i];
    info[2] = c.Wf; info[3] = c.rs.s.tracks;
}

// One track's terms: a track of `count` views headed in pair h of a ring of k pairs, its local view v at ring view (h + v) mod k
// with K (9), state (18) and observation (2) each; the partial band of a head pair that holds this track alone
void ring_adjust_track_terms(int count, int h, int k, int W, const float *Ks, const float *states, const float *xy, const float *X, float huber,
                             float lambda, double *part)
{
    auto view = [&](int o) {
        ChainView v = { { Ks[9 * o], Ks[9 * o + 1], Ks[9 * o + 4] }, ring_kind(ring_local_block(h, o, k)), states + kChainState * o, xy[2 * o], xy[2 * o + 1] };
        return v;
    };
    for (int q = 0; q < chain_part_values(W); ++q) part[q] = 0.0;
    track_terms(view, count, h, k, huber, lambda, X, W, part);
}

// the reduction alone: block (P, Q) (36 values) of the sum of k partial bands
void ring_adjust_reduce_block(const double *part, int W, int k, int P, int Q, double *out)
{
    for (int e = 0; e < 36; ++e) out[e] = ring_reduce_block(part, W, k, P, Q, e);
}

int ring_adjust_view(int obs_cam, int k) { return ring_view(obs_cam, k); }
int ring_adjust_fold_pos(int block, int nb) { return ring_fold_pos(block, nb); }
int ring_adjust_fold_block(int pos, int nb) { return ring_fold_block(pos, nb); }
int ring_adjust_band_width(int W, int nb) { return ring_band_width(W, nb); }

// ctypes layout check: sizeof, then the offset of every field in declaration order
int ring_adjust_layout(int which, int64_t *o)
{
    int n = 0;
#define F(T, f) o[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        o[0] = sizeof(sfm_adjust_ring_params);
        F(sfm_adjust_ring_params, max_iterations); F(sfm_adjust_ring_params, huber_px); F(sfm_adjust_ring_params, min_rel_decrease);
        F(sfm_adjust_ring_params, initial_lambda); F(sfm_adjust_ring_params, max_track_views); F(sfm_adjust_ring_params, reserved);
    } else if (which == 1) {
        o[0] = sizeof(sfm_adjust_ring_in);
        F(sfm_adjust_ring_in, pairs); F(sfm_adjust_ring_in, d_root); F(sfm_adjust_ring_in, d_cams); F(sfm_adjust_ring_in, d_track_offset);
        F(sfm_adjust_ring_in, d_obs_cam); F(sfm_adjust_ring_in, d_obs_record); F(sfm_adjust_ring_in, d_points); F(sfm_adjust_ring_in, d_flags);
        F(sfm_adjust_ring_in, d_counts); F(sfm_adjust_ring_in, d_ring_report);
    } else if (which == 2) {
        o[0] = sizeof(sfm_adjust_ring_report);
        F(sfm_adjust_ring_report, ring_status); F(sfm_adjust_ring_report, status); F(sfm_adjust_ring_report, iterations);
        F(sfm_adjust_ring_report, accepted); F(sfm_adjust_ring_report, num_cameras); F(sfm_adjust_ring_report, num_tracks);
        F(sfm_adjust_ring_report, num_seam_tracks); F(sfm_adjust_ring_report, num_observations); F(sfm_adjust_ring_report, num_over_long);
        F(sfm_adjust_ring_report, initial_rms_px); F(sfm_adjust_ring_report, final_rms_px); F(sfm_adjust_ring_report, final_cost);
        F(sfm_adjust_ring_report, lambda);
    } else {
        o[0] = sizeof(sfm_adjust_ring_out);
        F(sfm_adjust_ring_out, d_cams); F(sfm_adjust_ring_out, d_points); F(sfm_adjust_ring_out, d_used); F(sfm_adjust_ring_out, d_err);
        F(sfm_adjust_ring_out, d_report);
    }
#undef F
    return n;
}

}
