// tests/hostcheck/aligncheck.hip -- TEST HARNESS ONLY.
// Compiles the arithmetic of sfm_align_pair (cuda-sfm_amd/csrc/align_math.hpp) as HIP *host* code: the minimal solver and the
// Jacobian for the CPU tests, and a serial driver of the whole call -- the same header functions and LmControl as align.hip, the
// fp64 sums taken in candidate order -- that the CPU tests hold to the fp64 twin (tests/align_reference.py) and the GPU tests
// compare the device's outputs with.  Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/align_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace sfm;

extern "C" {

// a, b: 3 x 3 row-major (one point per row) -> sim (13); returns 1 when the sample gave a link
int aln_solve3(const float a[9], const float b[9], float sim[13])
{
    float A[3][3], B[3][3];
    memcpy(A, a, sizeof(A)); memcpy(B, b, sizeof(B));
    return align_solve3(A, B, sim) ? 1 : 0;
}

// cand: Xa (3), Xb (3), oa (2), ob (2).  out: r (4), J (28), then inlier flag and the larger pixel error at thr
void aln_jacobian(const float camA[3], const float camB[3], const float sim[13], const float cand[10], float thr, float out[34])
{
    const RefineCam KA = { camA[0], camA[1], camA[2] }, KB = { camB[0], camB[1], camB[2] };
    AlignCand c;
    memcpy(&c, cand, sizeof(c));
    float Pf[12], Pb[12];
    align_maps(sim, Pf, Pb);
    align_jacobian(KA, KB, Pf, Pb, c, out, out + 4);
    out[32] = align_inlier(KA, KB, thr, Pf, Pb, c) ? 1.0f : 0.0f;
    out[33] = sqrtf(align_sq_error(KA, KB, Pf, Pb, c));
}

// one step: d (7, double), sim (13) -> sim (13)
void aln_step(const double d[7], const float sim[13], float out[13]) { align_step(d, sim, out); }

// What sfm_align_pair computes, serially.  points_a: 4 x na, valid_a: na or null, X0a: 3 x lda, Ka: 9 (likewise b); index: na;
// p: the call's parameters (its pointers are not read).  Outputs as sfm_align_out (err, counts optional), + cand_order
// (optional, na): the record of every candidate in compact order, -1 behind the last.
void aln_run(int na, int lda, const float *points_a, const uint8_t *valid_a, const float *X0a, const float Kaf[9],
             int nb, int ldb, const float *points_b, const uint8_t *valid_b, const float *X0b, const float Kbf[9],
             const int32_t *index, const sfm_align_params *p,
             float *out_sim, uint8_t *out_inl, float *out_err, int32_t *out_counts, sfm_align_report *rep, int32_t *cand_order)
{
    const RefineCam KA = { Kaf[0], Kaf[1], Kaf[4] }, KB = { Kbf[0], Kbf[1], Kbf[4] };
    std::vector<AlignCand> cs;
    std::vector<int> slot((size_t)na, -1);
    for (int j = 0; j < na; ++j) {
        const int kb = index[j];
        if (!align_index_ok(kb, nb)) continue;
        float Xa[4], Xb[4];
        for (int c = 0; c < 4; ++c) { Xa[c] = points_a[(size_t)c * na + j]; Xb[c] = points_b[(size_t)c * nb + kb]; }
        if (!align_gate(!valid_a || valid_a[j] != 0, Xa, !valid_b || valid_b[kb] != 0, Xb)) continue;
        const float x0a[3] = { X0a[j], X0a[(size_t)lda + j], X0a[2 * (size_t)lda + j] };
        const float x0b[3] = { X0b[kb], X0b[(size_t)ldb + kb], X0b[2 * (size_t)ldb + kb] };
        AlignCand c;
        align_candidate(Xa, Xb, x0a, x0b, c);
        slot[(size_t)j] = (int)cs.size();
        cs.push_back(c);
    }
    const int m = (int)cs.size();
    if (cand_order) {
        for (int j = 0; j < na; ++j) cand_order[j] = -1;
        for (int j = 0; j < na; ++j) if (slot[(size_t)j] >= 0) cand_order[slot[(size_t)j]] = j;
    }
    // ---- RANSAC: every hypothesis' count, the first maximum ----
    const uint32_t H = p->num_hypotheses;
    uint64_t key = 0;
    float win[kAlignSim];
    for (int q = 0; q < kAlignSim; ++q) win[q] = 0.0f;
    for (uint32_t h = 0; h < H; ++h) {
        float sim[kAlignSim], Pf[12], Pb[12];
        align_hypothesis(p->seed, h, m, [&](int k, float *xa, float *xb) {
            for (int c = 0; c < 3; ++c) { xa[c] = cs[(size_t)k].Xa[c]; xb[c] = cs[(size_t)k].Xb[c]; }
        }, sim);
        align_maps(sim, Pf, Pb);
        uint32_t cnt = 0;
        for (const AlignCand &c : cs) cnt += align_inlier(KA, KB, p->threshold_px, Pf, Pb, c) ? 1u : 0u;
        if (out_counts) out_counts[h] = (int32_t)cnt;
        const uint64_t k = pack_key(cnt, h);
        if (k > key) { key = k; memcpy(win, sim, sizeof(win)); }
    }
    const uint32_t best = 0xFFFFFFFFu - (uint32_t)key;
    const int wcount = (int)(key >> 32);
    float sim[kAlignSim], Pf[12], Pb[12];
    memcpy(sim, win, sizeof(sim));
    if (!(sim[0] > 0.0f)) align_identity(sim);
    memcpy(out_sim + kAlignSim, sim, sizeof(sim));
    const bool degen = m < kAlignMinCand || wcount < kAlignMinInliers;
    align_maps(sim, Pf, Pb);
    std::vector<uint8_t> inl((size_t)m, 0);
    for (int k = 0; k < m; ++k) inl[(size_t)k] = (!degen && align_inlier(KA, KB, p->threshold_px, Pf, Pb, cs[(size_t)k])) ? 1 : 0;
    auto cost_at = [&](const float *Qf, const float *Qb, double v[2]) {
        v[0] = 0.0; v[1] = 0.0;
        for (int k = 0; k < m; ++k) {
            if (!inl[(size_t)k]) continue;
            float r[4], J[28], cost, sq;
            align_jacobian(KA, KB, Qf, Qb, cs[(size_t)k], r, J);
            align_cost(r, p->huber_px, cost, sq);
            v[0] += (double)cost; v[1] += (double)sq;
        }
    };
    double v[2];
    cost_at(Pf, Pb, v);
    LmControl lm(p->initial_lambda, v[0], v[1], degen);
    const int nin = degen ? 0 : wcount;
    rep->initial_rms_px = nin > 0 ? (float)sqrt(lm.sq / (4.0 * nin)) : 0.0f;
    while (lm.running(p->max_iterations)) {
        double sys[kAlignSys];
        for (int q = 0; q < kAlignSys; ++q) sys[q] = 0.0;
        for (int k = 0; k < m; ++k) {
            if (!inl[(size_t)k]) continue;
            float r[4], J[28], rho;
            align_jacobian(KA, KB, Pf, Pb, cs[(size_t)k], r, J);
            const float wf = refine_huber(r[0], r[1], p->huber_px, rho);
            const float wb = refine_huber(r[2], r[3], p->huber_px, rho);
            align_terms(r, J, wf, wb, [&](int q, float t) { sys[q] += (double)t; });
        }
        double S[28], d[kAlignPar];
        for (int q = 0; q < 28; ++q) S[q] = sys[q];
        for (int q = 0; q < kAlignPar; ++q) { S[symn<kAlignPar>(q, q)] += lm.lambda * sys[symn<kAlignPar>(q, q)]; d[q] = -sys[28 + q]; }
        if (!refine_cholesky<kAlignPar>(S, d)) {
            if (!lm.solve_failed()) break;
            continue;
        }
        float st[kAlignSim], Qf[12], Qb[12];
        align_step(d, sim, st);
        align_maps(st, Qf, Qb);
        cost_at(Qf, Qb, v);
        bool stop;
        if (lm.tentative(v[0], v[1], (double)p->min_rel_decrease, stop)) {
            memcpy(sim, st, sizeof(sim)); memcpy(Pf, Qf, sizeof(Pf)); memcpy(Pb, Qb, sizeof(Pb));
        }
        if (stop) break;
    }
    int nfin = 0;
    for (int j = 0; j < na; ++j) {
        const int k = slot[(size_t)j];
        float e = __builtin_inff();
        bool in = false;
        if (k >= 0) {
            e = sqrtf(align_sq_error(KA, KB, Pf, Pb, cs[(size_t)k]));
            in = !degen && align_inlier(KA, KB, p->threshold_px, Pf, Pb, cs[(size_t)k]);
        }
        if (out_err) out_err[j] = e;
        out_inl[j] = in ? 1 : 0;
        nfin += in ? 1 : 0;
    }
    memcpy(out_sim, sim, sizeof(sim));
    rep->status = lm.status;
    rep->num_candidates = m;
    rep->ransac_inliers = nin;
    rep->num_inliers = nfin;
    rep->best_hypothesis = best;
    rep->iterations = lm.iters; rep->accepted = lm.accepted;
    rep->final_rms_px = nin > 0 ? (float)sqrt(lm.sq / (4.0 * nin)) : 0.0f;
    rep->final_cost = (float)lm.cost;
    rep->lambda = (float)lm.lambda;
}

// ctypes layout check: sizeof, then the offset of every field in declaration order
int aln_layout(int which, int64_t *out)
{
    int n = 0;
#define F(T, f) out[++n] = (int64_t)offsetof(T, f)
    if (which == 0) {
        out[0] = sizeof(sfm_align_params);
        F(sfm_align_params, num_hypotheses); F(sfm_align_params, seed); F(sfm_align_params, threshold_px); F(sfm_align_params, max_iterations);
        F(sfm_align_params, huber_px); F(sfm_align_params, min_rel_decrease); F(sfm_align_params, initial_lambda);
        F(sfm_align_params, d_points_a); F(sfm_align_params, d_valid_a); F(sfm_align_params, d_points_b); F(sfm_align_params, d_valid_b);
        F(sfm_align_params, reserved);
    } else if (which == 1) {
        out[0] = sizeof(sfm_align_report);
        F(sfm_align_report, status); F(sfm_align_report, num_candidates); F(sfm_align_report, ransac_inliers); F(sfm_align_report, num_inliers);
        F(sfm_align_report, best_hypothesis); F(sfm_align_report, iterations); F(sfm_align_report, accepted);
        F(sfm_align_report, initial_rms_px); F(sfm_align_report, final_rms_px); F(sfm_align_report, final_cost); F(sfm_align_report, lambda);
    } else {
        out[0] = sizeof(sfm_align_out);
        F(sfm_align_out, d_sim); F(sfm_align_out, d_inlier); F(sfm_align_out, d_err); F(sfm_align_out, d_counts); F(sfm_align_out, d_report);
    }
#undef F
    return n;
}

}
