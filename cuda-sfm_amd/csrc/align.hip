// align.hip -- sfm_align_pair / sfm_align_pairs (gfx950): the similarity that carries pair A's frame into pair B's, by a 3-point
// RANSAC over the points the two pairs share and a 7-parameter Levenberg-Marquardt.  Arithmetic: align_math.hpp (shared with
// the host build of the CPU tests); damping, accept test and stop rules: LmControl (refine_math.hpp).
//
// Four launches on the context's stream, no host synchronisation:
//   align_gate_kernel    ONE block of 1024 threads per link, in rounds of 1024 consecutive records: thread i of a round reads
//                        record base + i (coalesced: index, A's column, then B's column where the index is a record of B), and
//                        block_scan gives its place among the round's candidates, as adjust_solve_kernel compacts its used set.
//                        The order is the record order whatever the scheduling.  (The registration's gate gives every thread a
//                        contiguous range of records: its loads are strided by that range.  A grid-wide scan would need a
//                        second launch or a block-to-block hand-over for a few thousand records per link; the batched call has
//                        one block per link anyway.)  Writes the candidates compactly -- (X_A, o_B.x), (X_B, o_B.y), o_A: 40
//                        bytes -- the record -> candidate map and the count.
//   align_solve_kernel   one lane per hypothesis: sample_distinct<3>, the two triads, 13 floats (s, R, t) into a
//                        per-hypothesis SoA array (52 bytes stored per hypothesis; the zero link for a degenerate sample), and
//                        clears the hypothesis' accumulator (hypothesis 0 the key) for the scoring launch behind it.  The
//                        rotation stays a matrix: the scoring lane would otherwise rebuild it from a quaternion, and 52 x 4096
//                        bytes are written once and read `splits` times out of L2.
//   align_score_kernel   register_score_kernel's shape: grid (hypotheses / 256) x splits, one lane per hypothesis, a contiguous
//                        share of the candidates staged through LDS in tiles of 1024 (40 KiB), one 64-bit integer atomic per
//                        hypothesis (count | arrivals), the completing lane stores the count and folds the packed key.  Integer
//                        atomics only: counts do not depend on the split.
//   align_refine_kernel  ONE block of 256 threads per link: the winner's inliers, the LM chain (fp32 per-candidate terms, 35
//                        fp64 sums per thread in a fixed order by block_sum, Cholesky on one lane), then every record's larger
//                        pixel error, the final flag and the report.
// Many links in one call (launch_align_pairs): the same four bodies over an array of AlignArgs in device memory.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "align_math.hpp"

namespace sfm {

constexpr int kAlnGateThreads = 1024;
constexpr int kAlnHypBlock = 256;         // hypotheses per scoring block (one per lane)
constexpr int kAlnTile = 1024;            // candidates per LDS stage of the scoring kernel (40 KiB)
constexpr int kAlnThreads = 256;          // the LM block
constexpr int kAlnWaves = kAlnThreads / 64;

// words at the head of pair->d_lwork
constexpr int kAlnKey = 0;                // uint64 packed arg-max key
constexpr int kAlnCount = 2;              // int number of candidates
constexpr int kAlnHead = 4;

struct AlignArgs {
    const float *pa, *pb;                 // 4 x na, 4 x nb
    const uint8_t *va, *vb;               // na, nb, or null
    const float *X0a, *X0b;               // 3 x lda, 3 x ldb: view-1 observations of the two pairs
    const float *Ka, *Kb;
    const int32_t *index;                 // na: record of A -> record of B, or outside [0, nb)
    int na, nb, lda, ldb;
    float thr;
    uint32_t seed, H;
    int max_iter;
    float huber, min_rel, lambda0;
    int *head;                            // kAlnHead words
    float4 *Ca, *Cb;                      // per candidate: (X_A, o_B.x), (X_B, o_B.y)
    float2 *Co;                           // per candidate: o_A
    int *slot;                            // record j -> candidate k or -1
    uint8_t *inl;                         // per candidate: inlier of the winner
    unsigned long long *acc;              // H: (arrived << 32) | count
    float *sims;                          // 13 x H
    sfm_align_out out;
};

__device__ __forceinline__ AlignCand load_cand(const float4 A, const float4 B, const float2 o)
{
    AlignCand c;
    c.Xa[0] = A.x; c.Xa[1] = A.y; c.Xa[2] = A.z;
    c.Xb[0] = B.x; c.Xb[1] = B.y; c.Xb[2] = B.z;
    c.oa[0] = o.x; c.oa[1] = o.y;
    c.ob[0] = A.w; c.ob[1] = B.w;
    return c;
}

__device__ __forceinline__ void align_gate_block(const AlignArgs &a)
{
    __shared__ int s_scan[kAlnGateThreads / 64 + 1];
    const int tid = threadIdx.x;
    const size_t na = (size_t)a.na, nb = (size_t)a.nb;
    int m = 0;
    for (int base = 0; base < a.na; base += kAlnGateThreads) {
        const int j = base + tid;
        bool ok = false;
        float Xa[4], Xb[4];
        int kb = -1;
        if (j < a.na) {
            kb = a.index[j];
            if (align_index_ok(kb, a.nb)) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { Xa[c] = a.pa[c * na + j]; Xb[c] = a.pb[c * nb + kb]; }
                ok = align_gate(!a.va || a.va[j] != 0, Xa, !a.vb || a.vb[kb] != 0, Xb);
            }
        }
        const int k = m + block_scan<kAlnGateThreads / 64>(ok ? 1 : 0, s_scan);
        m += s_scan[kAlnGateThreads / 64];
        if (j < a.na) {
            a.slot[j] = ok ? k : -1;
            if (ok) {
                const float x0a[3] = { a.X0a[j], a.X0a[(size_t)a.lda + j], a.X0a[2 * (size_t)a.lda + j] };
                const float x0b[3] = { a.X0b[kb], a.X0b[(size_t)a.ldb + kb], a.X0b[2 * (size_t)a.ldb + kb] };
                AlignCand c;
                align_candidate(Xa, Xb, x0a, x0b, c);
                a.Ca[k] = make_float4(c.Xa[0], c.Xa[1], c.Xa[2], c.ob[0]);
                a.Cb[k] = make_float4(c.Xb[0], c.Xb[1], c.Xb[2], c.ob[1]);
                a.Co[k] = make_float2(c.oa[0], c.oa[1]);
            }
        }
        __syncthreads();                                  // s_scan is read above and rewritten by the next round
    }
    if (tid == 0) a.head[kAlnCount] = m;
}

__device__ __forceinline__ void align_solve_block(const AlignArgs &a)
{
    const uint32_t h = blockIdx.x * kAlnHypBlock + threadIdx.x;
    if (h == 0) *reinterpret_cast<unsigned long long *>(a.head + kAlnKey) = 0ull;
    if (h >= a.H) return;
    a.acc[h] = 0ull;
    const int m = a.head[kAlnCount];
    float sim[kAlignSim];
    align_hypothesis(a.seed, h, m, [&](int k, float *xa, float *xb) {
        const float4 A = a.Ca[k], B = a.Cb[k];
        xa[0] = A.x; xa[1] = A.y; xa[2] = A.z;
        xb[0] = B.x; xb[1] = B.y; xb[2] = B.z;
    }, sim);
    float *o = a.sims + h;
#pragma unroll
    for (int q = 0; q < kAlignSim; ++q) o[(size_t)q * a.H] = sim[q];
}

// blockIdx.y of gridDim.y candidate shares (a share that is empty -- a link with few candidates -- still adds its arrival)
__device__ __forceinline__ void align_score_block(const AlignArgs &a)
{
    __shared__ float4 sA[kAlnTile];
    __shared__ float4 sB[kAlnTile];
    __shared__ float2 sO[kAlnTile];
    const uint32_t h = blockIdx.x * kAlnHypBlock + threadIdx.x;
    const int m = a.head[kAlnCount];
    const int splits = gridDim.y;
    const int chunk = (m + splits - 1) / splits;
    const int lo = min(m, (int)blockIdx.y * chunk), hi = min(m, lo + chunk);
    const RefineCam KA = { a.Ka[0], a.Ka[1], a.Ka[4] }, KB = { a.Kb[0], a.Kb[1], a.Kb[4] };
    float sim[kAlignSim], Pf[12], Pb[12];
#pragma unroll
    for (int q = 0; q < kAlignSim; ++q) sim[q] = h < a.H ? a.sims[(size_t)q * a.H + h] : 0.0f;
    align_maps(sim, Pf, Pb);
    int cnt = 0;
    for (int base = lo; base < hi; base += kAlnTile) {
        const int len = min(kAlnTile, hi - base);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += kAlnHypBlock) { sA[k] = a.Ca[base + k]; sB[k] = a.Cb[base + k]; sO[k] = a.Co[base + k]; }
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const AlignCand c = load_cand(sA[k], sB[k], sO[k]);
            cnt += align_inlier(KA, KB, a.thr, Pf, Pb, c) ? 1 : 0;
        }
    }
    unsigned long long key = 0ull;
    if (h < a.H) {
        const unsigned long long old = atomicAdd(&a.acc[h], (1ull << 32) | (unsigned long long)cnt);
        if ((uint32_t)(old >> 32) == (uint32_t)(splits - 1)) {
            const uint32_t total = (uint32_t)old + (uint32_t)cnt;
            if (a.out.d_counts) a.out.d_counts[h] = (int)total;
            key = pack_key(total, h);
        }
    }
    key = wave_max(key);
    if ((threadIdx.x & 63) == 0 && key) atomicMax(reinterpret_cast<unsigned long long *>(a.head + kAlnKey), key);
}

__device__ __forceinline__ void align_refine_block(const AlignArgs &a)
{
    __shared__ double s_part[kAlnWaves * kAlignSys];
    __shared__ double s_tot[kAlignSys];
    __shared__ float s_sim[kAlignSim], s_try[kAlignSim];
    __shared__ int s_go, s_degen, s_cnt[kAlnWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefineCam KA = { uniform(a.Ka[0]), uniform(a.Ka[1]), uniform(a.Ka[4]) };
    const RefineCam KB = { uniform(a.Kb[0]), uniform(a.Kb[1]), uniform(a.Kb[4]) };
    const int m = a.head[kAlnCount];
    const unsigned long long key = *reinterpret_cast<const unsigned long long *>(a.head + kAlnKey);
    const uint32_t best = 0xFFFFFFFFu - (uint32_t)key;
    const int wcount = (int)(key >> 32);

    // ---- the winner: its link (the identity when no sample gave one), whether there is anything to refine ----
    if (tid == 0) {
        float sim[kAlignSim];
#pragma unroll
        for (int q = 0; q < kAlignSim; ++q) sim[q] = best < a.H ? a.sims[(size_t)q * a.H + best] : 0.0f;
        if (!(sim[0] > 0.0f)) align_identity(sim);
#pragma unroll
        for (int q = 0; q < kAlignSim; ++q) { s_sim[q] = sim[q]; a.out.d_sim[kAlignSim + q] = sim[q]; }
        s_degen = (m < kAlignMinCand || wcount < kAlignMinInliers) ? 1 : 0;
    }
    __syncthreads();
    const bool degen = s_degen != 0;
    float sim[kAlignSim], Pf[12], Pb[12];
#pragma unroll
    for (int q = 0; q < kAlignSim; ++q) sim[q] = uniform(s_sim[q]);
    align_maps(sim, Pf, Pb);

    // ---- the winner's inliers: the candidates the LM runs over ----
    for (int k = tid; k < m; k += kAlnThreads) {
        const AlignCand c = load_cand(a.Ca[k], a.Cb[k], a.Co[k]);
        a.inl[k] = (!degen && align_inlier(KA, KB, a.thr, Pf, Pb, c)) ? 1 : 0;
    }
    __syncthreads();
    const float huber = a.huber;
    auto cost_at = [&](const float *Qf, const float *Qb, double v[2]) {
        v[0] = 0.0; v[1] = 0.0;
        for (int k = tid; k < m; k += kAlnThreads) {
            if (!a.inl[k]) continue;
            const AlignCand c = load_cand(a.Ca[k], a.Cb[k], a.Co[k]);
            float r[4], J[28], cost, sq;
            align_jacobian(KA, KB, Qf, Qb, c, r, J);
            align_cost(r, huber, cost, sq);
            v[0] += (double)cost;
            v[1] += (double)sq;
        }
    };
    {
        double v[2];
        cost_at(Pf, Pb, v);
        block_sum<kAlnWaves>(v, s_part, s_tot);
    }
    LmControl lm(a.lambda0, s_tot[0], s_tot[1], degen);
    const int nin = degen ? 0 : wcount;
    const float initial_rms = nin > 0 ? (float)sqrt(lm.sq / (4.0 * nin)) : 0.0f;

    while (lm.running(a.max_iter)) {
        // ---- the weighted normal equations at the committed link ----
        double sys[kAlignSys];
#pragma unroll
        for (int q = 0; q < kAlignSys; ++q) sys[q] = 0.0;
        for (int k = tid; k < m; k += kAlnThreads) {
            if (!a.inl[k]) continue;
            const AlignCand c = load_cand(a.Ca[k], a.Cb[k], a.Co[k]);
            float r[4], J[28], rho;
            align_jacobian(KA, KB, Pf, Pb, c, r, J);
            const float wf = refine_huber(r[0], r[1], huber, rho);
            const float wb = refine_huber(r[2], r[3], huber, rho);
            align_terms(r, J, wf, wb, [&](int q, float v) { sys[q] += (double)v; });
        }
        block_sum<kAlnWaves>(sys, s_part, s_tot);
        // ---- the step on one lane: (H + lambda diag H) d = -g ----
        if (tid == 0) {
            double S[28], d[kAlignPar];
#pragma unroll
            for (int q = 0; q < 28; ++q) S[q] = s_tot[q];
#pragma unroll
            for (int q = 0; q < kAlignPar; ++q) { S[symn<kAlignPar>(q, q)] += lm.lambda * s_tot[symn<kAlignPar>(q, q)]; d[q] = -s_tot[28 + q]; }
            const bool ok = refine_cholesky<kAlignPar>(S, d);
            s_go = ok ? 1 : 0;
            if (ok) {
                float cur[kAlignSim], nxt[kAlignSim];
#pragma unroll
                for (int q = 0; q < kAlignSim; ++q) cur[q] = s_sim[q];
                align_step(d, cur, nxt);
#pragma unroll
                for (int q = 0; q < kAlignSim; ++q) s_try[q] = nxt[q];
            }
        }
        __syncthreads();
        if (!s_go) {                                      // not positive definite: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        // ---- the cost of the tentative link ----
        float st[kAlignSim], Qf[12], Qb[12];
#pragma unroll
        for (int q = 0; q < kAlignSim; ++q) st[q] = uniform(s_try[q]);
        align_maps(st, Qf, Qb);
        double v[2];
        cost_at(Qf, Qb, v);
        block_sum<kAlnWaves>(v, s_part, s_tot);
        bool stop;
        if (lm.tentative(s_tot[0], s_tot[1], (double)a.min_rel, stop)) {     // accepted: commit the link
#pragma unroll
            for (int q = 0; q < kAlignSim; ++q) sim[q] = st[q];
#pragma unroll
            for (int q = 0; q < 12; ++q) { Pf[q] = Qf[q]; Pb[q] = Qb[q]; }
            __syncthreads();                              // every lane has read s_sim / s_try for this iteration
            if (tid < kAlignSim) s_sim[tid] = s_try[tid];
            __syncthreads();
        }
        if (stop) break;
    }

    // ---- every record under the final link: the larger pixel error, the final flag ----
    int mine = 0;
    for (int j = tid; j < a.na; j += kAlnThreads) {
        const int k = a.slot[j];
        float e = __builtin_inff();
        bool in = false;
        if (k >= 0) {
            const AlignCand c = load_cand(a.Ca[k], a.Cb[k], a.Co[k]);
            e = sqrtf(align_sq_error(KA, KB, Pf, Pb, c));
            in = !degen && align_inlier(KA, KB, a.thr, Pf, Pb, c);
        }
        if (a.out.d_err) a.out.d_err[j] = e;
        a.out.d_inlier[j] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        int nfin = 0;
        for (int w = 0; w < kAlnWaves; ++w) nfin += s_cnt[w];
#pragma unroll
        for (int q = 0; q < kAlignSim; ++q) a.out.d_sim[q] = sim[q];
        sfm_align_report rep;
        rep.status = lm.status;
        rep.num_candidates = m;
        rep.ransac_inliers = nin;
        rep.num_inliers = nfin;
        rep.best_hypothesis = best;
        rep.iterations = lm.iters; rep.accepted = lm.accepted;
        rep.initial_rms_px = initial_rms;
        rep.final_rms_px = nin > 0 ? (float)sqrt(lm.sq / (4.0 * nin)) : 0.0f;
        rep.final_cost = (float)lm.cost;
        rep.lambda = (float)lm.lambda;
        *a.out.d_report = rep;
    }
}

__global__ __launch_bounds__(kAlnGateThreads)
void align_gate_kernel(AlignArgs a) { align_gate_block(a); }

__global__ __launch_bounds__(kAlnHypBlock)
void align_solve_kernel(AlignArgs a) { align_solve_block(a); }

__global__ __launch_bounds__(kAlnHypBlock)
void align_score_kernel(AlignArgs a) { align_score_block(a); }

__global__ __launch_bounds__(kAlnThreads)
void align_refine_kernel(AlignArgs a) { align_refine_block(a); }

// ---- many links: job blockIdx.x (gate, refine) / blockIdx.y (solve) / blockIdx.z (score) of `jobs` ----
__device__ __forceinline__ AlignArgs load_job(const AlignArgs *__restrict__ jobs, const unsigned int job)
{
    AlignArgs a = jobs[job];
    a.pa = global_ptr(a.pa); a.pb = global_ptr(a.pb); a.va = global_ptr(a.va); a.vb = global_ptr(a.vb);
    a.X0a = global_ptr(a.X0a); a.X0b = global_ptr(a.X0b); a.Ka = global_ptr(a.Ka); a.Kb = global_ptr(a.Kb); a.index = global_ptr(a.index);
    a.head = global_ptr(a.head); a.Ca = global_ptr(a.Ca); a.Cb = global_ptr(a.Cb); a.Co = global_ptr(a.Co); a.slot = global_ptr(a.slot);
    a.inl = global_ptr(a.inl); a.acc = global_ptr(a.acc); a.sims = global_ptr(a.sims);
    a.out.d_sim = global_ptr(a.out.d_sim); a.out.d_inlier = global_ptr(a.out.d_inlier); a.out.d_err = global_ptr(a.out.d_err);
    a.out.d_counts = global_ptr(a.out.d_counts); a.out.d_report = global_ptr(a.out.d_report);
    return a;
}

// Every block of the four runs its body to the end (the solve body's lanes past H leave on their own, behind no barrier).
__global__ __launch_bounds__(kAlnGateThreads)
void align_gate_pairs_kernel(const AlignArgs *__restrict__ jobs)
{
    const AlignArgs a = load_job(jobs, blockIdx.x);
    align_gate_block(a);
}

__global__ __launch_bounds__(kAlnHypBlock)
void align_solve_pairs_kernel(const AlignArgs *__restrict__ jobs)
{
    const AlignArgs a = load_job(jobs, blockIdx.y);
    align_solve_block(a);
}

__global__ __launch_bounds__(kAlnHypBlock)
void align_score_pairs_kernel(const AlignArgs *__restrict__ jobs)
{
    const AlignArgs a = load_job(jobs, blockIdx.z);
    align_score_block(a);
}

__global__ __launch_bounds__(kAlnThreads)
void align_refine_pairs_kernel(const AlignArgs *__restrict__ jobs)
{
    const AlignArgs a = load_job(jobs, blockIdx.x);
    align_refine_block(a);
}

// index[j] = match of record j where it passes the registration's gate, else -1
__global__ __launch_bounds__(256)
void align_index_kernel(const sfm_sift_point *__restrict__ sift, int n, float min_score, float max_ambiguity, int32_t *__restrict__ index)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const sfm_sift_point &s = sift[j];
    index[j] = (s.match >= 0 && s.score > min_score && s.ambiguity < max_ambiguity) ? s.match : -1;
}

// pair->d_lwork for cap_points records: the arrays of `a` inside it; returns its size in bytes
static size_t align_work_layout(void *buffer, int cap_points, AlignArgs &a)
{
    const size_t cap = (size_t)cap_points;
    Carver w(buffer);
    a.head = w.take<int>(kAlnHead, 16);
    a.Ca = w.take<float4>(cap, 16);
    a.Cb = w.take<float4>(cap, 16);
    a.Co = w.take<float2>(cap, 8);
    a.slot = w.take<int>(cap, 4);
    a.inl = w.take<uint8_t>(cap);
    return w.used;
}

// pair->d_lhyp for `hyps` hypotheses, likewise
static size_t align_hyp_layout(void *buffer, size_t hyps, AlignArgs &a)
{
    Carver h(buffer);
    a.acc = h.take<unsigned long long>(hyps, 8);
    a.sims = h.take<float>(kAlignSim * hyps, 4);
    return h.used;
}

static void align_args(sfm_pair *pa, sfm_pair *pb, const AlignInputs &in, const sfm_align_params &p, const sfm_align_out &out, AlignArgs &a)
{
    a.pa = in.points_a; a.va = in.valid_a; a.pb = in.points_b; a.vb = in.valid_b;
    a.X0a = pa->d_X[0]; a.X0b = pb->d_X[0];
    a.Ka = pa->d_K; a.Kb = pb->d_K;
    a.index = in.index;
    a.na = pa->n; a.nb = pb->n; a.lda = pa->ld; a.ldb = pb->ld;
    a.thr = p.threshold_px;
    a.seed = p.seed; a.H = p.num_hypotheses;
    a.max_iter = p.max_iterations; a.huber = p.huber_px; a.min_rel = p.min_rel_decrease; a.lambda0 = p.initial_lambda;
    align_work_layout(pa->d_lwork, pa->cap_points, a);
    align_hyp_layout(pa->d_lhyp, pa->cap_lhyps, a);            // sized for the largest num_hypotheses seen
    a.out = out;
}

// candidate shares of a scoring launch: about four blocks per CU over all its links, each share at least 128 candidates when every
// record of the largest link is one (register_splits' rule)
static int align_splits(int num_cus, int hblocks, int num_jobs, int nmax)
{
    const long long blocks = (long long)hblocks * num_jobs;
    int splits = (int)((4LL * num_cus + blocks - 1) / blocks);
    const int max_splits = nmax / 128 > 1 ? nmax / 128 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    return splits;
}

int launch_align(sfm_pair *pa, sfm_pair *pb, const AlignInputs &in, const sfm_align_params &p, const sfm_align_out &out)
{
    AlignArgs a;
    align_args(pa, pb, in, p, out, a);
    hipStream_t st = pa->ctx->stream;
    const int hblocks = (int)((p.num_hypotheses + kAlnHypBlock - 1) / kAlnHypBlock);
    const int splits = align_splits(pa->ctx->num_cus, hblocks, 1, pa->n);
    hipLaunchKernelGGL(align_gate_kernel, dim3(1), dim3(kAlnGateThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_solve_kernel, dim3(hblocks), dim3(kAlnHypBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_score_kernel, dim3(hblocks, splits), dim3(kAlnHypBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_refine_kernel, dim3(1), dim3(kAlnThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_align_pairs(sfm_ctx *ctx, sfm_pair *const *as, sfm_pair *const *bs, int num_links, const AlignInputs *in, const sfm_align_params &p,
                       const sfm_align_out *outs)
{
    hipStream_t st = ctx->stream;
    const AlignArgs *d_jobs = nullptr;
    int nmax = 0;                                         // links with the most records first: the one-block gates and LM chains are dispatched in job order
    const int rc = job_array_stage(ctx->align_jobs, num_links, st, [&](int i) { return as[i]->n; },
                                   [&](AlignArgs &job, int i) { align_args(as[i], bs[i], in[i], p, outs[i], job); }, &d_jobs, &nmax);
    if (rc != SFM_OK) return rc;
    const int hblocks = (int)((p.num_hypotheses + kAlnHypBlock - 1) / kAlnHypBlock);
    const int splits = align_splits(ctx->num_cus, hblocks, num_links, nmax);                 // ONE for the launch: counts do not depend on it
    hipLaunchKernelGGL(align_gate_pairs_kernel, dim3(num_links), dim3(kAlnGateThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_solve_pairs_kernel, dim3(hblocks, num_links), dim3(kAlnHypBlock), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_score_pairs_kernel, dim3(hblocks, splits, num_links), dim3(kAlnHypBlock), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(align_refine_pairs_kernel, dim3(num_links), dim3(kAlnThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_align_index(sfm_ctx *ctx, const sfm_sift_point *d_sift, int n, float min_score, float max_ambiguity, int32_t *d_index)
{
    hipLaunchKernelGGL(align_index_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_sift, n, min_score, max_ambiguity, d_index);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

size_t align_work_bytes(int cap_points)
{
    AlignArgs a;
    return align_work_layout(nullptr, cap_points, a);
}

size_t align_hyp_bytes(size_t num_hypotheses)
{
    AlignArgs a;
    return align_hyp_layout(nullptr, num_hypotheses, a);
}

} // namespace sfm
