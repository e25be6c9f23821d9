// pair_fundamentals.hip -- sfm_pair_fundamentals: the F of many pairs in ONE launch.
//
// pair_fundamental_kernel (match_guided.hip) runs guided_fundamental on one lane of one block per call; a caller that refined 36
// or 630 pairs in one sfm_refine_pairs call paid 36 or 630 launches for 9 floats each.  Here lane i of a flat grid takes pair i:
// the same function on the same inputs, fp64 on one lane, rounded once -- the nine floats at d_F + 9 i are the single call's bits.
// What differs per pair, the address of its E (estimateE's, or the refined E inside the pair's refinement state) and of its K^-1,
// comes from a FundamentalJob record uploaded through a JobArray of the call's own (common.hpp), as the other batched calls do.
//
// A translation unit of its own: build/match_guided.usage.txt keeps exactly the three kernels of match_guided.hip.
#include "common.hpp"
#include "match_guided_math.hpp"

namespace sfm {

struct FundamentalJob { const float *E, *Kinv; };

__global__ __launch_bounds__(64)
void pair_fundamentals_kernel(const FundamentalJob *__restrict__ jobs, int num_pairs, int transpose, float *__restrict__ F)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= num_pairs) return;
    const FundamentalJob j = jobs[i];
    float e[9], k[9], f[9];
    for (int c = 0; c < 9; ++c) { e[c] = j.E[c]; k[c] = j.Kinv[c]; }
    guided_fundamental(e, k, transpose != 0, f);
    for (int c = 0; c < 9; ++c) F[(size_t)9 * i + c] = f[c];
}

// the pairs are of one context, each once, flushed and in the state `refined` needs (abi.hip); num_pairs >= 1
int launch_pair_fundamentals(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, int refined, float *d_F)
{
    JobArray &ja = ctx->fundamental_jobs;
    int rc = job_array_reserve(ja, (size_t)num_pairs, sizeof(FundamentalJob), ctx->stream);
    if (rc != SFM_OK) return rc;
    FundamentalJob *h = static_cast<FundamentalJob *>(ja.pinned);
    for (int i = 0; i < num_pairs; ++i)           // (the transposition rule of launch_pair_fundamental, match_guided.hip)
        h[i] = FundamentalJob{ refined ? pairs[i]->d_rstate + refine_pose_offset() + 16 : pairs[i]->d_E, pairs[i]->d_Kinv };
    rc = job_array_upload(ja, (size_t)num_pairs, sizeof(FundamentalJob), ctx->stream);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(pair_fundamentals_kernel, dim3((unsigned int)((num_pairs + 63) / 64)), dim3(64), 0, ctx->stream,
                       static_cast<const FundamentalJob *>(ja.dev), num_pairs, refined ? 0 : 1, d_F);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
