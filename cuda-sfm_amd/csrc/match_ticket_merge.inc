// match_ticket_merge.inc -- the ticket merge of the exact MFMA matchers, a fragment of a kernel body: included at the end of
// match_body (match.hip) and of match_guided_body.inc (the guided matcher's kernels), which must have in scope
//   CT, W; top[CT]; wave, col, half; nq, q0, qblock, split, nsplit; ws_best, ws_second, ws_idx, tickets; out_best, out_second,
//   out_idx (any of them null); sift1, sift2.
// It merges the two k-parity halves of each column, emits the split's partial, and lets the LAST split block of this query block to
// arrive merge the partials (ascending database ranges) and write the results, either to plain arrays or into the SiftPoint fields
// MatchSiftData updates (matching.cu:391-395): no merge launch, and no block waits for another.  (A fragment and not a function:
// the compiler simplifies a function's body before it is inlined, without what the kernel knows about q0, and the one-match
// kernels would come out as different instructions.)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        Top2 o;
        o.best = __shfl_xor(top[ct].best, 32);
        o.second = __shfl_xor(top[ct].second, 32);
        o.idx = __shfl_xor(top[ct].idx, 32);
        const Top2 mrg = top2_merge(top[ct], o);
        const int p1 = q0 + (wave * CT + ct) * 32 + col;
        if (half == 0 && p1 < nq) {
            // agent-scope stores (written through this XCD's L2): the block that merges may sit on another XCD
            const size_t w = (size_t)split * nq + p1;
            __hip_atomic_store(&ws_best[w], mrg.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ws_second[w], mrg.second, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ws_idx[w], mrg.idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // Ordering without a fence: the partials are agent-scope stores, acknowledged (vmcnt) before the block's ticket is drawn;
    // the merging block reads them with agent-scope loads after its own ticket came back.
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = atomicAdd(&tickets[qblock], 1u);
        s_last = (t == (unsigned int)nsplit - 1u) ? 1 : 0;
        if (s_last) __hip_atomic_store(&tickets[qblock], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next call
    }
    __syncthreads();
    if (!s_last) return;
    for (int k = threadIdx.x; k < CT * 32 * W; k += blockDim.x) {
        const int p1 = q0 + k;
        if (p1 >= nq) break;
        Top2 t{ __hip_atomic_load(&ws_best[p1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                __hip_atomic_load(&ws_second[p1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                __hip_atomic_load(&ws_idx[p1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) };
        // sixteen splits' partials are requested before the first is merged: one memory round trip per sixteen splits, not
        // per split (the loads are atomics, which the compiler never hoists over the merge of the previous split); one-match
        // launches have up to 16 or 17 splits for the small sizes, i.e. ONE trip
        constexpr int kMergeBatch = 16;
        for (int sp0 = 1; sp0 < nsplit; sp0 += kMergeBatch) {
            Top2 part[kMergeBatch];
#pragma unroll
            for (int u = 0; u < kMergeBatch; ++u) {
                const size_t w = (size_t)min(sp0 + u, nsplit - 1) * nq + p1;
                part[u].best = __hip_atomic_load(&ws_best[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                part[u].second = __hip_atomic_load(&ws_second[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                part[u].idx = __hip_atomic_load(&ws_idx[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int u = 0; u < kMergeBatch; ++u)
                if (sp0 + u < nsplit) t = top2_merge(t, part[u]);
        }
        match_emit(p1, t, out_best, out_second, out_idx, sift1, sift2);
    }
