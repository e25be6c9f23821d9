// match_guided_body.inc -- one block of the guided matcher, a fragment of a kernel body: included by match_guided_kernel
// (match_guided.hip: block (qblock, split) of a 2-D grid) and by match_guided_jobs_kernel (match_guided_pairs.hip: a unit of a
// 1-D grid, after the block has found its job), which must have in scope
//   CT, W; sift1, nq, sift2, ndb, rows_per_split, d_F, band; ws_best, ws_second, ws_idx, tickets; qblock, split, nsplit.
// match_body's schedule (match.hip) with the rows' positions staged beside their descriptors, then the ticket merge into the
// records of sift1.  (A fragment and not a function, for match_ticket_merge.inc's reason: the one-match kernel must come out as
// the instructions it had before the many-matches kernel existed.)
    __shared__ __attribute__((aligned(16))) float lds[2][kRowsPerStage * kLdsStride];
    __shared__ __attribute__((aligned(16))) GuidedRow side[2][kRowsPerStage];
    constexpr int ld = (int)(sizeof(sfm_sift_point) / sizeof(float));
    const float *q = sift1->data;
    const float *db = sift2->data;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 31;
    const int half = lane >> 5;
    const int q0 = qblock * (CT * 32 * W);
    const int row_begin = split * rows_per_split;
    const int row_end = min(ndb, row_begin + rows_per_split);

    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = d_F[i];        // (a uniform address: scalar loads)
    const bool f_ok = guided_finite(F);

    // the first database stage is requested before the prologue, as in match_body
    const int nstage = (row_end - row_begin + kRowsPerStage - 1) / kRowsPerStage;
    float4 dbregs[16 / W][2];
    float2 dbpos[16 / W];
    if (nstage > 0) { stage_load<W>(db, ld, row_begin, row_end, dbregs); stage_load_pos<W>(sift2, row_begin, row_end, dbpos); }

    // ---- prologue: the queries' lines and limits, then their resident fragments -------------------
    EpipolarGate<CT> gate;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int p1 = q0 + (wave * CT + ct) * 32 + col;
        const float2 u1 = *reinterpret_cast<const float2 *>(&sift1[min(p1, nq - 1)].xpos);
        guided_line(F, u1.x, u1.y, gate.l[ct]);
        gate.lim1[ct] = p1 < nq && f_ok ? guided_limit(gate.l[ct], band) : 0.0f;
    }
    float bq[CT][64];
    load_queries<CT, W>(q, nq, ld, q0, lds, bq);

    Top2 top[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { top[ct].best = 0.0f; top[ct].second = 0.0f; top[ct].idx = -1; }

    // ---- main loop over database stages of 64 rows ------------------------------------------
    float4 regs[16 / W][2];
    float2 pos[16 / W];
    if (nstage > 0) { stage_store<W>(lds[0], dbregs, row_begin, row_end); stage_store_pos<W>(side[0], dbpos, row_begin, row_end, F, f_ok, band); }
    __syncthreads();
    for (int s = 0; s < nstage; ++s) {
        const float *cur = lds[s & 1];
        gate.side = side[s & 1];
        const int next_row0 = row_begin + (s + 1) * kRowsPerStage;
        if (s + 1 < nstage) { stage_load<W>(db, ld, next_row0, row_end, regs); stage_load_pos<W>(sift2, next_row0, row_end, pos); }

        // a split is a multiple of 32 rows: its last stage may hold one row tile only (wave-uniform)
        const int stage_row0 = row_begin + s * kRowsPerStage;
        if (row_end - stage_row0 > 32) stage_scores<CT, 2>(cur, bq, top, stage_row0, gate);
        else stage_scores<CT, 1>(cur, bq, top, stage_row0, gate);

        if (s + 1 < nstage) { stage_store<W>(lds[(s + 1) & 1], regs, next_row0, row_end); stage_store_pos<W>(side[(s + 1) & 1], pos, next_row0, row_end, F, f_ok, band); }
        __syncthreads();
    }

    // ---- the ticket merge into the records of sift1 ------------------------------------------
    float *const out_best = nullptr, *const out_second = nullptr;
    int *const out_idx = nullptr;
#include "match_ticket_merge.inc"
