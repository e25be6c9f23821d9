// prefilter_lds.hpp -- the LDS footprint of the pre-filter scoring block (ransac_prefilter.hip): tile size, per-wavefront tables and the
// map of one block's dynamic shared memory.  Plain host + device arithmetic, in a header of its own so that the host-compiled check
// (tests/hostcheck/pfldscheck.hip, tests/test_register_budget.py) computes the very number launch_score_prefilter asks for: the block's
// LDS is dynamic, so the code object does not carry it.
#pragma once
#include "prefilter_record.hpp"

namespace sfm {

constexpr int kPfTileMax = 1024;         // points per tile at most; a launch picks the smallest multiple of 32 that covers the points with the fewest
                                         // tiles (pf_tile_points).  The band rule's 80 bytes per point would allow 1536 (3 tiles for 4096 points, 11 for
                                         // 16384: fewer, longer passes) -- measured SLOWER at every size (profiles/r05_ab_tile_size.txt: 0.369 against
                                         // 0.360 ms at 2^20 x 4096, 0.068 against 0.058 at a rank's share): coarser passes, longer tails.  AB build,
                                         // reserved[1] == 7: tiles of up to 1536 points.
constexpr int kPfWaves = 16;             // wavefronts per block (LDS is laid out for 16; the kernel also runs with 12, see launch_score_prefilter)
constexpr int kPfRing = 128;             // survivor ring entries (8 bytes) per wavefront: < 64 waiting + 64 appended per step;
                                         // a flush re-queues at most 64 more, onto slots its own 64 entries have just left

// LDS map
constexpr int kPfERow = 10;                                   // floats per hypothesis reserved in the E table (9 used): etab[32 k + row] -- a lane's nine
                                                              // reads for a random row hit bank (row mod 32) + const, so distinct rows never conflict
                                                              // (row-major 40-byte rows put rows r and r + 16 on the same banks: 19 % of the LDS cycles were conflicts)
// A wavefront's table holds the rows of ONE unit of its work: 32 (a pass), or 64 for the per-tile rule's paired passes (lane l = hypothesis
// 64 j + l, two scans of 32 rows each): etab[rows k + row].  A scan's own survivors touch 32 consecutive rows of one half, so their
// distinct rows sit on distinct banks exactly as with 32 rows.  The ring is carried from a pair's first scan into its second (an entry
// names its scan), so a flush that mixes carried and new entries can read rows r and r + 32 of one component together: a two-way
// conflict, possible only in the flushes that still hold carried entries -- the first one or two of a second scan and their re-queues.
// Measured: 5 % more bank-conflict cycles per launch (0.87e6 of 9e7 LDS-active cycles) with 4.7 % fewer LDS instructions
// (profiles/NOTES_r12.md) -- not worth another layout.
constexpr int kPfPassRows = 32, kPfPairRows = 64;
constexpr int pf_wave_bytes(int rows) { return rows * kPfERow * 4 + rows * 4; }
// The map for a tile of `tile` points (a multiple of 32); an even number of 32-point blocks is staged (the scan takes two per iteration).
template <int RULE> struct PfLds {
    static constexpr int kFragsPerBlock = RULE == kPfRuleG ? 3 : 2;
    static constexpr int kBlockBytes = kFragsPerBlock * 64 * 16;   // one 32-point block: [n k-step 0 | n k-step 1 (| G)][lane][8 fp16]
    static constexpr int kFrag = 0;
    static constexpr int kTileMax = kPfTileMax;
    int staged, pts, ring, wave, next, lut, bytes;
    // rows: hypotheses in a wavefront's table; the default is the product's largest block (the band rules' paired passes)
    __host__ __device__ explicit PfLds(int tile, int ring_entries = kPfRing, int entry_bytes = 8, int rows = RULE == kPfRuleG ? kPfPassRows : kPfPairRows)
    {
        staged = (tile + 63) & ~63;                           // points staged: whole iterations of two blocks (beyond `tile`: padding)
        pts = kFrag + (staged / 32) * kBlockBytes;            // float4 (x2x, x1x, x2y, x1y) per point
        ring = pts + staged * 16;                             // the wavefronts' survivor rings, 1024 bytes each, 1024-byte aligned (a slot's
                                                              // address is (offset & 1023) | base: one v_and_or_b32): staged is a multiple of 64
        ring = (ring + ring_entries * entry_bytes - 1) & ~(ring_entries * entry_bytes - 1);
        wave = ring + kPfWaves * ring_entries * entry_bytes;  // per wavefront: E table 9 x rows floats (component-major), rows counters
        next = wave + kPfWaves * pf_wave_bytes(rows);         // the block's pass counter
        lut = next + 16;                                      // packed scan: survivor bit -> (accumulator row, step), 32 bytes (pf_pack_code);
                                                              // paired passes: (survivor bit, half, scan) -> (row of 64, step), 128 bytes (pf_ring_lut_entry)
        bytes = lut + kPfRingLutBytes;                        // (the same map for every instance: the 32-byte table sits at its start)
    }
};
static_assert(kPfRing * 8 == 1024, "ring slots are addressed with (offset & 1023) | base");

// Tile size of a launch: the fewest tiles of at most `tmax` points, equal sizes rounded up to 32 (4096 points: 4 x 1024; 4608: 5 x 928).
static inline int pf_tile_points(int ld, int tmax)
{
    const int ntiles = (ld + tmax - 1) / tmax;
    const int t = ((ld + ntiles - 1) / ntiles + 31) & ~31;
    return t < 32 ? 32 : t;
}

// Which epilogue a launch of `count` hypotheses over tiles of `tile` points runs (ransac_prefilter.hip: pf_tail_var): from this many
// (hypothesis, tile) partial counts on, the counts are summed without an answer and ransac_argmax_counts makes the keys behind the
// launch; below it the extra launch costs more than the passes save (profiles/NOTES_r09.md).  In this header so that the host-compiled
// check (tests/hostcheck/pfdecodecheck.hip, tests/test_pf_decode.py) asks the very function the launcher asks.
constexpr unsigned long long kPfSumCountsMin = 1ull << 21;
static inline bool pf_sums_counts_at(unsigned count, int ld, int tile)
{
    return (unsigned long long)count * (unsigned long long)((ld + tile - 1) / tile) >= kPfSumCountsMin;
}

// Which launches of the per-tile rule prepare two passes at once (ransac_prefilter.hip: kPair).  A pair doubles the grain of the
// hand-out: the wavefronts of a block finish within one PAIR of each other, and what the shared preparation saves must pay for that
// tail.  A launch of c partial counts gives each wavefront of a full chip (256 blocks of 16) c / 2^18 pairs.  Measured on bench.py's
// pipelined step at 4096 points (profiles/NOTES_r11.md): 64 pairs per wavefront 4.1 % shorter, 16 pairs (the headline) 2.8 % shorter,
// 8 pairs (524288 hypotheses) 1.2 % LONGER -- so pairs from 2^22 partial counts on, single passes with the summing epilogue below.
constexpr unsigned long long kPfPairPassesMin = 1ull << 22;
static inline bool pf_pairs_passes_at(unsigned count, int ld, int tile)
{
    return (unsigned long long)count * (unsigned long long)((ld + tile - 1) / tile) >= kPfPairPassesMin;
}

} // namespace sfm
