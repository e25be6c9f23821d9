// pfdecodecheck.hip -- host program for tests/test_pf_decode.py: the scoring kernel's table-free decode of a survivor's bit position
// (prefilter_math.hpp, pf_pack_code_closed) against the table's entries (pf_pack_code), and the flush's walk over a survivor mask
// (clz -> decode -> clear) through both.
//   output: 32 lines "b closed table", then one line "walks <masks> mismatches <count>"; exit status 1 on any difference.
//   pfdecodecheck sums COUNT LD: one line "tile <points> tiles <n> sums <0|1>" -- which epilogue the launcher picks for COUNT
//   hypotheses over a pair of LD correspondences (prefilter_lds.hpp: pf_tile_points, pf_sums_counts_at).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../cuda-sfm_amd/csrc/prefilter_math.hpp"
#include "../../cuda-sfm_amd/csrc/prefilter_lds.hpp"

// the walk of ransac_prefilter.hip's flush over one ring entry's mask: (row offset, step) of every survivor, first bit first
template <typename Decode>
static int walk(uint32_t mask, Decode decode, uint32_t out[32])
{
    int k = 0;
    while (mask) {
        const int b = __builtin_clz(mask);
        mask &= ~(0x80000000u >> b);
        const uint32_t code = decode(b);
        out[k++] = (code & 31u) | ((code >> 5) << 8);       // row | step << 8
    }
    return k;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::strcmp(argv[1], "sums") == 0) {
        const unsigned count = (unsigned)std::strtoul(argv[2], nullptr, 10);
        const int ld = std::atoi(argv[3]);
        const int tile = sfm::pf_tile_points(ld, sfm::kPfTileMax);
        std::printf("tile %d tiles %d sums %d\n", tile, (ld + tile - 1) / tile, sfm::pf_sums_counts_at(count, ld, tile) ? 1 : 0);
        return 0;
    }
    unsigned char table[32];
    for (int b = 0; b < 32; ++b) table[b] = (unsigned char)sfm::pf_pack_code(b);          // what the kernel's staging writes to LDS
    int bad = 0;
    for (int b = 0; b < 32; ++b) {
        std::printf("%d %u %u\n", b, sfm::pf_pack_code_closed(b), (unsigned)table[b]);
        bad += sfm::pf_pack_code_closed(b) != table[b];
    }
    // every mask with one, two or three survivors
    long masks = 0, mismatches = 0;
    auto check = [&](uint32_t m) {
        uint32_t a[32], t[32];
        const int na = walk(m, [](int b) { return sfm::pf_pack_code_closed(b); }, a);
        const int nt = walk(m, [&](int b) { return (uint32_t)table[b]; }, t);
        bool same = na == nt && na == __builtin_popcount(m);
        for (int k = 0; same && k < na; ++k) same = a[k] == t[k];
        ++masks;
        mismatches += same ? 0 : 1;
    };
    for (int i = 0; i < 32; ++i) {
        check(1u << i);
        for (int j = i + 1; j < 32; ++j) {
            check((1u << i) | (1u << j));
            for (int k = j + 1; k < 32; ++k) check((1u << i) | (1u << j) | (1u << k));
        }
    }
    std::printf("walks %ld mismatches %ld\n", masks, mismatches);
    return (bad || mismatches) ? 1 : 0;
}
