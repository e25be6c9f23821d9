// TEST SUPPORT: the per-tile rule's operands built once per hypothesis (prefilter_record.hpp: pf_tile_operands_full, what a lane of
// the paired passes runs) against the per-half build of the single passes (pf_tile_operands_half with the divisor each half bounds and
// the one the other half hands over), host-compiled for tests/test_pf_pair_host.py.  The hardware's reciprocal and square root are the
// header's own host stand-ins (pf_rcp, pf_sqrt), the same on both sides.
#include <cstdint>
#include <cstring>
#include "../../cuda-sfm_amd/csrc/prefilter_record.hpp"

namespace {

// the box of a tile from the maxima of (x, -x, y, -y, u, -u, v, -v) over its feature-carrying points, through the words the scatter kernel leaves
sfm::PfBox box_of(const float ext[8], float B)
{
    uint32_t w[8];
    for (int k = 0; k < 8; ++k) w[k] = sfm::pf_order_bits(ext[k]);
    return sfm::pf_box_from_bits(w, B);
}

uint16_t bits16(_Float16 v) { uint16_t b; std::memcpy(&b, &v, 2); return b; }

}

extern "C" {

// n hypotheses (E: 9 floats each) x the four flag words 0..3 (scan, b-safe) over one tile; returns how many of the n x 4 x 2 x 16 fp16
// values differ, the first differing (hypothesis, flags, half, slot) in first_bad[4]; *nonzero counts hypotheses whose sigma is not 0
// (so that a test can tell the comparison was not one of zeros)
long pfpair_compare(const float *E, int n, float thr, float B, const float ext[8], int *first_bad, long *nonzero)
{
    const sfm::PfBox box = box_of(ext, B);
    long bad = 0;
    *nonzero = 0;
    for (int i = 0; i < n; ++i) {
        const float *e = E + 9 * (size_t)i;
        float dn, lin;
        sfm::prefilter_band_hyp_terms(e, B, dn, lin);
        for (uint32_t flags = 0; flags < 4; ++flags) {
            sfm::h8 x0, y0, x1, y1;
            sfm::pf_tile_operands_full(e, flags, dn, lin, thr, B, box, x0, y0, x1, y1);
            bool any = false;
            for (int half = 0; half < 2; ++half) {
                // what the two halves of a wavefront compute and exchange (pf_tile_operands: __shfl_xor(d_mine, 32))
                const float d_mine = sfm::prefilter_band_divisor_max(e, lin, box, half);
                const float d_other = sfm::prefilter_band_divisor_max(e, lin, box, half ^ 1);
                sfm::h8 n0, n1;
                sfm::pf_tile_operands_half(e, flags, dn, thr, B, half, d_mine, d_other, n0, n1);
                const sfm::h8 &f0 = half ? y0 : x0, &f1 = half ? y1 : x1;
                for (int j = 0; j < 16; ++j) {
                    const uint16_t want = bits16(j < 8 ? n0[j] : n1[j - 8]), got = bits16(j < 8 ? f0[j] : f1[j - 8]);
                    any = any || (want & 0x7FFFu) != 0 && !(half == 1 && j == 11);       // (k-slot 27 is the constant pad marker)
                    if (want != got) {
                        if (bad == 0) { first_bad[0] = i; first_bad[1] = (int)flags; first_bad[2] = half; first_bad[3] = j; }
                        ++bad;
                    }
                }
            }
            if (flags == 0 && any) ++*nonzero;
        }
    }
    return bad;
}

// the decoded box, for the test's own sanity check of the tiles it builds
void pfpair_box(const float ext[8], float B, float out[8])
{
    const sfm::PfBox b = box_of(ext, B);
    const float v[8] = { b.xlo, b.xhi, b.ylo, b.yhi, b.ulo, b.uhi, b.vlo, b.vhi };
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

}
