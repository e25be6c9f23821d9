// tests/hostcheck/matchguidedcheck.hip -- TEST HARNESS ONLY.
// Compiles the gate of sfm_match_guided and the arithmetic of sfm_pair_fundamental (cuda-sfm_amd/csrc/match_guided_math.hpp) as
// HIP *host* code: a serial driver of the whole call over the header's gate -- with a top-2 rule, a score chain and emit formulae
// of its OWN, in plain C, none of them taken from match_common.hpp -- and the header's pieces one by one.  The CPU tests hold it
// to the fp64 twin (tests/match_guided_reference.py), the GPU tests compare the device's records with it field by field.
// Nothing in the product loads this library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/match_guided_math.hpp"
#include "../../include/sfm_amd.h"
#include <math.h>

using namespace sfm;

extern "C" {

// What sfm_match_guided computes, serially: sift1's five match fields are written in place.  gated = 0 skips the gate
// (sfm_match's result, for the comparisons with the plain match).
void mg_run(sfm_sift_point *sift1, int n1, const sfm_sift_point *sift2, int n2, const float *F, float band, int gated)
{
    const bool f_ok = guided_finite(F);
    for (int p1 = 0; p1 < n1; ++p1) {
        sfm_sift_point *a = sift1 + p1;
        float l[3];
        guided_line(F, a->xpos, a->ypos, l);
        const float lim1 = f_ok ? guided_limit(l, band) : 0.0f;
        float best = 0.0f, second = 0.0f;
        int idx = -1;
        for (int p2 = 0; p2 < n2; ++p2) {                       // ascending row
            const sfm_sift_point *b = sift2 + p2;
            if (gated) {
                float lt[3];
                guided_line_t(F, b->xpos, b->ypos, lt);
                const float lim2 = f_ok ? guided_limit(lt, band) : 0.0f;
                if (!guided_pass(guided_residual(l, b->xpos, b->ypos), lim1, lim2)) continue;
            }
            float s = 0.0f;
            for (int d = 0; d < 128; ++d) s = fmaf(a->data[d], b->data[d], s);      // the d = 0..127 fused chain
            if (s > best) { second = best; best = s; idx = p2; }
            else if (s > second) second = s;
        }
        a->score = best;
        a->match = idx;
        a->match_xpos = idx >= 0 ? sift2[idx].xpos : 0.0f;
        a->match_ypos = idx >= 0 ? sift2[idx].ypos : 0.0f;
        a->ambiguity = second / (best + 1e-6f);
    }
}

// the header's pieces
void mg_line(const float *F, float x, float y, float *l) { guided_line(F, x, y, l); }
void mg_line_t(const float *F, float x, float y, float *l) { guided_line_t(F, x, y, l); }
float mg_limit(const float *l, float band) { return guided_limit(l, band); }
float mg_residual(const float *l, float x2, float y2) { return guided_residual(l, x2, y2); }
int mg_pass(float d, float lim1, float lim2) { return guided_pass(d, lim1, lim2) ? 1 : 0; }
int mg_finite(const float *F) { return guided_finite(F) ? 1 : 0; }

// the whole gate for one pair of positions, as the driver applies it
int mg_gate(const float *F, float band, float x1, float y1, float x2, float y2)
{
    const bool f_ok = guided_finite(F);
    float l[3], lt[3];
    guided_line(F, x1, y1, l);
    guided_line_t(F, x2, y2, lt);
    return guided_pass(guided_residual(l, x2, y2), f_ok ? guided_limit(l, band) : 0.0f, f_ok ? guided_limit(lt, band) : 0.0f) ? 1 : 0;
}

// the host form of sfm_pair_fundamental: refined = 0 takes estimateE's E (transposed), 1 the refined E as it is
void mg_fundamental(const float *E, const float *Kinv, int refined, float *F) { guided_fundamental(E, Kinv, refined == 0, F); }

int mg_sizeof_params(void) { return (int)sizeof(sfm_match_guided_params); }

} // extern "C"
