// tests/hostcheck/pairstatecheck.cpp -- TEST HARNESS ONLY.
// Drives the real sfm::PairState (cuda-sfm_amd/csrc/pair_state.hpp) from tests/test_pair_state_host.py.  Built by the plain host
// compiler: the header includes no HIP header.  Nothing in the product loads this library.
#include "../../cuda-sfm_amd/csrc/pair_state.hpp"

using namespace sfm;

extern "C" {

// io: have, unit_z, have_pts4, have_bound, key_clean, last_count.  Returns 0, or -1 for an unknown transition.
int ps_apply(int transition, int arg, uint32_t io[6])
{
    PairState s;
    s.have = io[0]; s.unit_z = io[1] != 0; s.have_pts4 = io[2] != 0; s.have_bound = io[3] != 0; s.key_clean = io[4] != 0; s.last_count = io[5];
    switch (transition) {
    case 0: s.reset(); break;
    case 1: s.points_filled(arg != 0); break;
    case 2: s.points_set(); break;
    case 3: s.E_finalized(); break;
    case 4: s.candidates_done(); break;
    case 5: s.pose_chosen(); break;
    case 6: s.triangulated(); break;
    case 7: s.chain_done(); break;
    case 8: s.refined(); break;
    case 9: s.view_registered(); break;
    case 10: s.view_dropped(); break;
    case 11: break;                         // a call that failed: no transition
    default: return -1;
    }
    io[0] = s.have; io[1] = s.unit_z; io[2] = s.have_pts4; io[3] = s.have_bound; io[4] = s.key_clean; io[5] = s.last_count;
    return 0;
}

uint32_t ps_fresh(void) { return PairState().have; }
int ps_has(uint32_t have, uint32_t stages) { PairState s; s.have = have; return s.has(stages) ? 1 : 0; }
uint32_t ps_missing(uint32_t have, uint32_t stages) { PairState s; s.have = have; return s.missing(stages); }
const char *ps_hint(uint32_t missing) { return pair_stage_hint(missing); }
uint32_t ps_stage(int k) { const uint32_t v[7] = { kPoints, kE, kP, kPose, kPoints3d, kRefined, kView }; return k >= 0 && k < 7 ? v[k] : 0; }

}
