// tests/hostcheck/lmcheck.hip -- TEST HARNESS ONLY, part of librefinecheck.so (built with refinecheck.hip).
// Compiles the LM control the one-block solvers share (LmControl in cuda-sfm_amd/csrc/refine_math.hpp) as HIP *host* code, so
// that tests/test_lm_control_host.py can replay iteration outcomes through it without a GPU.  Nothing in the product loads this
// library; it is not a CPU fallback.
#include "../../cuda-sfm_amd/csrc/refine_math.hpp"

using namespace sfm;

// Replays n iterations' outcomes through LmControl the way the two LM kernels drive it: failed[k] != 0 is "the solve failed",
// otherwise "the tentative state has cost nc[k] and squared sum nsq[k]".  dout: lambda, cost, sq; iout: iterations, accepted,
// status, events consumed.
extern "C" void rc_lm_replay(double lambda0, double cost0, double sq0, int degenerate, int max_iterations, double min_rel,
                             int n, const int *failed, const double *nc, const double *nsq, double dout[3], int iout[4])
{
    LmControl lm(lambda0, cost0, sq0, degenerate != 0);
    int k = 0;
    while (lm.running(max_iterations) && k < n) {
        const int e = k++;
        if (failed[e]) {
            if (!lm.solve_failed()) break;
            continue;
        }
        bool stop;
        lm.tentative(nc[e], nsq[e], min_rel, stop);
        if (stop) break;
    }
    dout[0] = lm.lambda; dout[1] = lm.cost; dout[2] = lm.sq;
    iout[0] = lm.iters; iout[1] = lm.accepted; iout[2] = lm.status; iout[3] = k;
}
