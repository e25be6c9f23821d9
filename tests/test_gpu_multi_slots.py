"""GPU: the two slots of a pair (per-shard buffers, key, capacity: csrc/common.hpp, ShardSlot) under the two-slot pipelined estimateE
of tests/test_gpu_multi.py -- each scoring launch is handed ONE slot and the stream it goes to, so a slot's capacity and key must never be
taken for the other's."""
import ctypes as C

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
from helpers import same_bits, make_pair
import oracle as O
from test_gpu_prefilter import check_all

pytestmark = pytest.mark.gpu


def ctx_stream(ctx):
    st = C.c_void_p()
    assert S._lib.sfm_ctx_get_stream(ctx._h, C.byref(st)) == 0
    return st.value


@pytest.mark.parametrize("n,kernel,burst,rules", [
    # (a) the fused kernel on slot 0, the split kernel on slot 1, and slot 1 larger than slot 0
    (1500, S.KERNEL_AUTO, ((300, S.KERNEL_FUSED), (20000, S.KERNEL_SPLIT)), None),
    # (b) the pre-filter's per-hypothesis form on slot 0, its per-tile form on slot 1 behind the cell table's event
    (1024, S.KERNEL_PREFILTER, ((16384, S.KERNEL_PREFILTER), (32768, S.KERNEL_PREFILTER)), (S.PREFILTER_PER_HYPOTHESIS, S.PREFILTER_PER_TILE)),
])
def test_each_slot_keeps_its_own_capacity_and_key(gpu, n, kernel, burst, rules):
    """A scoring launch is handed one of the pair's two slots (per-shard buffers, key, capacity) and its stream.  A fresh pair, two
    pipelined calls of different sizes -- slot 0 small, slot 1 large -- then a flush and a serial estimateE of the large size with
    another seed: slot 0 has to grow from the small size by its OWN capacity and reduce into its OWN key.  Capacity or key taken from
    the other slot shows as counts written out of a too-small buffer's range or a key left over from the burst: every count, the key,
    the winner, its E and mask against the oracle.  The context's stream is the caller's throughout."""
    torch, dev, ctx = gpu
    scene = synth.two_view_scene(n, seed=900 + n)
    pair, _ = make_pair(S, gpu, scene)
    stream = ctx_stream(ctx)
    for k, (H, family) in enumerate(burst):
        pair.estimateE_pipelined(S.default_params(n, num_hypotheses=H, seed=5 + k, kernel=kernel))
        launch = pair.last_launch()
        assert launch["kernel"] == family and (rules is None or launch["prefilter_rule"] == rules[k]), (k, launch)
        assert ctx_stream(ctx) == stream
    pair.flush()
    H = burst[1][0]
    # the burst's result is slot 1's (E, mask and best only: the plain getters describe no slot's counts after pipelined calls)
    _, _, X0, X1 = O.fill_xu(scene["sift"], scene["Kinv"])
    q = S.default_params(n, num_hypotheses=H, seed=6)
    key, _, oE = O.ransac_range(X0, X1, 0, H, q.threshold, q.jacobi_sweeps, seed=q.seed, want_E=True)
    ocnt, ohyp = O.unpack_key(key)
    assert pair.get_best() == (ohyp, ocnt) and same_bits(pair.get_E(), oE[ohyp].reshape(3, 3))
    assert np.array_equal(pair.get_inlier_mask(), O.count_inliers(oE[ohyp], X0, X1, q.threshold)[1])
    p = S.default_params(n, num_hypotheses=H, seed=77, kernel=kernel)
    pair.estimateE(p)
    assert pair.last_launch()["kernel"] == burst[1][1] and ctx_stream(ctx) == stream
    check_all(pair, scene, p, H, n)
