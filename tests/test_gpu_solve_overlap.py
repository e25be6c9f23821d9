"""Pipelined estimateE with the next call's lane-solve kernel resident NEXT TO the current call's scoring kernel.

The pre-filter scoring kernel leaves a solve wavefront's registers free on every SIMD (tests/test_register_budget.py), so in a burst of
sfm_estimate_E_pipelined calls the solve of call k + 1 -- which also clears call k + 1's keys and accumulators and writes its candidates
and records -- runs while call k is still scoring out of the other slot's buffers.  Results must not notice: every call of a burst is
compared with a serial estimateE of the same seed on a fresh pair.

Shapes: the smallest that take the path -- two tiles' blocks on the chip and both slots in use: 1100 matches (2 tiles of 576) x 65536
hypotheses, and a ragged 2100 matches (3 tiles of 704) x 43776 hypotheses, whose last pass of 32 is partial for a shard cut at an odd
place.  A burst starts straight after a fillXU, so call 0 runs the per-hypothesis form, call 1 builds the ordered copy of the
correspondences and runs the per-tile form, and calls 2..5 run the per-tile form on alternating slots.

What is compared: the winner and its count (the arg-max key's two halves), E bit for bit and the inlier mask after every call; the key
word itself after the calls of slot 0 (sfm_get_key reads the pair's own key buffer, which is slot 0's).  The per-hypothesis counts of a
pipelined slot are not readable through the library (sfm_get_inlier_counts describes serial calls only), so all counts are compared
where they are: a serial call on the pair the burst ran on, after the burst, against the fresh pair's.  No timing is asserted."""
import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
import oracle as O
from helpers import same_bits, make_pair

pytestmark = pytest.mark.gpu

BURST = 6
SCENES = {"two_tiles": (1100, 65536, 31), "ragged": (2100, 43776, 47)}       # matches, hypotheses, first seed


def shard_of(H, which):
    """(hyp_begin, hyp_count): the whole range, or its second half"""
    return (0, H) if which == "whole" else (H // 2, H - H // 2)


def params(n, H, seed, which):
    begin, count = shard_of(H, which)
    return S.default_params(n, num_hypotheses=H, seed=seed, kernel=S.KERNEL_PREFILTER, hyp_begin=begin, hyp_count=count)


@pytest.fixture(scope="module")
def scenes():
    return {name: synth.two_view_scene(n, seed=900 + n) for name, (n, _, _) in SCENES.items()}


@pytest.fixture(scope="module")
def serial(gpu, scenes):
    """(scene, shard, seed) -> what one serial estimateE on a pair fresh from fillXU returns; computed once, never modified"""
    want = {}
    for name, (n, H, s0) in SCENES.items():
        for which in ("whole", "second_half"):
            count = shard_of(H, which)[1]
            for seed in range(s0, s0 + BURST):
                pair, _ = make_pair(S, gpu, scenes[name])
                pair.estimateE(params(n, H, seed, which))
                assert pair.last_launch()["kernel"] == S.KERNEL_PREFILTER
                res = {"key": pair.get_key(), "best": pair.get_best(), "E": pair.get_E().copy(), "mask": pair.get_inlier_mask().copy(),
                       "counts": pair.get_inlier_counts(count).copy()}
                for a in (res["E"], res["mask"], res["counts"]):
                    a.setflags(write=False)
                assert O.unpack_key(res["key"])[::-1] == res["best"]
                want[name, which, seed] = res
    return want


@pytest.mark.parametrize("which", ["whole", "second_half"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_burst_equals_serial_calls(gpu, scenes, serial, name, which):
    n, H, s0 = SCENES[name]
    begin, count = shard_of(H, which)
    pair, _ = make_pair(S, gpu, scenes[name])                    # straight after fillXU
    for k in range(BURST):
        p = params(n, H, s0 + k, which)
        pair.estimateE_pipelined(p)                              # slot k % 2
        pair.flush()
        launch = pair.last_launch()
        assert launch["kernel"] == S.KERNEL_PREFILTER
        assert launch["prefilter_rule"] == (S.PREFILTER_PER_HYPOTHESIS if k == 0 else S.PREFILTER_PER_TILE), k
        want = serial[name, which, s0 + k]
        assert pair.get_best() == want["best"], (k, pair.get_best(), want["best"])
        assert begin <= pair.get_best()[0] < begin + count
        assert same_bits(pair.get_E(), want["E"]), k
        assert np.array_equal(pair.get_inlier_mask(), want["mask"]), k
        assert int(pair.get_inlier_mask().sum()) == want["best"][1]
        if k % 2 == 0:
            assert pair.get_key() == want["key"], k
    # all counts, where the library lets them be read: a serial call on the pair the burst has used both slots of
    last = s0 + BURST - 1
    pair.estimateE(params(n, H, last, which))
    want = serial[name, which, last]
    counts = pair.get_inlier_counts(count)
    bad = np.flatnonzero(counts != want["counts"])
    assert bad.size == 0, f"{bad.size} counts differ, first: {bad[:5]} {counts[bad[:5]]} {want['counts'][bad[:5]]}"
    assert pair.get_key() == want["key"] and same_bits(pair.get_E(), want["E"]) and np.array_equal(pair.get_inlier_mask(), want["mask"])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_unflushed_burst_equals_the_last_serial_call(gpu, scenes, serial, name):
    """The same burst without a flush between the calls -- the way the bench issues them, and the only way two calls are on the chip
    together: the solve of call k + 1 next to the scoring of call k.  Results are those of the last call."""
    n, H, s0 = SCENES[name]
    pair, _ = make_pair(S, gpu, scenes[name])
    for upto in (2, 3, BURST):                                   # ends on slot 1, 0, 1
        for k in range(upto):
            pair.estimateE_pipelined(params(n, H, s0 + k, "whole"))
        pair.flush()
        want = serial[name, "whole", s0 + upto - 1]
        assert pair.get_best() == want["best"], upto
        assert same_bits(pair.get_E(), want["E"]) and np.array_equal(pair.get_inlier_mask(), want["mask"]), upto
