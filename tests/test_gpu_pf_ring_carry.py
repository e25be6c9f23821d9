"""The survivor ring of a paired pass carried from its first scan into its second (csrc/ransac_prefilter.hip, VAR = 0: an entry's tag
names the scan that wrote it) against round 11's drain between the scans (kPfVarPairDrain).  The lab-bench library forces either at
every size: reserved[1] = 19 carries, 21 drains; reserved[3] = 7 makes the first call after a fillXU run the per-tile rule.  Every
count, the key, the winner's E and mask against the oracle, through both, at two and three ragged tiles and at hypothesis counts that
give a second scan of 1, 32 and 33 rows, an even and an odd number of passes and a last pair with one scan; a shard that begins at
hypothesis 33; two calls followed by a pipelined burst on both slots.  The lab bench's probe says how many entries block 0's first
wavefront held when its second scans began: some with the carried ring, none with the drain."""
import numpy as np
import pytest

import oracle as O
from helpers import same_bits, make_pair
from test_gpu_prefilter import check_all
from test_gpu_pf_pairs import scene_of, want_of, params, lds_bytes, scan_flags, HMAX

pytestmark = pytest.mark.gpu

NS = [1100, 2100]                          # two and three ragged tiles
HS = [65, 96, 97, 128, 4096 + 33]          # second scan of 1, 32, 33, 32 rows; 3, 3, 4, 4 passes; 130 passes whose last pair has one scan of 1
CARRIED, DRAINED = (0, 19, 0, 7), (0, 21, 0, 7)      # reserved[]: paired passes with the ring carried / drained between the scans, per-tile rule on every call
assert max(HS) <= HMAX


def carried_entries(pair):
    """ring entries block 0's wavefront 0 held when a second scan began, summed over its pairs (include/sfm_amd_ab.h: ticks[6] >> 32)"""
    return int(pair.last_phases()[6]) >> 32


@pytest.mark.parametrize("reserved", [CARRIED, DRAINED], ids=["carried", "drained"])
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_counts_key_E_mask(gpu_ab, n, H, reserved):
    import cuda_sfm_amd_ab as A
    torch, dev, _ = gpu_ab
    pair, _ = make_pair(A, gpu_ab, scene_of(n))
    p = params(A, n, H, reserved)
    pair.estimateE(p)
    launch = pair.last_launch()
    assert launch["kernel"] == A.KERNEL_PREFILTER and launch["prefilter_rule"] == A.PREFILTER_PER_TILE
    assert launch["lds_bytes"] == lds_bytes(n, 64), launch
    check_all(pair, scene_of(n), p, H, n, want_of(n, p.seed, 0, H))
    if H == 4096 + 33:
        # scan-flagged hypotheses ("all pairs survive" rows: entries with many survivors, which straddle the boundary) in both lane halves
        flagged = np.flatnonzero(scan_flags(torch, dev, pair, H))
        low, high = flagged[flagged % 64 < 32], flagged[flagged % 64 >= 32]
        held = carried_entries(pair)
        print(f"n {n}: {flagged.size} scan-flagged hypotheses, {low.size} in a low lane half, {high.size} in a high one; {held} entries held at second scans")
        assert low.size > 0 and high.size > 0
        assert (held > 0) if reserved[1] == 19 else (held == 0)
    pair.close()


@pytest.mark.parametrize("reserved", [CARRIED, DRAINED], ids=["carried", "drained"])
def test_shard_that_begins_at_hypothesis_33(gpu_ab, reserved):
    import cuda_sfm_amd_ab as A
    torch, dev, _ = gpu_ab
    n, begin, count = 2100, 33, 4096 + 33
    pair, _ = make_pair(A, gpu_ab, scene_of(n))
    p = params(A, n, HMAX, reserved, hyp_begin=begin, hyp_count=count)
    key, counts, _, _ = want_of(n, p.seed, begin, count)
    out = torch.full((1,), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64, device=dev)
    pair.ransac_score(p, key_out=out)
    torch.cuda.synchronize()
    assert pair.last_launch()["prefilter_rule"] == A.PREFILTER_PER_TILE
    assert np.array_equal(pair.get_inlier_counts(count), counts)
    assert int(out.item()) == key == pair.get_key()
    pair.close()


@pytest.mark.parametrize("reserved", [(0, 19, 0, 0), (0, 21, 0, 0)], ids=["carried", "drained"])
def test_two_calls_then_a_pipelined_burst_on_both_slots(gpu_ab, reserved):
    """per-hypothesis operands on the first call after a fillXU, per-tile operands (the paired passes) from the second on, then pipelined
    calls alternating between the pair's two slots and streams (the last one's winner, E and mask stand for its counts)"""
    import cuda_sfm_amd_ab as A
    n, H = 4096, 4096 + 33
    pair, _ = make_pair(A, gpu_ab, scene_of(n))
    p = params(A, n, H, reserved)
    for form in (A.PREFILTER_PER_HYPOTHESIS, A.PREFILTER_PER_TILE):
        pair.estimateE(p)
        assert pair.last_launch()["prefilter_rule"] == form
        check_all(pair, scene_of(n), p, H, n, want_of(n, p.seed, 0, H))
    assert pair.last_launch()["lds_bytes"] == lds_bytes(n, 64)
    seeds = (21, 22, 23)
    for s in seeds:
        pair.estimateE_pipelined(params(A, n, H, reserved, seed=s))
    key, _, oE, omask = want_of(n, seeds[-1], 0, H)
    ocnt, ohyp = O.unpack_key(key)
    assert pair.get_best() == (ohyp, ocnt)
    assert same_bits(pair.get_E(), oE) and np.array_equal(pair.get_inlier_mask(), omask)
    pair.close()
