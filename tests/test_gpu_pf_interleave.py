"""The two scans of a paired pass interleaved over ONE walk of the tile (csrc/ransac_prefilter.hip, VAR = 0: every 32-point block's B
fragments are read from LDS once and meet the A fragments of hypotheses 0..31 and then those of 32..63) against round 12's two scans back
to back (kPfVarPairSeq).  The lab-bench library forces either at every size: reserved[1] = 19 interleaves, 22 scans back to back;
reserved[3] = 7 makes the first call after a fillXU run the per-tile rule.  Every count, the key, the winner's E and mask against the
oracle, through both, at two and three ragged tiles, at a point count whose tiles have an odd number of 32-point blocks (the walk's last
iteration multiplies a block of padding), and at hypothesis counts that give a second half of 1, 32 and 33 - 32 rows, a last unit with
one scan, and odd and even unit counts; a shard that begins at hypothesis 33; two calls followed by a pipelined burst on both slots."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from helpers import same_bits, make_pair
from test_gpu_prefilter import check_all
from test_gpu_pf_pairs import scene_of, want_of, params, lds_bytes, scan_flags, HMAX, ROOT

pytestmark = pytest.mark.gpu

# 1100 and 2100 points: two tiles of 576 and three of 736, 736, 704 points.  2900 points (a row of 2944): tiles of 992, 992 and 960 points,
# 31, 31 and 30 blocks of 32 -- the first two walk 16 iterations of two blocks whose last second block is padding only
# (test_the_odd_point_count_has_tiles_of_an_odd_number_of_blocks holds that to pfcheck_tile_points).
N_ODD = 2900
NS = [1100, 2100, N_ODD]
# units of 64 and the rows of their second half: 33 -> 1 unit, 1 row; 64 -> 1, 32; 65 -> 2, the last with one scan of 1; 96 -> 2, one scan of 32;
# 97 -> 2, 1 row; 128 -> 2, 32; 4096 + 33 -> 65 units, the last with a second half of 1 row
HS = [33, 64, 65, 96, 97, 128, 4096 + 33]
INTERLEAVED, BACK_TO_BACK = (0, 19, 0, 7), (0, 22, 0, 7)      # reserved[]: the pair's scans interleaved / back to back (ring carried), per-tile rule on every call
assert max(HS) <= HMAX


def test_the_odd_point_count_has_tiles_of_an_odd_number_of_blocks():
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpfldscheck.so"))
    ld = (N_ODD + 127) // 128 * 128
    tile = lib.pfcheck_tile_points(ld)
    assert tile % 32 == 0 and (tile // 32) % 2 == 1, tile
    assert ld - 2 * tile > 0 and ld - 2 * tile <= tile            # three tiles, the first two of `tile` points


@pytest.mark.parametrize("reserved", [INTERLEAVED, BACK_TO_BACK], ids=["interleaved", "back_to_back"])
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
        # scan-flagged hypotheses ("all pairs survive" rows) in both lane halves: those of the high half are the rows whose patch must land
        # in the second half's fragments
        flagged = np.flatnonzero(scan_flags(torch, dev, pair, H))
        low, high = flagged[flagged % 64 < 32], flagged[flagged % 64 >= 32]
        held = int(pair.last_phases()[6]) >> 32
        print(f"n {n}: {flagged.size} scan-flagged hypotheses, {low.size} in a low lane half, {high.size} in a high one; ticks[6] >> 32 = {held}")
        assert low.size > 0 and high.size > 0
    pair.close()


@pytest.mark.parametrize("reserved", [INTERLEAVED, BACK_TO_BACK], ids=["interleaved", "back_to_back"])
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


@pytest.mark.parametrize("reserved", [(0, 19, 0, 0), (0, 22, 0, 0)], ids=["interleaved", "back_to_back"])
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
