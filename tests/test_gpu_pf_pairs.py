"""Paired passes of the per-tile pre-filter rule (csrc/ransac_prefilter.hip, VAR = 0): a wavefront takes 64 hypotheses at a time, one
per lane, prepares their operands once and scans them in two halves.  The lab-bench library forces the paired passes at every size
(reserved[1] = 19) and the single passes they replace (reserved[1] = 20); reserved[3] = 7 makes the first call after a fillXU run the
per-tile rule.  Every count, the key, the winner's E and mask against the oracle, through both, at 2, 3 and 4 tiles (two of them
ragged) and at hypothesis counts that give an odd number of passes, a last pair with one scan, and a last scan with fewer or more than
32 hypotheses; a shard that does not begin at 0; two calls on the same points followed by a pipelined burst on both slots; and the
product library on both sides of the size from which its own rule pairs the passes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
import oracle as O
from helpers import same_bits, make_pair
from test_gpu_prefilter import check_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1100, 2100, 4096]                    # 2, 3 and 4 tiles; the first two ragged
HS = [33, 64, 65, 4096 + 31, 4096 + 32, 4096 + 33, 8192 + 63]
HMAX = max(HS)
THR = 1e-6
PAIRED, SINGLE = (0, 19, 0, 7), (0, 20, 0, 7)      # reserved[]: paired / single passes, summing epilogue, per-tile rule on every call
SCAN_FLAG = 1                              # prefilter_record.hpp: kPfTileFlagScan, word 0 of a hypothesis' 16-byte record


@functools.lru_cache(maxsize=None)
def scene_of(n):
    return synth.two_view_scene(n, seed=1100 + n)


@functools.lru_cache(maxsize=None)
def oracle_of(n, seed):
    sc = scene_of(n)
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    _, counts, oE = O.ransac_range_fast(X0, X1, 0, HMAX, np.float32(THR), 0, seed=seed, want_E=True)
    counts.setflags(write=False)
    return X0, X1, counts, oE


def want_of(n, seed, begin, count):
    """(key, counts, E, mask) of the shard [begin, begin + count): first maximum = highest count, lowest id."""
    X0, X1, counts, oE = oracle_of(n, seed)
    c = counts[begin:begin + count]
    h = begin + int(np.argmax(c))
    return O.pack_key(int(counts[h]), h), c, oE[h].reshape(3, 3), O.count_inliers(oE[h], X0, X1, np.float32(THR))[1]


def params(mod, n, H, reserved=None, seed=11, **kw):
    p = mod.default_params(n, num_hypotheses=H, seed=seed, kernel=mod.KERNEL_PREFILTER, threshold=THR, **kw)
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    return p


def lds_bytes(n, rows):
    """the scoring block's LDS for a pair of n points with `rows` hypotheses per wavefront table (prefilter_lds.hpp through the host check:
    its default is the paired passes' 64 rows; 32 rows take 16 x 32 x 44 bytes less)"""
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpfldscheck.so"))
    ld = (n + 127) // 128 * 128
    full = lib.pfcheck_lds_bytes(lib.pfcheck_tile_points(ld))
    return full if rows == 64 else full - 16 * 32 * 44


class _DeviceBytes:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def scan_flags(torch, dev, pair, count):
    """the scan flag of every hypothesis of the last per-tile launch (lab bench: SFM_AB_BUF_PF_RECORDS, 16 bytes per hypothesis)"""
    ptr, nbytes = pair.device_ptr(100)
    assert ptr and nbytes >= 16 * count
    torch.cuda.synchronize()
    rec = torch.as_tensor(_DeviceBytes(ptr, nbytes), device=dev).cpu().numpy()[:16 * count].view(np.uint32).reshape(count, 4)
    return (rec[:, 0] & SCAN_FLAG) != 0


@pytest.mark.parametrize("reserved", [PAIRED, SINGLE], ids=["paired", "single"])
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
    assert launch["lds_bytes"] == lds_bytes(n, 64 if reserved[1] == 19 else 32), launch
    check_all(pair, scene_of(n), p, H, n, want_of(n, p.seed, 0, H))
    if H == HMAX:
        # the zero-divisor scan of a paired pass takes a lane's OWN flag: both halves of the lanes must have met one
        flagged = np.flatnonzero(scan_flags(torch, dev, pair, H))
        low, high = flagged[flagged % 64 < 32], flagged[flagged % 64 >= 32]
        print(f"n {n}: {flagged.size} scan-flagged hypotheses, {low.size} in a low lane half, {high.size} in a high one")
        assert low.size > 0 and high.size > 0
    pair.close()


@pytest.mark.parametrize("reserved", [PAIRED, SINGLE], ids=["paired", "single"])
def test_shard_that_does_not_begin_at_zero(gpu_ab, reserved):
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


@pytest.mark.parametrize("reserved", [(0, 19, 0, 0), (0, 20, 0, 0)], ids=["paired", "single"])
def test_two_calls_then_a_pipelined_burst_on_both_slots(gpu_ab, reserved):
    """The product's order of events: per-hypothesis operands on the first call after a fillXU, per-tile operands from the second on,
    then pipelined calls alternating between the pair's two slots and streams (the last one's winner, E and mask stand for its counts)."""
    import cuda_sfm_amd_ab as A
    n, H = 4096, 4096 + 33
    pair, _ = make_pair(A, gpu_ab, scene_of(n))
    p = params(A, n, H, reserved)
    for form in (A.PREFILTER_PER_HYPOTHESIS, A.PREFILTER_PER_TILE):
        pair.estimateE(p)
        assert pair.last_launch()["prefilter_rule"] == form
        check_all(pair, scene_of(n), p, H, n, want_of(n, p.seed, 0, H))
    assert pair.last_launch()["lds_bytes"] == lds_bytes(n, 64 if reserved[1] == 19 else 32)
    seeds = (21, 22, 23)
    for s in seeds:
        pair.estimateE_pipelined(params(A, n, H, reserved, seed=s))
    key, _, oE, omask = want_of(n, seeds[-1], 0, H)
    ocnt, ohyp = O.unpack_key(key)
    assert pair.get_best() == (ohyp, ocnt)
    assert same_bits(pair.get_E(), oE) and np.array_equal(pair.get_inlier_mask(), omask)
    pair.close()


@functools.lru_cache(maxsize=None)
def product_oracle():
    """1025 points, 2^21 hypotheses: computed once for both sides of the threshold"""
    sc = synth.two_view_scene(1025, seed=31)
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    _, counts, _ = O.ransac_range_fast(X0, X1, 0, 1 << 21, np.float32(THR), 0, seed=11)
    counts.setflags(write=False)
    return sc, counts


@pytest.mark.parametrize("H,paired", [((1 << 21) - 1, False), (1 << 21, True)])
def test_product_pairs_its_passes_from_its_own_size_on(gpu, H, paired):
    """1025 points (a row of 1152) are two tiles of 576: 2^21 hypotheses make 2^22 partial counts, the smallest launch whose passes the
    product pairs (prefilter_lds.hpp: pf_pairs_passes_at); one hypothesis fewer keeps the single passes.  The launch says which through
    its rule and the size of its block's LDS."""
    n = 1025
    sc, all_counts = product_oracle()
    ocounts = all_counts[:H]
    best = int(np.argmax(ocounts))
    key = O.pack_key(int(ocounts[best]), best)
    p = params(S, n, H)
    pair, _ = make_pair(S, gpu, sc)
    for form in (S.PREFILTER_PER_HYPOTHESIS, S.PREFILTER_PER_TILE):
        pair.estimateE(p)
        launch = pair.last_launch()
        assert launch["kernel"] == S.KERNEL_PREFILTER and launch["prefilter_rule"] == form
        counts = pair.get_inlier_counts(H)
        bad = np.flatnonzero(counts != ocounts)
        assert bad.size == 0, f"form {form}: {bad.size} counts differ, first: hyp {bad[:5]} gpu {counts[bad[:5]]} oracle {ocounts[bad[:5]]}"
        assert pair.get_key() == key
    assert launch["lds_bytes"] == lds_bytes(n, 64 if paired else 32), launch
    pair.close()
