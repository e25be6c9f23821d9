"""The tail of a scoring pass of the pre-filter kernel (csrc/ransac_prefilter.hip).  Large launches (2^21 partial counts on) sum
their counts into counts[] without waiting for an answer and get their keys from ransac_argmax_counts behind the launch; smaller
ones keep the returning atomic.  The lab-bench library runs the summing epilogue at every size (reserved[1] = 18) and keeps the two
parts that did not pay: the drain in which a lane works through several survivors of its ring entry, and the survivor decode
without its table.  Every count, the key, the winner's E and mask against the oracle, through both forms of the kernel (first and
second call after a fillXU), at sizes around the tile, the 64-entry flush and the 32-hypothesis pass, in the product and with the
summing epilogue forced; the paths the launcher treats differently (pipelined slots, a shard with a caller's key, caller-supplied
candidates whose pairs ALL survive) likewise; the product on both sides of its size threshold; and every lab-bench part switched
alone, which must give the product's results bit for bit."""
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
import oracle as O
from helpers import same_bits, to_dev, make_pair
from test_gpu_prefilter import check_all

pytestmark = pytest.mark.gpu

NS = [96, 1000, 1056, 3000, 4096]          # one short tile, a tile that is no multiple of 64, two, three and four tiles
HS = [33, 64, 65, 2049]                    # a partial last group of 32; one more pass than a block has wavefronts
HMAX = max(HS)


@functools.lru_cache(maxsize=None)
def scene_of(n):
    return synth.two_view_scene(n, seed=900 + n)


@functools.lru_cache(maxsize=None)
def oracle_of(n, thr, seed):
    """Counts and candidates of hypotheses 0 .. HMAX - 1, computed once per (points, threshold, seed): a call on the first H of them
    has the first H counts."""
    sc = scene_of(n)
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    _, counts, oE = O.ransac_range(X0, X1, 0, HMAX, np.float32(thr), 0, seed=seed, want_E=True)
    counts.setflags(write=False)
    return X0, X1, counts, oE


def want_of(n, thr, seed, begin, count):
    """(key, counts, E, mask) of the shard [begin, begin + count): first maximum = highest count, lowest id."""
    X0, X1, counts, oE = oracle_of(n, thr, seed)
    c = counts[begin:begin + count]
    h = begin + int(np.argmax(c))
    return O.pack_key(int(counts[h]), h), c, oE[h].reshape(3, 3), O.count_inliers(oE[h], X0, X1, np.float32(thr))[1]


def params(mod, n, H, thr, seed=11, **kw):
    return mod.default_params(n, num_hypotheses=H, seed=seed, kernel=mod.KERNEL_PREFILTER, threshold=thr, **kw)


def both_forms(mod, fixture, n, H, thr, reserved=None):
    """Two calls on a pair fresh from fillXU: per-hypothesis operands, then per-tile operands; each against the oracle."""
    pair, _ = make_pair(mod, fixture, scene_of(n))
    p = params(mod, n, H, thr)
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    want = want_of(n, thr, p.seed, 0, H)
    out = []
    for form in (mod.PREFILTER_PER_HYPOTHESIS, mod.PREFILTER_PER_TILE):
        pair.estimateE(p)
        assert pair.last_launch()["kernel"] == mod.KERNEL_PREFILTER and pair.last_launch()["prefilter_rule"] == form
        check_all(pair, scene_of(n), p, H, n, want)
        out.append((pair.get_inlier_counts(H).copy(), pair.get_key(), pair.get_E().copy(), pair.get_inlier_mask().copy()))
    pair.close()
    return out


SUM = (0, 18, 0, 0)                        # lab bench: the summing epilogue + ransac_argmax_counts at every size


def flavour(request, name):
    """("product" | "sum") -> (module, fixture, reserved)"""
    if name == "product":
        return S, request.getfixturevalue("gpu"), None
    import cuda_sfm_amd_ab as A
    return A, request.getfixturevalue("gpu_ab"), SUM


@pytest.mark.parametrize("which", ["product", "sum"])
@pytest.mark.parametrize("thr", [1e-8, 1e-6])
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_pass_tail_counts_key_E_mask(request, n, H, thr, which):
    mod, fx, reserved = flavour(request, which)
    both_forms(mod, fx, n, H, thr, reserved)


@pytest.mark.parametrize("H,sums", [((1 << 20) - 1, False), (1 << 20, True)])
def test_product_on_both_sides_of_the_size_threshold(gpu, H, sums):
    """1025 points (a row of 1152) are two tiles of 576: 2^20 hypotheses make 2^21 partial counts, the smallest launch that sums them;
    one hypothesis fewer keeps the returning atomic.  The product library does not say which epilogue ran -- both must give the
    oracle's counts and key; WHICH one the launcher picks for these two sizes, the headline and the other bench configurations is
    asserted on the launcher's own rule by tests/test_pf_decode.py::test_which_launches_sum_their_counts.  One call per form."""
    n, thr = 1025, 1e-6
    sc = synth.two_view_scene(n, seed=31)
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    p = params(S, n, H, thr)
    key, ocounts, _ = O.ransac_range_fast(X0, X1, 0, H, np.float32(thr), 0, seed=p.seed)
    pair, _ = make_pair(S, gpu, sc)
    for form in (S.PREFILTER_PER_HYPOTHESIS, S.PREFILTER_PER_TILE):
        pair.estimateE(p)
        assert pair.last_launch()["kernel"] == S.KERNEL_PREFILTER and pair.last_launch()["prefilter_rule"] == form
        counts = pair.get_inlier_counts(H)
        bad = np.flatnonzero(counts != ocounts)
        assert bad.size == 0, f"sums={sums} form {form}: {bad.size} counts differ, first: hyp {bad[:5]} gpu {counts[bad[:5]]} oracle {ocounts[bad[:5]]}"
        assert pair.get_key() == key
    pair.close()


@pytest.mark.parametrize("which", ["product", "sum"])
def test_pipelined_burst_of_three_from_a_fresh_pair(request, which):
    """Both slots and slot 1's first use: bursts of one, two and three pipelined calls, each from a fresh fillXU; the counts of a slot
    are not readable through the pair, so the last call's winner, E and mask stand for them (they come from ransac_argmax_counts' key)."""
    mod, fx, reserved = flavour(request, which)
    n, H, thr = 3000, HMAX, 1e-6
    seeds = (21, 22, 23)
    for upto in (3, 1, 2):                                           # (3 first: slot 1's buffers are created inside a burst)
        pair, d_sift = make_pair(mod, fx, scene_of(n))
        for k in range(upto):
            p = params(mod, n, H, thr, seed=seeds[k])
            for i, v in enumerate(reserved or ()):
                p.reserved[i] = v
            pair.estimateE_pipelined(p)
        key, _, oE, omask = want_of(n, thr, seeds[upto - 1], 0, H)
        ocnt, ohyp = O.unpack_key(key)
        assert pair.get_best() == (ohyp, ocnt), upto
        assert same_bits(pair.get_E(), oE) and np.array_equal(pair.get_inlier_mask(), omask), upto
        pair.close()


@pytest.mark.parametrize("which", ["product", "sum"])
@pytest.mark.parametrize("begin,count", [(0, 33), (33, 1000), (2000, 49)])
def test_shard_with_a_callers_key(request, begin, count, which):
    """hyp_begin / hyp_count through sfm_ransac_score_into: the shard's counts, its key in the pair AND in the caller's word (filled
    with garbage before), twice (per-hypothesis, then per-tile operands)."""
    mod, fx, reserved = flavour(request, which)
    torch, dev, ctx = fx
    n, thr = 3000, 1e-6
    pair, _ = make_pair(mod, fx, scene_of(n))
    p = params(mod, n, HMAX, thr, hyp_begin=begin, hyp_count=count)
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    key, counts, _, _ = want_of(n, thr, p.seed, begin, count)
    for _ in range(2):
        out = torch.full((1,), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64, device=dev)
        pair.ransac_score(p, key_out=out)
        torch.cuda.synchronize()
        assert pair.last_launch()["kernel"] == mod.KERNEL_PREFILTER
        assert np.array_equal(pair.get_inlier_counts(count), counts)
        assert int(out.item()) == key == pair.get_key()
    pair.close()


@pytest.mark.parametrize("which", ["product", "sum"])
@pytest.mark.parametrize("n", [1000, 4096])
def test_candidates_whose_pairs_all_survive(request, n, which):
    """sfm_ransac_score_candidates with matrices whose first and second rows are zero: the first divisor vanishes at every point, so
    every pair of every tile survives the matrix cores -- 32 survivors in every ring entry, the worst case of the drain's cap and of
    the ring.  The rest of the set are the oracle's solved candidates.  Counts from the oracle's count_inliers."""
    mod, fx, reserved = flavour(request, which)
    torch, dev, ctx = fx
    H, thr = 65, 1e-6
    X0, X1, _, oE = oracle_of(n, thr, 11)
    Es = np.ascontiguousarray(oE[:H]).reshape(H, 9).copy()
    rng = np.random.default_rng(n)
    zero_rows = [0, 1, 7, 31, 32, 40, 64]
    for h in zero_rows:
        Es[h, :6] = 0.0
        Es[h, 6:] = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
    Es[7, 6:] = 0.0                                                  # and the zero matrix
    with np.errstate(invalid="ignore", over="ignore"):
        ocounts = np.array([O.count_inliers(Es[h], X0[:, :n], X1[:, :n], np.float32(thr), want_mask=False)[0] for h in range(H)], np.int32)
    best = int(np.argmax(ocounts))
    pair, _ = make_pair(mod, fx, scene_of(n))
    d_E = to_dev(torch, dev, Es.reshape(-1))
    p = params(mod, n, H, thr)
    for i, v in enumerate(reserved or ()):
        p.reserved[i] = v
    for form in (mod.PREFILTER_PER_HYPOTHESIS, mod.PREFILTER_PER_TILE):
        pair.ransac_score_candidates(p, d_E)
        assert pair.last_launch()["kernel"] == mod.KERNEL_PREFILTER and pair.last_launch()["prefilter_rule"] == form
        counts = pair.get_inlier_counts(H)
        bad = np.flatnonzero(counts != ocounts)
        assert bad.size == 0, f"form {form}: {bad.size} counts differ, first: hyp {bad[:8]} gpu {counts[bad[:8]]} oracle {ocounts[bad[:8]]}"
        assert pair.get_key() == O.pack_key(int(ocounts[best]), best)
    pair.close()


# lab bench: reserved[3] = 8 + (1: the drain takes up to 3 further survivors per lane, 2: table-free decode, 4: the returning atomic
# and the keys inside the kernel at every size); reserved[1] = 18: the summing epilogue at every size, 16 / 17: with the drain
# taking 1 / 7 further survivors per lane (per-tile form)
SWITCHES = [(0, 0, 0, 9), (0, 0, 0, 10), (0, 0, 0, 12), (0, 0, 0, 13), (0, 0, 0, 14), (0, 0, 0, 11), (0, 0, 0, 15), (0, 18, 0, 9), (0, 18, 0, 10), (0, 18, 0, 11),
            (0, 16, 0, 0), (0, 17, 0, 0), SUM]


@pytest.mark.parametrize("reserved", SWITCHES)
@pytest.mark.parametrize("n,H", [(96, 33), (96, 64), (3000, 2049)])
def test_each_part_switched_alone_agrees_with_the_product(gpu, gpu_ab, n, H, reserved):
    import cuda_sfm_amd_ab as A
    thr = 1e-6
    prod = both_forms(S, gpu, n, H, thr)
    lab = both_forms(A, gpu_ab, n, H, thr, reserved)
    for (pc, pk, pE, pm), (lc, lk, lE, lm) in zip(prod, lab):
        assert np.array_equal(pc, lc) and pk == lk and same_bits(pE, lE) and np.array_equal(pm, lm)
