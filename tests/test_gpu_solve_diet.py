"""The lane-solve kernels (ransac_solve_lanes1_qr, ransac_solve_lanes1_qr_rec) after their addressing change: the sample's eight
correspondences gathered as eight 16-byte loads at 32-bit offsets, candidates / records / accumulators stored from the block's base.
Nothing they compute may differ: E of EVERY hypothesis is compared with the oracle bit for bit, and so are the per-hypothesis counts and
the arg-max key of the scoring launch that reads the kernel's candidates and records.  The records themselves (64 bytes per hypothesis
on the first call after a fillXU, 16 bytes from the second call on) are only readable in the lab-bench flavour of the library, which has
a second, stand-alone builder of the same records (reserved[3] = 3: pf_prep_kernel, its own addressing): the two must agree byte for byte.

Shapes: the smallest the issue names -- 8 points (every sample needs the redraw loop of the sampler) with 65 hypotheses (a partial
wavefront behind a full one), 9 and 100 points, 4096 points x 129 hypotheses (two full wavefronts and one lane; the bench's point
count), a scene of repeated and collinear points (zero and NaN branches of the square roots, degenerate E), and a shard that does
not start at hypothesis 0.  All of them are fillXU pairs (16-byte records); the scattered-word gather of generic-z points is the parent's
source again and is run by tests/test_gpu_ransac.py::test_set_points_generic_z.  Every case runs two calls on one pair: the first takes the per-hypothesis instance, the second the per-tile
instance wherever the pre-filter applies."""
import numpy as np
import pytest

import cuda_sfm_amd as S
import cuda_sfm_amd_ab as A
from cuda_sfm_amd import synth
import oracle as O
from helpers import same_bits, make_pair

pytestmark = pytest.mark.gpu

SEED = 23
#        name: (points, hypotheses of the whole range, hyp_begin, hyp_count, degenerate scene)
CASES = {
    "n8": (8, 65, 0, 65, False),
    "n9": (9, 65, 0, 65, False),
    "n100": (100, 129, 0, 129, False),
    "n4096": (4096, 129, 0, 129, False),
    "degenerate": (256, 129, 0, 129, True),
    "shard": (1000, 400, 143, 129, False),
}


def scene_of(name):
    n, _, _, _, degenerate = CASES[name]
    scene = synth.two_view_scene(n, seed=700 + n)
    if degenerate:
        s = scene["sift"]
        # three quarters of the points one and the same correspondence (about one sample in ten draws eight of them: a zero matrix, NaN
        # out of the square roots), the rest on one line in both images
        m = 3 * n // 4
        s["xpos"][:m] = 100.0; s["ypos"][:m] = 50.0; s["match_xpos"][:m] = 100.0; s["match_ypos"][:m] = 50.0
        k = np.arange(m, n, dtype=np.float32)
        s["xpos"][m:] = k; s["ypos"][m:] = 2.0 * k
        s["match_xpos"][m:] = k + 3.0; s["match_ypos"][m:] = 2.0 * k + 1.0
    return scene


@pytest.fixture(scope="module")
def reference():
    """name -> (scene, key, counts, E of every hypothesis of the shard) from the oracle; computed once, never modified"""
    ref = {}
    for name, (n, H, begin, count, _) in CASES.items():
        scene = scene_of(name)
        _, _, X0, X1 = O.fill_xu(scene["sift"], scene["Kinv"])
        thr = S.default_params(n).threshold
        key, counts, E = O.ransac_range(X0, X1, begin, count, thr, 0, seed=SEED, want_E=True)
        for a in (counts, E):
            a.setflags(write=False)
        if name == "degenerate":                  # the case is about non-finite candidates: some, not all
            bad = int((~np.isfinite(E).all(axis=1)).sum())
            assert 0 < bad < count, f"{bad} of {count} candidates of the degenerate scene are non-finite"
        ref[name] = (scene, key, counts, E)
    return ref


def params(M, name):
    n, H, begin, count, _ = CASES[name]
    return M.default_params(n, num_hypotheses=H, seed=SEED, kernel=M.KERNEL_PREFILTER, jacobi_sweeps=0, hyp_begin=begin, hyp_count=count)


@pytest.mark.parametrize("name", list(CASES))
def test_candidates_counts_and_key_are_the_oracles(gpu, reference, name):
    n, H, begin, count, _ = CASES[name]
    scene, key, counts, E = reference[name]
    pair, _ = make_pair(S, gpu, scene)
    for call in (0, 1):
        pair.estimateE(params(S, name))
        launch = pair.last_launch()
        print(name, "call", call, launch)
        if name == "n4096":                       # the bench's geometry: the first call writes 64-byte records, the second 16-byte ones
            assert launch["kernel"] == S.KERNEL_PREFILTER
            assert launch["prefilter_rule"] == (S.PREFILTER_PER_HYPOTHESIS, S.PREFILTER_PER_TILE)[call]
        assert same_bits(pair.get_E_candidates(count), E), f"call {call}: per-hypothesis E differs from the oracle"
        assert np.array_equal(pair.get_inlier_counts(count), counts), f"call {call}: counts differ from the oracle"
        assert pair.get_key() == key, f"call {call}: arg-max key differs from the oracle"


class _DeviceBytes:
    """a device buffer of the library as something torch can wrap without copying"""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def records(torch, dev, pair, count):
    """the records the last launch left, as bytes: 64 per hypothesis under the per-hypothesis rule, 16 under the per-tile rule"""
    ptr, nbytes = pair.device_ptr(100)            # SFM_AB_BUF_PF_RECORDS
    assert ptr and nbytes == 64 * count
    torch.cuda.synchronize()
    per = 16 if pair.last_launch()["prefilter_rule"] == A.PREFILTER_PER_TILE else 64
    return torch.as_tensor(_DeviceBytes(ptr, nbytes), device=dev).cpu().numpy()[:per * count].reshape(count, per).copy()


@pytest.mark.parametrize("name", list(CASES))
def test_records_equal_the_stand_alone_builders(gpu_ab, reference, name):
    torch, dev, ctx = gpu_ab
    n, H, begin, count, _ = CASES[name]
    scene, key, counts, E = reference[name]
    inline, _ = make_pair(A, gpu_ab, scene)
    alone, _ = make_pair(A, gpu_ab, scene)
    compared = 0
    for call in (0, 1):
        inline.estimateE(params(A, name))
        q = params(A, name)
        q.reserved[3] = 3                         # records from pf_prep_kernel instead of the lane-solve kernel
        alone.estimateE(q)
        li, la = inline.last_launch(), alone.last_launch()
        print(name, "call", call, li, la)
        assert li["kernel"] == la["kernel"] and li["prefilter_rule"] == la["prefilter_rule"]
        assert same_bits(inline.get_E_candidates(count), E) and same_bits(alone.get_E_candidates(count), E)
        assert np.array_equal(inline.get_inlier_counts(count), counts) and np.array_equal(alone.get_inlier_counts(count), counts)
        if li["kernel"] == A.KERNEL_PREFILTER:
            ri, ra = records(torch, dev, inline, count), records(torch, dev, alone, count)
            bad = np.flatnonzero((ri != ra).any(axis=1))
            assert bad.size == 0, f"call {call}: records of hypotheses {bad[:8].tolist()} differ between the two builders"
            compared += 1
    if name == "n4096":
        assert compared == 2                      # both record forms were compared where the bench runs
