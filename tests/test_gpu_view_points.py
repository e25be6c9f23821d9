"""GPU: sfm_triangulate_view / sfm_triangulate_views (csrc/view_points.hip) -- every output byte against the host build of the
same arithmetic (tests/hostcheck/libviewpointscheck.so), the full chain on the device against the fp64 twin with nothing in
the pair changed, the state contract, the batched call against the single call, the dino frames 0, 1, 2."""
import ctypes as C
import os

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import DINO_K, DINO_KINV, make_pair, to_dev
import register_scene as RS
import view_points_reference as VR
import view_points_scene as VS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0xA5


@pytest.fixture(scope="module")
def HL():
    return VS.host_lib()


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def device_scene(gpu, n, seed):
    """A pair that only has points (fillXU) and the scene of the issue over the pair's OWN normalised observations."""
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
    s = VS.finish(sc, rec, truth, pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1))
    return pair, d_sift, s


def run_device(gpu, pair, s, **kw):
    torch, dev, _ = gpu
    valid = None if s["valid"] is None else to_dev(torch, dev, s["valid"])
    return pair.triangulate_view(to_dev(torch, dev, s["rec"]), points=to_dev(torch, dev, s["points"]), valid=valid,
                                 poses=to_dev(torch, dev, s["poses"]), **kw)


@pytest.mark.parametrize("max_iterations", [0, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 257, 1024])
def test_every_byte_equals_the_host_build(gpu, HL, n, max_iterations):
    """Exact-camera overrides on a pair that only has points: one lane, a wave edge, a ragged last block with ld != n; then the
    same scene with an input column whose W is 0 and one that holds a NaN: those records come out new or rejected, never
    refined or kept."""
    pair, _, s = device_scene(gpu, n, 61 if n == 1024 else 7 + n)
    assert pair.ld != n or n % 128 == 0
    for variant in ("plain", "w0", "nan"):
        if variant != "plain":
            s["rec"]["score"][0] = 0.95                                   # record 0 is seen and flagged valid
            s["valid"][0] = 1
            s["points"][:, 0] = (0.1, -0.2, 5.0, 0.0) if variant == "w0" else (np.nan, -0.2, 5.0, 1.0)
        got = run_device(gpu, pair, s, max_iterations=max_iterations)
        want = VS.run_host(HL, S, s, max_iterations=max_iterations)
        for name, a, b in zip(("points", "flags", "err", "counts"), got, want):
            assert a.shape == b.shape and np.array_equal(u8(a), u8(b)), (variant, name, int((u8(a) != u8(b)).sum()))
        if variant != "plain":
            assert got[1][0] in (S.VP_NEW, S.VP_NEW_REJECTED), (variant, got[1][0])
    pair.close()


def read_buffers(pair, ctx):
    """Every SFM_BUF_* of the pair as bytes (None where the id answers (NULL, 0))."""
    L = S.lib()
    L.sfm_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    out = []
    for which in range(19):
        ptr, nbytes = pair.device_ptr(which)
        if not ptr:
            out.append(None)
            continue
        buf = np.empty(nbytes, np.uint8)
        assert L.sfm_copy_to_host(ctx._h, buf.ctypes.data_as(C.c_void_p), ptr, nbytes) == S.OK
        out.append(buf)
    return out


def getters(pair):
    scored = pair.device_ptr(S.BUF_COUNTS)[1] // 4          # hypotheses of the last scoring launch: what the two count getters fill
    return (pair.get_E(), pair.get_inlier_mask(), pair.get_points(), pair.get_result(), *pair.get_refined_pose(), pair.get_refined_points(),
            *pair.get_reprojection_errors(), *pair.get_view_pose(), *pair.get_view_errors(), pair.get_view_counts(), pair.get_pose_candidates(),
            pair.get_pose_inverses(), np.array([pair.get_pose_index()]), pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1),
            np.array(list(pair.get_refine_report().values()), np.float64), np.array(list(pair.get_register_report().values()), np.float64),
            np.array([pair.get_key()], np.uint64), np.array(pair.get_best(), np.int64), pair.get_inlier_counts(1024)[:scored], pair.get_E_candidates(1024)[:scored])


def band(ref, threshold_px=4.0, min_parallax_deg=1.0):
    with np.errstate(invalid="ignore"):
        return ref["seen"] & ((np.abs(ref["err"] - threshold_px) <= 0.1 * threshold_px) |
                              (np.abs(ref["parallax"] - min_parallax_deg) <= 0.1 * min_parallax_deg))


def chain(gpu, n, seed):
    """fillXU -> estimateE -> pose_chain(CORRECT) -> refine -> register on the device; the pair and the records of view 3."""
    torch, dev, _ = gpu
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=seed))
    pair.pose_chain(S.POSE_CORRECT)
    pair.refine(max_iterations=20)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
    d_rec = to_dev(torch, dev, rec)
    pair.register_view(d_rec)
    return sc, pair, d_sift, rec, d_rec


def twin_on_device_state(pair, sc, rec):
    """The fp64 twin over what the device holds: the pair's poses, refined points, used flags and observations."""
    P2, _ = pair.get_refined_pose()
    P3, _ = pair.get_view_pose()
    pts = pair.get_refined_points()
    _, used = pair.get_reprojection_errors()
    cam = lambda P: (P[:3, :3].astype(np.float64), P[:3, 3].astype(np.float64))
    ref = VR.view_points(sc["K"], sc["Kinv"], rec, pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1), pts, used, cam(P2), cam(P3))
    return ref, pts


def test_full_chain_reads_the_pair_and_changes_nothing(gpu):
    torch, dev, ctx = gpu
    sc, pair, d_sift, rec, d_rec = chain(gpu, 1024, 61)
    ref, pts_in = twin_on_device_state(pair, sc, rec)
    buffers, answers = read_buffers(pair, ctx), getters(pair)
    points, flags, err, counts = pair.triangulate_view(d_rec)
    again = pair.triangulate_view(d_rec)
    # the pair: every buffer and every getter as before
    for which, (a, b) in enumerate(zip(buffers, read_buffers(pair, ctx))):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    for a, b in zip(answers, getters(pair)):
        assert np.array_equal(u8(a), u8(b))
    for a, b in zip((points, flags, err, counts), again):
        assert np.array_equal(u8(a), u8(b))
    # classes against the twin, outside the 10 % bands
    ex = band(ref)
    seen = int(ref["seen"].sum())
    print(f"full chain: counts {counts[:5].tolist()}, twin {np.bincount(ref['flags'], minlength=5).tolist()}, {int(ex.sum())} of {seen} seen in a band, "
          f"{int((flags != ref['flags'])[~ex].sum())} class differences outside")
    assert np.array_equal(flags[~ex], ref["flags"][~ex])
    assert ex.sum() <= 0.01 * seen
    assert np.array_equal(counts[:5], np.bincount(flags, minlength=5)) and not counts[5:].any()
    assert counts[S.VP_NEW] > 0 and counts[S.VP_REFINED] > 0
    keep = (flags == S.VP_UNSEEN) | (flags == S.VP_KEPT) | (flags == S.VP_NEW_REJECTED)
    assert np.array_equal(u8(points[:, keep]), u8(pts_in[:, keep]))
    acc = ~keep
    assert (points[3, acc] == 1.0).all() and np.isfinite(points[:, acc]).all() and np.isposinf(err[flags == S.VP_UNSEEN]).all()
    pair.close()


def code_and_text(fn):
    with pytest.raises(S.SfmError) as e:
        fn()
    return e.value.code, str(e.value)


def test_state_contract(gpu):
    torch, dev, _ = gpu
    n = 257
    sc = synth.two_view_scene(n, seed=9, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    rec, truth = RS.third_view(sc, seed=9, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
    d_rec = to_dev(torch, dev, rec)
    s = VS.finish(sc, rec, truth, pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1))
    d_pts, d_valid, d_poses = (to_dev(torch, dev, s[k]) for k in ("points", "valid", "poses"))
    assert code_and_text(lambda: pair.triangulate_view(d_rec))[0] == S.E_STATE
    pair.estimateE(S.default_params(n, num_hypotheses=512, seed=9))
    code, text = code_and_text(lambda: pair.triangulate_view(d_rec))
    assert code == S.E_STATE and "no refinement" in text
    code, text = code_and_text(lambda: pair.triangulate_view(d_rec, poses=d_poses))          # its own points: still the refinement
    assert code == S.E_STATE and "no refinement" in text
    pair.refine(max_iterations=5)
    code, text = code_and_text(lambda: pair.triangulate_view(d_rec))
    assert code == S.E_STATE and "no registration" in text
    code, text = code_and_text(lambda: pair.triangulate_view(d_rec, points=d_pts, valid=d_valid))
    assert code == S.E_STATE and "no registration" in text
    pair.triangulate_view(d_rec, poses=d_poses)                                              # refined points, given cameras
    pair.register_view(d_rec)
    first = pair.triangulate_view(d_rec)
    pair.estimateE(S.default_params(n, num_hypotheses=512, seed=10))                         # a new E makes neither stale
    assert np.array_equal(u8(first[0]), u8(pair.triangulate_view(d_rec)[0]))
    pair.fillXU(d_sift)                                                                      # new points do
    code, text = code_and_text(lambda: pair.triangulate_view(d_rec))
    assert code == S.E_STATE and "no refinement" in text
    out = pair.triangulate_view(d_rec, points=d_pts, valid=d_valid, poses=d_poses)           # all three overrides: points are enough
    assert out[3][:5].sum() == n
    pair.close()


def filled(torch, dev, n):
    return (torch.full((4, n), float("nan"), dtype=torch.float32, device=dev), torch.full((n,), PATTERN, dtype=torch.uint8, device=dev),
            torch.full((n,), -7.0, dtype=torch.float32, device=dev), torch.full((8,), -1, dtype=torch.int32, device=dev))


# n = 8 stands where the issue lists n = 1: estimateE refuses fewer than 8 correspondences, so a pair of one point cannot reach the
# refinement and the registration the batched call needs (n = 1 runs through the overrides in the byte-parity test above).  A block
# with ONE live lane inside a batched launch is still run: the second block of the 257-point job.
@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_batched_call_equals_the_single_call(gpu, order):
    torch, dev, ctx = gpu
    sizes = [8, 64, 257, 1024, 300]
    if order == "reversed":
        sizes = sizes[::-1]
    made = [chain(gpu, n, 20 + n) for n in sizes]
    pairs = [m[1] for m in made]
    recs = [m[4] for m in made]
    single = [p.triangulate_view(r) for p, r in zip(pairs, recs)]
    outs = [filled(torch, dev, p.num_points) for p in pairs]
    S.triangulate_views_enqueue(pairs, recs, S.view_points_params(), outs)
    ctx.synchronize()
    for k, (want, got) in enumerate(zip(single, outs)):
        for name, a, b in zip(("points", "flags", "err", "counts"), want, got):
            assert np.array_equal(u8(a), u8(b.cpu().numpy())), (order, sizes[k], name)
    assert [tuple(u8(a).tobytes() for a in r) for r in S.triangulate_views(pairs, recs)] == [tuple(u8(a).tobytes() for a in r) for r in single]
    # one pair without its registration: SFM_E_STATE naming it, nothing written
    sc = synth.two_view_scene(64, seed=5, noise_px=0.5, outlier_frac=0.3)
    bare, _ = make_pair(S, gpu, sc)
    bare.estimateE(S.default_params(64, num_hypotheses=256, seed=5))
    bare.refine(max_iterations=5)
    outs = [filled(torch, dev, p.num_points) for p in pairs[:2] + [bare] + pairs[2:]]
    with pytest.raises(S.SfmError) as e:
        S.triangulate_views_enqueue(pairs[:2] + [bare] + pairs[2:], recs[:2] + [recs[1]] + recs[2:], S.view_points_params(), outs)
    assert e.value.code == S.E_STATE and "pairs[2]" in str(e.value) and "no registration" in str(e.value)
    ctx.synchronize()
    for pts, flags, err, counts in outs:
        assert torch.isnan(pts).all() and (flags == PATTERN).all() and (err == -7.0).all() and (counts == -1).all()
    for p in pairs + [bare]:
        p.close()


def test_dino_frames_0_1_2(gpu):
    torch, dev, ctx = gpu
    (d0, n0), (d1, n1), (d2, n2) = (VS.dino_extract(gpu, k) for k in (0, 1, 2))
    ctx.match(d0, n0, d1, n1)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    pair.refine(max_iterations=20)
    ctx.match(d0, n0, d2, n2)
    pair.register_view(d0)
    points, flags, err, counts = pair.triangulate_view(d0)
    print(f"dino 0-1-2: {n0} records, counts unseen {counts[0]}, new {counts[1]}, refined {counts[2]}, new rejected {counts[3]}, kept {counts[4]}")
    assert counts[S.VP_NEW] + counts[S.VP_REFINED] > 0 and counts[:5].sum() == n0
    # every accepted point passes the acceptance test in fp64, within the 10 % band
    rec = d0.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)[:n0]
    ref, _ = twin_on_device_state(pair, {"K": DINO_K, "Kinv": DINO_KINV}, rec)
    cam = lambda P: (P[:3, :3].astype(np.float64), P[:3, 3].astype(np.float64))
    P2, P3 = cam(pair.get_refined_pose()[0]), cam(pair.get_view_pose()[0])
    K = DINO_K.astype(np.float64)
    for cls, use2 in ((S.VP_NEW, False), (S.VP_REFINED, True)):
        m = flags == cls
        if not m.any():
            continue
        X = points[:3, m].T.astype(np.float64)
        e = VR.pixel_errors(K, P2, P3, use2, ref["obs"][m], X).max(1)
        assert (e < 4.0 * 1.1).all(), (cls, e.max())
        assert np.abs(e - err[m]).max() < 0.05
        if not use2:
            assert (VR.parallax_deg(X, P3) >= 0.9).all()
    pair.close()
