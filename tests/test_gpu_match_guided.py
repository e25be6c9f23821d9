"""GPU: sfm_match_guided and sfm_pair_fundamental against the host build (tests/hostcheck/libmatchguidedcheck.so): all five match
fields bit for bit over the launch plan's configurations and splits, a band that gates nothing against sfm_match, degenerate
gates, the contract, and the whole chain plain match -> estimateE -> refine -> F -> guided match on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
import match_guided_scene as MS
from helpers import to_dev as _to_dev

pytestmark = pytest.mark.gpu

# (2155, 2170): many splits; (4600, 97): configuration (1,8); (11100, 97): where sfm_match takes (2,8) -- the guided call runs (1,8)
SHAPES = [(1, 1), (31, 33), (33, 31), (255, 64), (257, 65), (1024, 1025), (2155, 2170), (4600, 97), (11100, 97)]


def to_dev(torch, dev, arr):
    return _to_dev(torch, dev, np.array(arr, copy=True))          # (the scenes' arrays are shared and read-only)


def records(t, n):
    return t.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)[:n]


def run(gpu, s1, s2, F, band=4.0, **kw):
    """-> (sift1 after the call, sift2 after the call), as records"""
    torch, dev, ctx = gpu
    d1, d2 = to_dev(torch, dev, s1), to_dev(torch, dev, s2)
    dF = torch.from_numpy(np.ascontiguousarray(np.asarray(F, np.float32).reshape(9))).to(dev)
    S.match_guided(ctx, d1, len(s1), d2, len(s2), dF, band_px=band, **kw)
    torch.cuda.synchronize()
    return records(d1, len(s1)), records(d2, len(s2))


def assert_only_match_fields_moved(got, before):
    for f in before.dtype.names:
        if f not in MS.FIELDS:
            assert np.array_equal(got[f].view(np.uint32), before[f].view(np.uint32)), f


@functools.lru_cache(maxsize=None)
def host(n1, n2, seed, band):
    sc = MS.scene(n1, n2, seed)
    return MS.host_run(sc["sift1"], sc["sift2"], sc["F"], band)


# 1 ---- shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_equals_the_host_build(gpu, n1, n2):
    sc = MS.scene(n1, n2, 7)
    got, db = run(gpu, sc["sift1"], sc["sift2"], sc["F"], 4.0)
    want = host(n1, n2, 7, 4.0)
    assert (want["match"] >= 0).sum() >= min(n1, n2) // 2 or min(n1, n2) < 4         # the gate lets the true rows through
    for f in MS.FIELDS:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert_only_match_fields_moved(got, sc["sift1"])
    assert np.array_equal(db.view(np.uint8), sc["sift2"].view(np.uint8))              # every field of d_sift2


# 2 ---- a band that gates nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(1024, 1025), (2155, 2170)])
def test_huge_band_is_sfm_match(gpu, n1, n2):
    torch, dev, ctx = gpu
    sc = MS.scene(n1, n2, 7)
    got, _ = run(gpu, sc["sift1"], sc["sift2"], sc["F"], 1e6)
    ctx.set_quirks(0)
    ctx.set_match_kernel(S.MATCH_EXACT)
    try:
        d1, d2 = to_dev(torch, dev, sc["sift1"]), to_dev(torch, dev, sc["sift2"])
        ctx.match(d1, n1, d2, n2)
        torch.cuda.synchronize()
        assert ctx.last_match_kernel() == S.MATCH_EXACT
        plain = records(d1, n1)
        dF = torch.from_numpy(np.asarray(sc["F"], np.float32).reshape(9).copy()).to(dev)
        S.match_guided(ctx, d1, n1, d2, n2, dF, band_px=1e6)                              # (leaves last_match_kernel alone)
        assert ctx.last_match_kernel() == S.MATCH_EXACT
    finally:
        ctx.set_match_kernel(S.MATCH_AUTO)
    assert MS.fields_equal(got, plain)
    assert (got["match"] >= 0).all()


# 3 ---- degenerate gates -----------------------------------------------------------------------------------------------------------
def assert_no_match(rec):
    assert np.all(rec["match"] == -1)
    for f in ("score", "match_xpos", "match_ypos", "ambiguity"):
        assert np.all(rec[f].view(np.uint32) == 0), f


def test_degenerate_gates_match_nothing(gpu):
    sc = MS.scene(257, 65, 7)
    s1 = np.array(sc["sift1"], copy=True)
    s1["match"] = 5; s1["score"] = 0.5; s1["ambiguity"] = 0.5; s1["match_xpos"] = 1.0; s1["match_ypos"] = 2.0
    Fnan = np.array(sc["F"], np.float64); Fnan[1, 1] = np.nan
    Finf = np.array(sc["F"], np.float64); Finf[0, 0] = np.inf
    for F, band in ((np.zeros((3, 3)), 4.0), (Fnan, 4.0), (Finf, 4.0), (sc["F"], 1e-6)):
        got, _ = run(gpu, s1, sc["sift2"], F, band)
        assert_no_match(got)
        assert MS.fields_equal(got, MS.host_run(s1, sc["sift2"], F, band))


def test_nan_positions_neither_match_nor_are_matched(gpu):
    sc = MS.scene(1024, 1025, 7)
    s1, s2 = np.array(sc["sift1"], copy=True), np.array(sc["sift2"], copy=True)
    bad1, bad2 = [0, 31, 32, 500, 1023], [1, 64, 65, 700, 1024]
    s1["xpos"][bad1] = np.nan
    s2["xpos"][bad2] = np.nan
    got, _ = run(gpu, s1, s2, sc["F"], 4.0)
    assert_no_match(got[bad1])
    assert not np.isin(got["match"], bad2).any()
    want = MS.host_run(s1, s2, sc["F"], 4.0)
    assert MS.fields_equal(got, want)
    assert (got["match"] >= 0).sum() > 900


# 4 ---- repeatability and the contract --------------------------------------------------------------------------------------------------
def test_second_call_gives_the_same_bytes(gpu):
    torch, dev, ctx = gpu
    sc = MS.scene(2155, 2170, 7)
    d1, d2 = to_dev(torch, dev, sc["sift1"]), to_dev(torch, dev, sc["sift2"])
    dF = torch.from_numpy(np.asarray(sc["F"], np.float32).reshape(9).copy()).to(dev)
    S.match_guided(ctx, d1, 2155, d2, 2170, dF, band_px=4.0)
    first = d1.clone()
    S.match_guided(ctx, d1, 2155, d2, 2170, dF, band_px=4.0)
    torch.cuda.synchronize()
    assert torch.equal(first, d1)


def test_contract(gpu):
    torch, dev, ctx = gpu
    sc = MS.scene(255, 64, 7)
    canary = np.array(sc["sift1"], copy=True)
    canary["match"] = 123456; canary["score"] = -7.0; canary["ambiguity"] = -8.0; canary["match_xpos"] = -9.0; canary["match_ypos"] = -10.0
    d1, d2 = to_dev(torch, dev, canary), to_dev(torch, dev, sc["sift2"])
    before = d1.clone()
    dF = torch.from_numpy(np.asarray(sc["F"], np.float32).reshape(9).copy()).to(dev)
    L = S.lib()
    ok = S.match_guided_params()
    call = lambda ctx_h, a, n1, b, n2, f, p: L.sfm_match_guided(ctx_h, a, n1, b, n2, f, C.byref(p) if p is not None else None)
    p1, p2, pf = d1.data_ptr(), d2.data_ptr(), dF.data_ptr()
    refusals = [(None, p1, 255, p2, 64, pf, ok), (ctx._h, None, 255, p2, 64, pf, ok), (ctx._h, p1, 255, None, 64, pf, ok),
                (ctx._h, p1, 255, p2, 64, None, ok), (ctx._h, p1, 255, p2, 64, pf, None),
                (ctx._h, p1, -1, p2, 64, pf, ok), (ctx._h, p1, 255, p2, -1, pf, ok)]
    for band in (0.0, -1.0, float("nan"), float("inf")):
        refusals.append((ctx._h, p1, 255, p2, 64, pf, S.match_guided_params(band_px=band)))
    for k in range(4):
        r = [0, 0, 0, 0]; r[k] = 1
        refusals.append((ctx._h, p1, 255, p2, 64, pf, S.match_guided_params(reserved=r)))
    for args in refusals:
        assert call(*args) == S.E_INVALID, args[2:5]
    torch.cuda.synchronize()
    assert torch.equal(before, d1)
    with pytest.raises(S.SfmError) as e:
        S.match_guided(ctx, d1, 255, d2, 64, dF, band_px=-2.0)
    assert e.value.code == S.E_INVALID
    # zero sizes write nothing
    for n1, n2 in ((0, 64), (255, 0), (0, 0)):
        assert call(ctx._h, p1, n1, p2, n2, pf, ok) == S.OK
    torch.cuda.synchronize()
    assert torch.equal(before, d1)
    assert call(ctx._h, p1, 255, p2, 64, pf, ok) == S.OK
    torch.cuda.synchronize()
    assert not torch.equal(before, d1)


# 5 ---- sfm_pair_fundamental --------------------------------------------------------------------------------------------------------------
def test_pair_fundamental(gpu):
    torch, dev, ctx = gpu
    n = 1024
    sc = synth.two_view_scene(n)
    d_sift = to_dev(torch, dev, sc["sift"])
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    pair.fillXU(d_sift)
    dF = torch.full((9,), -3.0, dtype=torch.float32, device=dev)
    for refined in (False, True):
        with pytest.raises(S.SfmError) as e:
            pair.fundamental(refined=refined, out=dF)
        assert e.value.code == S.E_STATE
    pair.estimateE(S.default_params(n, num_hypotheses=2048))
    with pytest.raises(S.SfmError) as e:
        pair.fundamental(refined=True, out=dF)
    assert e.value.code == S.E_STATE
    assert S.lib().sfm_pair_fundamental(pair._h, 2, dF.data_ptr()) == S.E_INVALID
    assert S.lib().sfm_pair_fundamental(pair._h, 0, None) == S.E_INVALID
    assert S.lib().sfm_pair_fundamental(None, 0, dF.data_ptr()) == S.E_INVALID
    torch.cuda.synchronize()
    assert torch.all(dF == -3.0)
    E = pair.get_E()
    F0 = pair.fundamental(refined=False).cpu().numpy()
    assert np.array_equal(F0.view(np.uint32), MS.host_fundamental(E, sc["Kinv"], 0).view(np.uint32))
    pair.refine(max_iterations=20)
    E0, mask0, (P, Er), pts0 = pair.get_E(), pair.get_inlier_mask(), pair.get_refined_pose(), pair.get_refined_points()
    F1 = pair.fundamental(refined=True).cpu().numpy()
    F0b = pair.fundamental(refined=False).cpu().numpy()
    assert np.array_equal(F1.view(np.uint32), MS.host_fundamental(Er, sc["Kinv"], 1).view(np.uint32))
    assert np.array_equal(F0b.view(np.uint32), F0.view(np.uint32))
    # the pair's buffers stay as they were
    assert np.array_equal(pair.get_E(), E0) and np.array_equal(pair.get_inlier_mask(), mask0)
    assert np.array_equal(pair.get_refined_pose()[1], Er) and np.array_equal(pair.get_refined_points(), pts0)
    # the pair's OWN records satisfy u2^T F u1 = 0 under both forms.  The scene's inliers carry 0.5 px of noise per view: under the
    # refined F they lie within 2 px (four sigma) of their lines in the median, under the F of estimateE's eight-point winner within
    # a fifth of what the outliers (uniform over the image) lie from theirs -- and under the OTHER transposition of the same E the
    # inliers are as far out as outliers
    s = sc["sift"]
    u1 = np.stack([s["xpos"], s["ypos"], np.ones(n, np.float32)]).astype(np.float64)
    u2 = np.stack([s["match_xpos"], s["match_ypos"], np.ones(n, np.float32)]).astype(np.float64)
    inl = ~sc["outlier"]

    def distances(F):
        l = np.asarray(F, np.float64).reshape(3, 3) @ u1
        return np.abs(np.sum(u2 * l, 0)) / np.hypot(l[0], l[1])
    d0, d1 = distances(F0), distances(F1)
    w0, w1 = distances(MS.host_fundamental(E, sc["Kinv"], 1)), distances(MS.host_fundamental(Er, sc["Kinv"], 0))
    print(f"median distance of the scene's inliers to their epipolar lines: estimateE's F {np.median(d0[inl]):.3f} px, refined F {np.median(d1[inl]):.3f} px; "
          f"outliers {np.median(d0[~inl]):.1f} / {np.median(d1[~inl]):.1f} px; inliers under the other transposition {np.median(w0[inl]):.1f} / {np.median(w1[inl]):.1f} px")
    assert np.median(d1[inl]) < 2.0
    assert np.median(d0[inl]) < 0.2 * np.median(d0[~inl]) and np.median(d1[inl]) < 0.2 * np.median(d1[~inl])
    assert np.median(w0[inl]) > 5 * np.median(d0[inl]) and np.median(w1[inl]) > 5 * np.median(d1[inl])
    pair.close()


# 6 ---- the whole chain on the device -----------------------------------------------------------------------------------------------------
def test_chain_plain_estimate_refine_guided(gpu):
    torch, dev, ctx = gpu
    n = 1024
    sc = MS.scene(n, n, 61)
    d1, d2 = to_dev(torch, dev, sc["sift1"]), to_dev(torch, dev, sc["sift2"])
    ctx.match(d1, n, d2, n)
    torch.cuda.synchronize()
    plain = records(d1, n)
    pc, pw = MS.accepted(plain, sc["truth"])
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    pair.fillXU(d1)
    pair.estimateE(S.default_params(n, num_hypotheses=4096))
    rep = pair.refine(max_iterations=20)
    dF = pair.fundamental(refined=True)
    S.match_guided(ctx, d1, n, d2, n, dF, band_px=4.0)
    torch.cuda.synchronize()
    got = records(d1, n)
    F = dF.cpu().numpy()
    want = MS.host_run(plain, sc["sift2"], F, 4.0)
    assert MS.fields_equal(got, want)
    gc, gw = MS.accepted(got, sc["truth"])
    Ft = np.asarray(sc["F"], np.float64).reshape(9)
    Fd = F.astype(np.float64)
    cosine = abs(Ft @ Fd) / (np.linalg.norm(Ft) * np.linalg.norm(Fd))
    print(f"chain on the device, n = {n}: refinement used {rep['num_used']} points, rms {rep['final_rms_px']:.3f} px, |cos(F, true F)| {cosine:.6f}; "
          f"plain accepted {pc} correct / {pw} wrong, guided at 4 px {gc} correct / {gw} wrong")
    assert gc >= pc
    pair.close()
