"""GPU: registering a further view (sfm_register_view, csrc/register.hip) -- every RANSAC count, the winner and its pose bit for
bit against the host build of the same arithmetic, ground truth from exact points, robustness, the LM against the numpy fp64
twin, the full chain on a synthetic three-view scene and on the dino frames 0, 1, 2, the call contracts, no side effects,
determinism and sfm_main's 11th argument."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import DINO_K, DINO_KINV, DINO_SIFT, make_pair, read_pnm_grey, to_dev
import register_reference as GR
import register_scene as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINO = os.path.join(ROOT, "tests", "golden", "dino")
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def HL():
    h = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libregistercheck.so"))
    h.rg_ransac.argtypes = [C.c_uint32, C.c_uint32, C.c_int, f32p, C.c_float, f32p, f32p, C.POINTER(C.c_int32), f32p]
    h.rg_ransac.restype = C.c_uint64
    return h


def cam_of(K):
    return (float(K[0, 0]), float(K[0, 1]), float(K[1, 1]))


def host_candidates(rec, points, valid, Kinv, min_score=0.85, max_ambiguity=0.95):
    """The gate in numpy: the candidates in point order, X / W and the observation as the device computes them (fp32; the
    observation through fill_xu's K^-1 u with Kinv's last row (0 0 1))."""
    P = np.asarray(points, np.float32)
    with np.errstate(all="ignore"):
        ok = (rec["match"] >= 0) & (rec["score"] > min_score) & (rec["ambiguity"] < max_ambiguity) & np.isfinite(P).all(0) \
            & (P[3] != 0) & (P[2] / P[3] > 0)
    if valid is not None:
        ok &= valid.astype(bool)
    idx = np.flatnonzero(ok)
    Xc = np.zeros((len(idx), 4), np.float32)
    for c in range(3):
        Xc[:, c] = P[c, idx] / P[3, idx]
    return idx, Xc


def host_ransac(HL, sc_K, Oc, Xc, H, seed=0x5EED5F3D, thr=4.0):
    m = len(Xc)
    counts = np.zeros(H, np.int32)
    poses = np.zeros(12 * H, np.float32)
    key = HL.rg_ransac(seed, H, m, np.array(cam_of(sc_K), np.float32).ctypes.data_as(f32p), thr,
                       np.ascontiguousarray(Xc, np.float32).ctypes.data_as(f32p), np.ascontiguousarray(Oc, np.float32).ctypes.data_as(f32p),
                       counts.ctypes.data_as(C.POINTER(C.c_int32)), poses.ctypes.data_as(f32p))
    return key, counts, poses.reshape(12, H)


def setup(gpu, n, seed=1, **kw):
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.0, outlier_frac=0.0)
    pair, d_sift = make_pair(S, gpu, sc)
    rec, truth = RS.third_view(sc, seed=seed, **kw)
    return sc, pair, rec, truth


def obs_on_device(gpu, sc, rec):
    """K^-1 (match_xpos, match_ypos, 1) exactly as the gate computes it: fillXU of a scratch pair over the same records
    (fill_xu_kernel's arithmetic) and the z = 1 division."""
    torch, dev, ctx = gpu
    q = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, len(rec))
    q.fillXU(to_dev(torch, dev, rec))
    X1 = q.get_XU(S.BUF_X1)
    q.close()
    return np.stack([X1[0] / X1[2], X1[1] / X1[2]], 1).astype(np.float32)


@pytest.mark.parametrize("m,H", [(5, 1), (5, 4096), (37, 4096), (1000, 4096), (1000, 65536), (4096, 4096), (4096, 1), (4096, 65536)])
def test_counts_winner_and_pose_equal_the_host_build(gpu, HL, m, H):
    torch, dev, _ = gpu
    sc, pair, rec, truth = setup(gpu, max(m, 64), seed=m, noise_px=0.5, outlier_frac=0.3)
    n = len(rec)
    rec["score"][m:] = 0.5                                 # exactly m candidates
    pts = RS.homogeneous(sc["points3d"])
    rep = pair.register_view(to_dev(torch, dev, rec), points=torch.from_numpy(pts).to(dev), num_hypotheses=H)
    idx, Xc = host_candidates(rec, pts, None, sc["Kinv"])
    assert len(idx) == m == rep["num_candidates"]
    Oc = obs_on_device(gpu, sc, rec)[idx]
    key, counts, poses = host_ransac(HL, sc["K"], Oc, Xc, H)
    got = pair.get_view_counts()
    assert got.shape == (H,) and np.array_equal(got, counts)
    cnt, hyp = S.unpack_key(key)
    assert rep["best_hypothesis"] == hyp and (rep["ransac_inliers"] == cnt or rep["status"] == S.REFINE_DEGENERATE)
    _, Pr = pair.get_view_pose()
    wp = poses[:, hyp]
    if wp.any():
        assert np.array_equal(Pr[:3, :3].ravel().view(np.uint32), wp[:9].view(np.uint32))
        assert np.array_equal(Pr[:3, 3].view(np.uint32), wp[9:].view(np.uint32))
    assert n >= m


def test_noise_free_exact_points_recover_the_pose(gpu):
    torch, dev, _ = gpu
    sc, pair, rec, truth = setup(gpu, 2048, seed=3)
    pts = RS.homogeneous(sc["points3d"])
    rep = pair.register_view(to_dev(torch, dev, rec), points=torch.from_numpy(pts).to(dev))
    assert rep["status"] in (S.REFINE_CONVERGED, S.REFINE_MAX_ITER) and rep["num_inliers"] == 2048
    P, _ = pair.get_view_pose()
    assert GR.rotation_angle(P[:3, :3].astype(np.float64), truth["R3"]) < 1e-4
    assert np.linalg.norm(P[:3, 3] - truth["t3"]) < 1e-4 * np.linalg.norm(truth["t3"])


def test_noisy_outliers_refined_pose_beats_ransac_and_mask(gpu):
    torch, dev, _ = gpu
    e_ransac, e_ref = [], []
    for seed in range(5):
        sc, pair, rec, truth = setup(gpu, 2048, seed=10 + seed, noise_px=0.5, outlier_frac=0.3)
        pts = RS.homogeneous(sc["points3d"])
        rep = pair.register_view(to_dev(torch, dev, rec), points=torch.from_numpy(pts).to(dev))
        P, Pr = pair.get_view_pose()
        e_ref.append(GR.rotation_angle(P[:3, :3].astype(np.float64), truth["R3"]))
        e_ransac.append(GR.rotation_angle(Pr[:3, :3].astype(np.float64), truth["R3"]))
        err, inl = pair.get_view_errors()
        out = truth["outlier"]
        assert inl[~out].mean() >= 0.95 and inl[out].mean() <= 0.01, (inl[~out].mean(), inl[out].mean())
        assert inl.sum() == rep["num_inliers"] and np.isfinite(err).all()
        assert rep["final_rms_px"] < rep["initial_rms_px"]
    assert np.mean(e_ref) < np.mean(e_ransac), (e_ref, e_ransac)


def test_lm_matches_the_numpy_twin(gpu):
    torch, dev, _ = gpu
    sc, pair, rec, truth = setup(gpu, 3000, seed=21, noise_px=0.7, outlier_frac=0.2)
    pts = RS.homogeneous(sc["points3d"])
    d_rec, d_pts = to_dev(torch, dev, rec), torch.from_numpy(pts).to(dev)
    rep = pair.register_view(d_rec, points=d_pts, max_iterations=30)
    P, Pr = pair.get_view_pose()
    idx, Xc = host_candidates(rec, pts, None, sc["Kinv"])
    Oc = obs_on_device(gpu, sc, rec)[idx]
    cam = cam_of(sc["K"])
    inl = np.array([GR.pixel_error(cam, Pr[:3, :3].astype(np.float64), Pr[:3, 3].astype(np.float64), Xc[k:k + 1, :3].astype(np.float64),
                                   Oc[k:k + 1].astype(np.float64))[0] < 4.0 for k in range(len(idx))])
    assert abs(int(inl.sum()) - rep["ransac_inliers"]) <= 2            # (fp64 error vs the fp32 division-free test at the border)
    ref = GR.refine_pose(cam, Pr[:3, :3], Pr[:3, 3], Xc[inl, :3], Oc[inl], max_iterations=30)
    assert abs(rep["final_rms_px"] - ref["final_rms_px"]) <= 1e-3 * ref["final_rms_px"]
    assert GR.rotation_angle(P[:3, :3].astype(np.float64), ref["R"]) <= 2e-5
    assert np.abs(P[:3, 3] - ref["t"]).max() <= 2e-5 * max(1.0, np.linalg.norm(ref["t"]))


def test_full_chain_three_view_scene(gpu):
    """fillXU -> estimateE -> refine -> register on the refined points: t3 in the pair's gauge (|t12| = 1 here)."""
    torch, dev, _ = gpu
    n = 4096
    sc = synth.two_view_scene(n, seed=5, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=5))
    pair.refine(max_iterations=20)
    rec, truth = RS.third_view(sc, seed=5, noise_px=0.5, outlier_frac=0.3)
    rep = pair.register_view(to_dev(torch, dev, rec))
    # the candidates are the points refine used (the inliers of estimateE's tight epipolar threshold); 30 % of them are
    # outliers in view 3
    assert rep["status"] in (S.REFINE_CONVERGED, S.REFINE_MAX_ITER) and rep["num_inliers"] > 0.6 * rep["num_candidates"] > 100
    P, _ = pair.get_view_pose()
    Pr2, _ = pair.get_refined_pose()
    scale = np.linalg.norm(sc["t"])                       # the true |t12| (1): the gauge's unit
    rot = GR.rotation_angle(P[:3, :3].astype(np.float64), truth["R3"])
    terr = np.linalg.norm(P[:3, 3] / scale - truth["t3"]) / np.linalg.norm(truth["t3"])
    rot2 = GR.rotation_angle(Pr2[:3, :3].astype(np.float64), sc["R"])
    print(f"three-view chain: rotation error {rot:.2e} rad (the pair's own {rot2:.2e}), t3 relative error {terr:.2e}, "
          f"inliers {rep['num_inliers']} of {rep['num_candidates']}")
    # The pose is in the pair's gauge, so it carries the pair's error: measured 1.1e-2 rad and 0.8 % here, where the pair's
    # rotation is 6.7e-3 rad off and its points 2.5 % too deep; from exact points the same records give 6.5e-5 rad.
    assert rot < 2e-2 and terr < 3e-2 and rot < 2.5 * rot2 + 1e-3


def dino_extract(gpu, k, max_pts=32768):
    torch, dev, ctx = gpu
    img = read_pnm_grey(os.path.join(DINO, f"dino_grey_{k:03d}.pgm"))
    h, w = img.shape
    pitch = (w + 127) // 128 * 128
    pad = np.zeros((h, pitch), np.float32); pad[:, :w] = img
    d = torch.zeros((max_pts, 576), dtype=torch.uint8, device=dev)
    n, _ = ctx.extract_sift(d, max_pts, torch.from_numpy(pad).to(dev), w, h, pitch, **DINO_SIFT)
    return d, n


def test_dino_frames_0_1_2(gpu, HL):
    torch, dev, ctx = gpu
    (d0, n0), (d1, n1), (d2, n2) = (dino_extract(gpu, k) for k in (0, 1, 2))
    ctx.match(d0, n0, d1, n1)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    pair.refine(max_iterations=20)
    ctx.match(d0, n0, d2, n2)
    rep = pair.register_view(d0)
    P, Pr = pair.get_view_pose()
    P2, _ = pair.get_refined_pose()
    ang = lambda R: np.degrees(np.arccos(np.clip((np.trace(R.astype(np.float64)) - 1) / 2, -1, 1)))
    C3 = -P[:3, :3].T.astype(np.float64) @ P[:3, 3]
    C2 = -P2[:3, :3].T.astype(np.float64) @ P2[:3, 3]
    ratio = ang(P[:3, :3]) / ang(P2[:3, :3])
    print(f"dino 0-1-2: {rep}, angle(R2) {ang(P2[:3, :3]):.3f} deg, angle(R3) {ang(P[:3, :3]):.3f} deg, ratio {ratio:.3f}, "
          f"|C2| {np.linalg.norm(C2):.4f}, |C3| {np.linalg.norm(C3):.4f}")
    assert rep["num_inliers"] > 50
    # count parity on the candidates the device gated (records and refined points read back)
    rec = d0.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)[:n0]
    pts = pair.get_refined_points()
    _, used = pair.get_reprojection_errors()
    idx, Xc = host_candidates(rec, pts, used, DINO_KINV)
    assert len(idx) == rep["num_candidates"]
    sc = {"K": DINO_K, "Kinv": DINO_KINV}
    Oc = obs_on_device(gpu, sc, rec)[idx]
    key, counts, _ = host_ransac(HL, DINO_K, Oc, Xc, 4096)
    assert np.array_equal(pair.get_view_counts(), counts) and S.unpack_key(key)[1] == rep["best_hypothesis"]
    # Turntable expectation for equal steps: ratio 2, |C3| = 2 cos 5 deg.  Measured 1.90 and 2.30: the pair's own
    # rotation is 3.4 deg, not the 10 deg step, so its gauge is not metric and |C3| inherits that; the band on |C3| is 20 %.
    assert abs(ratio - 2.0) < 0.2 and abs(np.linalg.norm(C3) / (2 * np.cos(np.radians(5))) - 1.0) < 0.2


def test_contracts_degenerate_and_side_effects(gpu):
    torch, dev, _ = gpu
    n = 1024
    sc = synth.two_view_scene(n, seed=51)
    pair, d_sift = make_pair(S, gpu, sc)
    rec, _ = RS.third_view(sc, seed=51, noise_px=0.5)
    d_rec = to_dev(torch, dev, rec)
    with pytest.raises(S.SfmError) as e:                 # no refined points yet
        pair.register_view(d_rec)
    assert e.value.code == S.E_STATE
    d_pts = torch.from_numpy(RS.homogeneous(sc["points3d"])).to(dev)
    bad = (dict(reserved=[0, 0, 1, 0]), dict(num_hypotheses=0), dict(num_hypotheses=(1 << 20) + 1), dict(threshold_px=0.0),
           dict(threshold_px=float("nan")), dict(max_iterations=-1), dict(max_iterations=201), dict(huber_px=-1.0),
           dict(min_rel_decrease=-1.0), dict(initial_lambda=float("inf")), dict(min_score=float("nan")))
    for kw in bad:
        with pytest.raises(S.SfmError) as e:
            pair.register_enqueue(d_rec, S.register_params(points=d_pts, **kw))
        assert e.value.code == S.E_INVALID, kw
    with pytest.raises(S.SfmError) as e:
        pair.register_enqueue(d_rec, S.register_params(valid=d_pts))    # d_valid without d_points
    assert e.value.code == S.E_INVALID
    for fn in (pair.get_register_report, pair.get_view_pose, pair.get_view_errors, pair.get_view_counts):
        with pytest.raises(S.SfmError) as e:
            fn()
        assert e.value.code == S.E_STATE
    # side effects: everything estimateE, the pose chain and refine produced stays, bit for bit; two calls give the same bits
    pair.estimateE(S.default_params(n, num_hypotheses=512))
    pair.pose_chain(S.POSE_CORRECT)
    pair.refine(max_iterations=10)
    snap = lambda: (pair.get_E(), pair.get_inlier_mask(), pair.get_points(), pair.get_result(), pair.get_refined_pose()[0],
                    pair.get_refined_points(), *pair.get_reprojection_errors())
    before = snap()
    outs = []
    for _ in range(2):
        rep = pair.register_view(d_rec)
        outs.append((rep, *pair.get_view_pose(), *pair.get_view_errors(), pair.get_view_counts()))
    for a, b in zip(before, snap()):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert pair.device_ptr(S.BUF_VIEW_POSE)[1] == 128 and pair.device_ptr(S.BUF_VIEW_COUNTS)[1] == 4 * 4096
    assert pair.device_ptr(S.BUF_VIEW_REPROJ)[1] == 5 * n
    # estimateE / refine after the registration leave it readable; fillXU makes it stale
    pair.estimateE(S.default_params(n, num_hypotheses=512))
    assert pair.get_register_report() == outs[0][0]
    pair.fillXU(d_sift)
    for which in (S.BUF_VIEW_POSE, S.BUF_VIEW_COUNTS, S.BUF_VIEW_REPROJ):
        assert pair.device_ptr(which) == (None, 0)
    with pytest.raises(S.SfmError) as e:
        pair.get_view_pose()
    assert e.value.code == S.E_STATE
    # degenerate: 3 candidates, then a winner with < 6 inliers
    rec3 = rec.copy(); rec3["score"][3:] = 0.0
    rep = pair.register_view(to_dev(torch, dev, rec3), points=d_pts)
    assert rep["status"] == S.REFINE_DEGENERATE and rep["num_candidates"] == 3 and rep["num_inliers"] == 0
    P, Pr = pair.get_view_pose()
    assert np.array_equal(P, np.eye(4, dtype=np.float32)) and np.array_equal(Pr, P)
    err, inl = pair.get_view_errors()
    assert not inl.any() and not np.isnan(err).any()
    rec5 = rec.copy(); rec5["score"][5:] = 0.0
    rng = np.random.default_rng(0)
    rec5["match_xpos"][:5] = rng.random(5) * 720; rec5["match_ypos"][:5] = rng.random(5) * 576
    rep = pair.register_view(to_dev(torch, dev, rec5), points=d_pts)
    assert rep["status"] == S.REFINE_DEGENERATE and rep["num_inliers"] == 0 and rep["iterations"] == 0
    P, Pr = pair.get_view_pose()
    assert np.isfinite(P).all() and np.array_equal(P, Pr)
    assert not pair.get_view_errors()[1].any()


def test_sfm_main_third_image(tmp_path):
    app = os.path.join(ROOT, "cuda-sfm_amd", "host", "sfm_main")
    frames = [os.path.join(DINO, f"dino_grey_00{k}.pgm") for k in (0, 1, 2)]
    defaults = ["", "0", "0", "1.0", "1.5", "2360"]
    ply = str(tmp_path / "cloud.ply")
    r = subprocess.run([app, frames[0], frames[1], ply, *defaults, "20", frames[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^view3: (\d+)/(\d+) inliers, rms ([0-9.]+) -> ([0-9.]+) px, \|C3\| ([0-9.]+)$", r.stdout, flags=re.M)
    assert m, r.stdout
    inl, cand, rms0, rms1, c3 = int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))
    assert 50 < inl <= cand and rms1 <= rms0 and 1.5 < c3 < 2.5
    r2 = subprocess.run([app, frames[0], frames[1], ply, *defaults, "20", ""], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "view3:" not in r2.stdout
