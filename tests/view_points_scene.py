"""Inputs of the sfm_triangulate_view tests: two_view_scene + third_view with the true cameras, the two-view points a pair would
hold (fp64 DLT of views 1 and 2, usable where the match in view 2 was right), and the wrappers around the host build
(tests/hostcheck/libviewpointscheck.so)."""
import ctypes as C
import os

import numpy as np

from cuda_sfm_amd_synth import synth
import register_scene as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(1024, 61), (257, 7), (4096, 3)]           # (n, seed) of the checked inputs
f32p = C.POINTER(C.c_float)


def normalised(Kinv, x, y, ld):
    """3 x ld float32 K^-1 (x, y, 1), the tail NaN as the pair keeps it."""
    n = len(x)
    out = np.full((3, ld), np.nan, np.float32)
    out[:, :n] = (Kinv.astype(np.float64) @ np.stack([x.astype(np.float64), y.astype(np.float64), np.ones(n)])).astype(np.float32)
    return out


def two_view_points(X0, X1, R, t):
    """fp64 SVD DLT of every correspondence under [I|0], [R|t]: n x 3."""
    n = X0.shape[1]
    M1 = np.hstack([np.eye(3), np.zeros((3, 1))]); M2 = np.hstack([R, t[:, None]])
    a = X0[:2].astype(np.float64) / X0[2]; b = X1[:2].astype(np.float64) / X1[2]
    A = np.stack([a[0, :, None] * M1[2] - M1[0], a[1, :, None] * M1[2] - M1[1], b[0, :, None] * M2[2] - M2[0], b[1, :, None] * M2[2] - M2[1]], 1)
    v = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(all="ignore"):
        return (v[:, :3] / v[:, 3:]).reshape(n, 3)


def build(n, seed, noise3=0.5, outlier3=0.3, gated3=0.1, **third):
    """The scene of the issue: two_view_scene(n, seed, 0.5 px, 30 % outliers), third_view(seed, ...), exact cameras."""
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=noise3, outlier_frac=outlier3, gated_frac=gated3, **third)
    ld = (n + 127) // 128 * 128
    X0 = normalised(sc["Kinv"], sc["sift"]["xpos"], sc["sift"]["ypos"], ld)
    X1 = normalised(sc["Kinv"], sc["sift"]["match_xpos"], sc["sift"]["match_ypos"], ld)
    return finish(sc, rec, truth, X0, X1)


def finish(sc, rec, truth, X0, X1):
    """Points, flags and poses for given normalised observations (3 x ld; the GPU tests pass the pair's own)."""
    n = len(rec)
    pts = np.ones((4, n), np.float32)
    pts[:3] = two_view_points(X0[:, :n], X1[:, :n], sc["R"], sc["t"]).T.astype(np.float32)
    valid = (~sc["outlier"]).astype(np.uint8)
    poses = np.concatenate([sc["R"].ravel(), sc["t"], truth["R3"].ravel(), truth["t3"]]).astype(np.float32)
    return {"sc": sc, "rec": rec, "truth": truth, "X0": X0, "X1": X1, "ld": X0.shape[1], "n": n, "points": pts, "valid": valid, "poses": poses,
            "P2": (poses[:9].reshape(3, 3).astype(np.float64), poses[9:12].astype(np.float64)),
            "P3": (poses[12:21].reshape(3, 3).astype(np.float64), poses[21:].astype(np.float64))}


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libviewpointscheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    return C.CDLL(path)


def run_host(HL, S, s, **kw):
    """The host build over scene s with ViewPointsParams fields kw: (points 4 x n, flags, err, counts)."""
    n = s["n"]
    p = S.view_points_params(**kw)
    rec = np.ascontiguousarray(s["rec"])
    X0 = np.ascontiguousarray(s["X0"], np.float32); X1 = np.ascontiguousarray(s["X1"], np.float32)
    K = np.ascontiguousarray(s["sc"]["K"], np.float32); Kinv = np.ascontiguousarray(s["sc"]["Kinv"], np.float32)
    pts = np.ascontiguousarray(s["points"], np.float32)
    valid = None if s["valid"] is None else np.ascontiguousarray(s["valid"], np.uint8)
    poses = np.ascontiguousarray(s["poses"], np.float32)
    out = np.empty((4, n), np.float32); flags = np.empty(n, np.uint8); err = np.empty(n, np.float32); counts = np.empty(8, np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    HL.vp_run.restype = None
    HL.vp_run.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 13
    HL.vp_run(n, s["ld"], vp(rec), vp(X0), vp(X1), vp(K), vp(Kinv), vp(pts), vp(valid), vp(poses), C.cast(C.byref(p), C.c_void_p),
              vp(out), vp(flags), vp(err), vp(counts))
    return out, flags, err, counts


def dino_extract(gpu, k, max_pts=32768):
    """The records of dino frame k on the device, as tests/test_gpu_register.py extracts them: (tensor, count)."""
    torch, dev, ctx = gpu
    from helpers import DINO_SIFT, read_pnm_grey
    img = read_pnm_grey(os.path.join(ROOT, "tests", "golden", "dino", f"dino_grey_{k:03d}.pgm"))
    h, w = img.shape
    pitch = (w + 127) // 128 * 128
    pad = np.zeros((h, pitch), np.float32); pad[:, :w] = img
    d = torch.zeros((max_pts, 576), dtype=torch.uint8, device=dev)
    n, _ = ctx.extract_sift(d, max_pts, torch.from_numpy(pad).to(dev), w, h, pitch, **DINO_SIFT)
    return d, n
