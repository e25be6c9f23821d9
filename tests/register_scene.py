"""Synthetic third views for the registration tests: a camera over two_view_scene's points, its projections written into the
match fields of view 1's records (match / match_xpos / match_ypos / score / ambiguity), as sfm_match would leave them."""
import numpy as np


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


R3_DEFAULT = rot_y(np.deg2rad(20.0)) @ rot_x(np.deg2rad(6.0))
T3_DEFAULT = np.array([2.0, 0.2, 0.4]) / np.linalg.norm([1.0, 0.1, 0.2])    # twice the pair's baseline, same direction


def third_view(sc, seed=0, noise_px=0.0, outlier_frac=0.0, gated_frac=0.0, R3=R3_DEFAULT, t3=T3_DEFAULT, width=720, height=576):
    """View 1's records of scene sc re-matched against a third camera X3 = R3 X + t3: observations with noise (px), a fraction
    replaced by uniform image points (outliers), a fraction failing the score gate.  Returns (records, truth) where truth
    holds R3, t3, the outlier and gated flags and the exact pixel positions."""
    rng = np.random.default_rng(seed)
    K = sc["K"].astype(np.float64)
    X = np.asarray(sc["points3d"], np.float64)
    n = len(X)
    Y = X @ R3.T + t3
    p = Y @ K.T
    uv = p[:, :2] / p[:, 2:]
    obs = uv + noise_px * rng.standard_normal((n, 2))
    out = rng.random(n) < outlier_frac
    obs[out] = rng.random((int(out.sum()), 2)) * [width, height]
    gated = rng.random(n) < gated_frac
    rec = sc["sift"].copy()
    rec["match"] = np.arange(n, dtype=np.int32)
    rec["match_xpos"] = obs[:, 0].astype(np.float32)
    rec["match_ypos"] = obs[:, 1].astype(np.float32)
    rec["score"] = np.where(gated, 0.5, 0.95).astype(np.float32)
    rec["ambiguity"] = np.full(n, 0.5, np.float32)
    return rec, {"R3": R3, "t3": t3, "outlier": out, "gated": gated, "uv": uv}


def homogeneous(points3d):
    """4 x n float32 (X, Y, Z, 1) in the layout sfm_register_params.d_points takes."""
    X = np.asarray(points3d, np.float64)
    return np.ascontiguousarray(np.vstack([X.T, np.ones(len(X))]).astype(np.float32))
