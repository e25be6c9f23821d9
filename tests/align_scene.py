"""Inputs of the sfm_align_pair tests (helper, not a test): V >= 3 synthetic views of one point set, every pair (v, v + 1)
reconstructed in its own gauge (camera 1 = [I|0], |t| = 1) at the exact relative pose from observations with pixel noise, wrong
view-2 matches in a given share of every pair's records, the index that carries a record of pair v to the same feature's record
of pair v + 1 with a given share of wrong entries, the true links -- and the wrappers around the host build
(tests/hostcheck/libaligncheck.so).

Every view keeps its records in an order of its own (a permutation of the point set), so an index is a real look-up.  With the
relative pose X_{v+1} = Rrel_v X_v + trel_v and baselines b_v = |trel_v|, pair v's points are X_v / b_v and the link of pairs
(v, v + 1) is s = b_v / b_{v+1}, R = Rrel_v, t = trel_v / b_{v+1}: t / s is the unit translation of pair v's camera 2."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(1024, 61), (257, 7), (4096, 3)]           # (n, seed) of the checked inputs
WIDTH, HEIGHT, FOCAL = 720, 576, 2360.0
BASELINES = [1.0, 1.3, 0.8, 1.1, 0.9]                # |trel_v|: the gauges differ from pair to pair


def camera():
    K = np.array([[FOCAL, 0, WIDTH / 2.0], [0, FOCAL, HEIGHT / 2.0], [0, 0, 1]], np.float64).astype(np.float32)
    Kinv = np.array([[1.0 / FOCAL, 0, -(WIDTH / 2.0) / FOCAL], [0, 1.0 / FOCAL, -(HEIGHT / 2.0) / FOCAL], [0, 0, 1]], np.float64).astype(np.float32)
    return K, Kinv


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def relative_pose(v):
    """Camera v + 1 against camera v: about ten degrees around y, a few around x, the baseline mostly along x."""
    R = rot_y(np.deg2rad(10.0 - 1.5 * v)) @ rot_x(np.deg2rad(3.0 + v))
    d = np.array([1.0, 0.1 - 0.05 * v, 0.2])
    return R, BASELINES[v % len(BASELINES)] * d / np.linalg.norm(d)


def normalised(Kinv, u, v, ld):
    """3 x ld float32: K^-1 (u, v, 1) in float32, NaN behind the last record (the pair's X0 layout)."""
    n = len(u)
    X = np.full((3, ld), np.nan, np.float32)
    u = np.asarray(u, np.float32); v = np.asarray(v, np.float32)
    for r in range(3):
        X[r, :n] = (Kinv[r, 0] * u + Kinv[r, 1] * v).astype(np.float32) + Kinv[r, 2]
    return X


def triangulate(x1, x2, R, t):
    """DLT of normalised observations x1, x2 (n x 2) under [I|0] and [R|t], fp64: n x 3 points in the camera-1 frame and whether
    each lies in front of both cameras."""
    n = len(x1)
    P2 = np.hstack([R, t[:, None]])
    A = np.empty((n, 4, 4))
    A[:, 0] = np.array([1.0, 0, 0, 0]) * 1.0; A[:, 0, 2] = -x1[:, 0]
    A[:, 1] = np.array([0, 1.0, 0, 0]) * 1.0; A[:, 1, 2] = -x1[:, 1]
    A[:, 2] = P2[0][None] - x2[:, 0:1] * P2[2][None]
    A[:, 3] = P2[1][None] - x2[:, 1:2] * P2[2][None]
    _, _, Vt = np.linalg.svd(A)
    Xh = Vt[:, 3]
    X = Xh[:, :3] / Xh[:, 3:]
    Y = X @ R.T + t
    return X, (X[:, 2] > 0) & (Y[:, 2] > 0) & np.isfinite(X).all(1)


def build(n, seed, views=4, noise_px=0.5, wrong_match=0.15, wrong_index=0.05):
    """`views` cameras, views - 1 pairs, views - 2 links.  Returns {"K", "Kinv", "pairs": [...], "links": [...]} and the views'
    noisy pixel positions, record orders and their inverses (uv, perm, inv).  pairs[v]: n, ld, sift (view v's records matched
    against view v + 1), X0 / X1 (3 x ld), points (4 x n float32, W = 1), valid (uint8), good (the view-2 match is right), R, t
    (the exact camera 2 in the pair's gauge).  links[v] (pair v -> pair v + 1): index (int32 n), index_ok, good (both matches
    and the index right), s, R, t."""
    import cuda_sfm_amd as S
    rng = np.random.default_rng(seed)
    K, Kinv = camera()
    K64 = K.astype(np.float64)
    P = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)     # view 0's frame
    Xv = [P]
    rel = []
    for v in range(views - 1):
        R, t = relative_pose(v)
        rel.append((R, t))
        Xv.append(Xv[-1] @ R.T + t)
    perm = [np.arange(n)] + [rng.permutation(n) for _ in range(views - 1)]  # record r of view v is point perm[v][r]
    inv = [np.argsort(p) for p in perm]
    uv = []
    for v in range(views):
        p = Xv[v] @ K64.T
        uv.append(p[:, :2] / p[:, 2:] + noise_px * rng.standard_normal((n, 2)))
    ld = (n + 127) // 128 * 128
    pairs = []
    for v in range(views - 1):
        R, t = rel[v]
        b = np.linalg.norm(t)
        u1 = uv[v][perm[v]]
        u2 = uv[v + 1][perm[v]]
        bad = rng.random(n) < wrong_match
        u2 = np.where(bad[:, None], rng.random((n, 2)) * [WIDTH, HEIGHT], u2)
        sift = np.zeros(n, S.SIFT_DTYPE)
        sift["xpos"], sift["ypos"] = u1[:, 0].astype(np.float32), u1[:, 1].astype(np.float32)
        sift["match_xpos"], sift["match_ypos"] = u2[:, 0].astype(np.float32), u2[:, 1].astype(np.float32)
        sift["match"] = inv[v + 1][perm[v]].astype(np.int32)
        sift["score"], sift["ambiguity"] = 0.95, 0.5
        X0 = normalised(Kinv, sift["xpos"], sift["ypos"], ld)
        X1 = normalised(Kinv, sift["match_xpos"], sift["match_ypos"], ld)
        X, front = triangulate(X0[:2, :n].T.astype(np.float64), X1[:2, :n].T.astype(np.float64), R, t / b)
        pts = np.ascontiguousarray(np.vstack([X.T, np.ones(n)]).astype(np.float32))
        pairs.append(dict(n=n, ld=ld, sift=sift, X0=X0, X1=X1, points=pts, valid=front.astype(np.uint8), good=~bad, R=R, t=t / b, baseline=b))
    links = []
    for v in range(views - 2):
        index = inv[v + 1][perm[v]].astype(np.int32)
        wrong = rng.random(n) < wrong_index
        index = np.where(wrong, rng.integers(0, n, n), index).astype(np.int32)
        ok = index == inv[v + 1][perm[v]]
        good = ok & pairs[v]["good"] & pairs[v + 1]["good"][np.clip(index, 0, n - 1)]
        R, t = rel[v]
        links.append(dict(index=index, index_ok=ok, good=good, s=pairs[v]["baseline"] / pairs[v + 1]["baseline"], R=R, t=t / pairs[v + 1]["baseline"]))
    return dict(K=K, Kinv=Kinv, pairs=pairs, links=links, uv=uv, perm=perm, inv=inv)


def candidates(A, B, index):
    """The gate in numpy: the records of A that are candidates (bool n)."""
    nb = B["n"]
    ok = (index >= 0) & (index < nb)
    k = np.clip(index, 0, nb - 1)

    def usable(P, v):
        with np.errstate(all="ignore"):
            return (v != 0) & np.isfinite(P).all(0) & (P[3] != 0) & (P[2] / P[3] > 0)
    return ok & usable(A["points"], A["valid"]) & usable(B["points"], B["valid"])[k]


def sim_errors(sim, link):
    """(relative error of s, rotation angle against R, |t - true t| / |true t|) of 13 floats against the link's truth."""
    import refine_reference as RR
    sim = np.asarray(sim, np.float64)
    return (abs(sim[0] - link["s"]) / link["s"], RR.rotation_angle(sim[1:10].reshape(3, 3), link["R"]),
            float(np.linalg.norm(sim[10:13] - link["t"]) / np.linalg.norm(link["t"])))


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libaligncheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.aln_run.restype = None
    h.aln_run.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 12
    return h


def run_host(HL, S, A, B, index, K=None, **kw):
    """The host build over pairs A, B (dicts with n, ld, points, valid, X0) with AlignParams fields kw: (sim 26, inlier, err,
    counts, report dict, candidate order)."""
    p = S.align_params(**kw)
    na, nb = A["n"], B["n"]
    f = lambda a: np.ascontiguousarray(a, np.float32)
    Ka = f(A.get("K", K)); Kb = f(B.get("K", K))
    keep = [f(A["points"]), None if A.get("valid") is None else np.ascontiguousarray(A["valid"], np.uint8), f(A["X0"]), Ka,
            f(B["points"]), None if B.get("valid") is None else np.ascontiguousarray(B["valid"], np.uint8), f(B["X0"]), Kb,
            np.ascontiguousarray(index, np.int32)]
    out = [np.empty(26, np.float32), np.empty(na, np.uint8), np.empty(na, np.float32), np.empty(p.num_hypotheses, np.int32)]
    order = np.empty(na, np.int32)
    rep = S.AlignReport()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    HL.aln_run(na, A["ld"], *[vp(a) for a in keep[:4]], nb, B["ld"], *[vp(a) for a in keep[4:]], C.cast(C.byref(p), C.c_void_p),
               *[vp(a) for a in out], C.cast(C.byref(rep), C.c_void_p), vp(order))
    return out[0], out[1], out[2], out[3], {f: getattr(rep, f) for f, _ in S.AlignReport._fields_}, order
