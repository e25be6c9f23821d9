"""Inputs of the sfm_intersect_tracks tests (helper, not a test): a fused table and a camera table as the arrays the call reads, the
wrapper around the host build (tests/hostcheck/libintersectcheck.so), and two hand-built tables -- the table is the caller's data,
so neither needs a fusion: a ring of 130 pairs with tracks of 2 .. 131 views, and three pairs whose views share one centre."""
import ctypes as C
import functools
import os

import numpy as np

import align_scene as AS
import chain_adjust_scene as CS

ROOT = AS.ROOT
LENGTHS = (2, 3, 31, 32, 33, 63, 64, 65, 66, 128, 129, 131)       # views per track of hand_built(): 131 = k + 1
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libintersectcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.intersect_run.restype = None
    h.intersect_run.argtypes = [C.c_int] + [C.c_void_p] * 9
    h.intersect_check_linear.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    h.intersect_check_choose.argtypes = [C.c_int, C.c_float, C.c_int, C.c_float]
    h.intersect_layout.argtypes = [C.c_int, C.c_void_p]
    return h


def table_arrays(res, k, N, cams=None, points=None, skip=None):
    """A fused dict (cuda_sfm_amd.fuse_chain's) -> host arrays in the order of sfm_intersect_in behind `pairs` (cams, track_offset,
    obs_cam, obs_record, points, flags, counts, skip), padded to the lengths sfm_fuse_out has.  cams / points: an adjustment's, in
    place of the table's own; skip: one byte per track, or None."""
    root, own, off, ocam, orec, pts, flags, counts = CS.fused_arrays(dict(res, points=res["points"] if points is None else points), k, N)
    if cams is not None:
        own = np.ascontiguousarray(cams, np.float32).ravel()
    sk = None
    if skip is not None:
        sk = np.zeros(N, np.uint8); sk[:len(skip)] = skip
    return [own, off, ocam, orec, pts, flags, counts, sk]


def empty_outputs(N, fill=0):
    return [np.full(4 * N, fill, np.float32), np.full(N, fill, np.uint8), np.full(N, fill, np.float32), np.full(8, fill, np.int32)]


def results(S, outs, N, T):
    pts, flags, err, counts = outs
    return dict(points=pts.reshape(4, N)[:, :T].copy(), flags=flags[:T].copy(), err=err[:T].copy(),
                counts={name: int(counts[i]) for i, name in enumerate(S.INTERSECT_COUNTS)})


def run_host(HL, S, chain, arrays, **kw):
    """The host build over a chain's pairs and the arrays of table_arrays, IntersectParams fields kw: results' dict + `start` (per
    track 0 no eligible start, 1 from C, 2 from L, 3 copied through) + `raw` (the whole output arrays)."""
    p = S.intersect_params(**kw)
    pairs = chain["pairs"]
    k = len(pairs)
    N = sum(P["n"] for P in pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = dict(X0=[f32(P["X0"]) for P in pairs], X1=[f32(P["X1"]) for P in pairs], K=[f32(P.get("K", chain["K"])) for P in pairs])
    tables = {name: (C.c_void_p * k)(*[a.ctypes.data for a in arrs]) for name, arrs in keep.items()}
    n = np.array([P["n"] for P in pairs], np.int32); ld = np.array([P["ld"] for P in pairs], np.int32)
    outs = empty_outputs(N)
    starts = np.zeros(N, np.uint8)
    i = S.IntersectIn(None, *[a.ctypes.data if a is not None else None for a in arrays])
    o = S.IntersectOut(*[a.ctypes.data for a in outs])
    HL.intersect_run(k, vp(n), vp(ld), C.cast(tables["X0"], C.c_void_p), C.cast(tables["X1"], C.c_void_p), C.cast(tables["K"], C.c_void_p),
                     C.cast(C.byref(i), C.c_void_p), C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(o), C.c_void_p), vp(starts))
    T = int(arrays[6][0])
    return dict(results(S, outs, N, T), start=starts[:T].copy(), raw=outs)


def _look_at(c, target):
    z = (target - c) / np.linalg.norm(target - c)
    x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ c


def _table(k, n, views, tracks, points, seed):
    """Pairs and table of a ring of k pairs (pair p = views p, p + 1 mod k) over `views` [(R, t)] for `tracks` [(head pair, views,
    flag)] of the scene points `points`, every observation projected exactly (fp64, rounded to the record's fp32 pixels).  Pairs are
    padded with unused records to n each."""
    import cuda_sfm_amd as S
    rng = np.random.default_rng(seed)
    K, Kinv = AS.camera()
    K64 = K.astype(np.float64)
    pix = lambda v, X: (lambda Y: Y[:2] / Y[2])(K64 @ (views[v][0] @ X + views[v][1]))
    recs = [[] for _ in range(k)]                                  # per pair its records: (pixel in view p, pixel in view p + 1)
    off, ocam, orec = [0], [], []
    for (h, m, flag), X in zip(tracks, points):
        for j in range(m - 1):
            q = (h + j) % k
            ocam.append(2 * q); orec.append(len(recs[q]))
            recs[q].append((pix(q, X), pix((q + 1) % len(views), X)))
        ocam.append(2 * q + 1); orec.append(len(recs[q]) - 1)
        off.append(len(ocam))
    assert max(len(r) for r in recs) <= n, max(len(r) for r in recs)
    ld = (n + 127) // 128 * 128
    pairs = []
    for p in range(k):
        sift = np.zeros(n, S.SIFT_DTYPE)
        sift["xpos"], sift["ypos"] = rng.uniform(0, AS.WIDTH, n), rng.uniform(0, AS.HEIGHT, n)
        sift["match_xpos"], sift["match_ypos"] = rng.uniform(0, AS.WIDTH, n), rng.uniform(0, AS.HEIGHT, n)
        for r, (a, b) in enumerate(recs[p]):
            sift["xpos"][r], sift["ypos"][r] = a
            sift["match_xpos"][r], sift["match_ypos"][r] = b
        sift["score"], sift["ambiguity"] = 0.95, 0.5
        pairs.append(dict(n=n, ld=ld, sift=sift, X0=AS.normalised(Kinv, sift["xpos"], sift["ypos"], ld),
                          X1=AS.normalised(Kinv, sift["match_xpos"], sift["match_ypos"], ld), points=np.ones((4, n), np.float32),
                          valid=np.ones(n, np.uint8), pose=np.concatenate([np.eye(3).ravel(), [1.0, 0.0, 0.0]]).astype(np.float32)))
    cams = np.zeros((k, 2, 12), np.float32)
    for p in range(k):
        for s in (0, 1):
            R, t = views[(p + s) % len(views)] if len(views) == k else views[p + s]
            cams[p, s] = np.concatenate([R.ravel(), t])
    T = len(tracks)
    pts = np.ones((4, T), np.float32)
    pts[:3] = np.asarray(points).T
    table = dict(root=np.zeros(k, np.int32), cams=cams, track_offset=np.array(off, np.int32), obs_cam=np.array(ocam, np.int32),
                 obs_record=np.array(orec, np.int32), points=pts, flags=np.array([f for _, _, f in tracks], np.uint8), err=np.zeros(T, np.float32),
                 counts=dict(tracks=T, observations=len(ocam), refined=T, kept=0, segments=1, longest_track=max(m for _, m, _ in tracks)))
    return dict(K=K, Kinv=Kinv, pairs=pairs, links=[]), table


@functools.lru_cache(maxsize=None)
def hand_built(k=130, n=32, seed=11):
    """A ring of k views on a circle of radius 10 round a blob of points (view 0 is [I|0]; every view sees every point), pair p =
    views (p, p + 1 mod k), and tracks of LENGTHS views: per length one headed in pair 0, one in pair 17 and one in pair k - length / 2.
    A track whose list crosses the seam (its first pair larger than its last) is of the seam class, flag 3 or 4, the others carry
    1 or 2; the track of k + 1 views runs round the whole ring and is listed once, in the seam class.  Exact observations and
    cameras; the table's columns are the TRUE points.  Returns (chain, table, truth (T x 3), depth (T: the smallest depth over the
    track's views))."""
    rng = np.random.default_rng(seed)
    centre = np.array([0.0, 0.0, 10.0])
    views = []
    for v in range(k):
        a = 2.0 * np.pi * v / k
        c = centre + 10.0 * np.array([np.sin(a), 0.15 * np.sin(3.0 * a), -np.cos(a)])
        views.append(_look_at(c, centre) if v else (np.eye(3), np.zeros(3)))
    tracks = []
    for m in LENGTHS:
        for h in ((0,) if m == k + 1 else (0, 17, k - m // 2)):
            seam = h + m - 2 >= k or m == k + 1                     # the last pair lies behind the seam: first pair larger than last
            tracks.append((h, m, (3 if m % 3 else 4) if seam else (2 if m % 2 else 1)))
    tracks.sort(key=lambda x: x[0])
    P = rng.uniform(-1.0, 1.0, (len(tracks), 3)) + centre
    chain, table = _table(k, n, views, tracks, P, seed)
    depth = np.array([min((views[(h + j) % k][0] @ X + views[(h + j) % k][1])[2] for j in range(m)) for (h, m, _), X in zip(tracks, P)])
    return chain, table, P, depth


@functools.lru_cache(maxsize=None)
def shared_centre(n=16, seed=13):
    """Three pairs over four views that all sit at the origin and only turn (a chain: view v is camera slot (v, 0) or (v - 1, 1)),
    tracks of 2, 3 and 4 views of points at depth 10, projected exactly: every track's rays coincide, so its linear intersection is
    singular.  Returns (chain, table, truth)."""
    rng = np.random.default_rng(seed)
    views = [(AS.rot_y(np.deg2rad(2.0 * v)) @ AS.rot_x(np.deg2rad(-1.0 * v)), np.zeros(3)) for v in range(4)]
    tracks = [(0, 2, 1), (0, 3, 1), (0, 4, 2), (1, 2, 1), (1, 3, 2), (2, 2, 1)]
    P = np.stack([rng.uniform(-0.5, 0.5, len(tracks)), rng.uniform(-0.5, 0.5, len(tracks)), rng.uniform(9.0, 11.0, len(tracks))], 1)
    chain, table = _table(3, n, views, tracks, P, seed)
    return chain, table, P


def displaced(table, truth, depth, share, seed=5):
    """The table with every column moved off the truth by `share` of the track's depth in a random direction."""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, truth.shape)
    d *= (share * depth / np.linalg.norm(d, axis=1))[:, None]
    pts = table["points"].copy()
    pts[:3] = (truth + d).T
    return dict(table, points=pts)
