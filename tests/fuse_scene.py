"""Inputs of the sfm_fuse_chain tests (helper, not a test): the six-view scene of align_scene.build as a chain of five pairs and
four links, and the wrapper around the host build (tests/hostcheck/libfusecheck.so).

A chain is {"K", "pairs": [...], "links": [...]}.  pairs[i]: n, ld, points (4 x n float32), valid (uint8 n), X0 / X1 (3 x ld),
pose (12 float32: camera 2 as R row-major, then t).  links[i] (pair i -> pair i + 1): index (int32 n_i), sim (13 float32), inlier
(uint8 n_i), err (float32 n_i), status.  The default links are the scene's true links: inlier is the link's `good` flag within
align_scene.candidates, err a fixed small value."""
import ctypes as C
import os

import numpy as np

import align_scene as AS

ROOT = AS.ROOT
SCENES = [(257, 7), (1024, 61), (64, 5), (65, 5)]    # (n, seed) of the checked inputs, six views each
VIEWS = 6
ERR = 0.25                                           # the default d_err of an inlier (px)


def sim13(s, R, t):
    return np.concatenate([[s], np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()]).astype(np.float32)


def chain_from_scene(sc):
    """The scene's pairs and true links as a chain."""
    pairs = [dict(n=P["n"], ld=P["ld"], points=P["points"].copy(), valid=P["valid"].copy(), X0=P["X0"], X1=P["X1"],
                  pose=np.concatenate([P["R"].ravel(), P["t"]]).astype(np.float32), sift=P["sift"]) for P in sc["pairs"]]
    links = []
    for i, L in enumerate(sc["links"]):
        inl = (L["good"] & AS.candidates(sc["pairs"][i], sc["pairs"][i + 1], L["index"])).astype(np.uint8)
        links.append(dict(index=L["index"].copy(), sim=sim13(L["s"], L["R"], L["t"]), inlier=inl, err=np.full(len(inl), ERR, np.float32), status=0))
    return dict(K=sc["K"], Kinv=sc["Kinv"], pairs=pairs, links=links)


def build(n, seed, views=VIEWS, **kw):
    """(scene, chain) of align_scene.build(n, seed, views=6, **kw)."""
    sc = AS.build(n, seed, views=views, **kw)
    # the scene's point set in view 0's frame: the first three draws of its generator, checked against view 0's pixels
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)
    q = P @ sc["K"].astype(np.float64).T
    assert np.median(np.abs(q[:, :2] / q[:, 2:] - sc["uv"][0])) <= 4.0 * kw.get("noise_px", 0.5) + 1e-9
    sc["P"] = P
    return sc, chain_from_scene(sc)


def truncated(chain, sizes):
    """The chain with pair i cut to its first sizes[i] records (ld kept): indices that now point past the end stay as they are."""
    pairs, links = [], []
    for P, m in zip(chain["pairs"], sizes):
        pairs.append(dict(P, n=m, points=np.ascontiguousarray(P["points"][:, :m]), valid=P["valid"][:m].copy(), sift=P["sift"][:m]))
    for L, m in zip(chain["links"], sizes):
        links.append(dict(L, index=L["index"][:m].copy(), inlier=L["inlier"][:m].copy(), err=L["err"][:m].copy()))
    return dict(chain, pairs=pairs[:len(sizes)], links=links[:len(sizes) - 1])


def head(chain, k):
    """The first k pairs of the chain."""
    return dict(chain, pairs=chain["pairs"][:k], links=chain["links"][:k - 1])


def tiled(chain, times):
    """The chain repeated `times` times, the copies joined by a cut (a degenerate link with an out-of-range index)."""
    pairs, links = [], []
    for r in range(times):
        pairs += chain["pairs"]
        links += chain["links"]
        if r + 1 < times:
            n = chain["pairs"][-1]["n"]
            links.append(dict(index=np.full(n, -1, np.int32), sim=sim13(1.0, np.eye(3), np.zeros(3)), inlier=np.zeros(n, np.uint8),
                              err=np.full(n, ERR, np.float32), status=2))
    return dict(chain, pairs=pairs, links=links)


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libfusecheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.fuse_run.restype = None
    h.fuse_run.argtypes = [C.c_int] + [C.c_void_p] * 15
    h.fuse_layout.argtypes = [C.c_int, C.c_void_p]
    return h


def empty_outputs(k, N):
    """Host arrays in the order of sfm_fuse_out."""
    return [np.zeros(13 * k, np.float32), np.zeros(k, np.int32), np.zeros(24 * k, np.float32), np.zeros(N, np.int32), np.zeros(N + 1, np.int32),
            np.zeros(2 * N, np.int32), np.zeros(2 * N, np.int32), np.zeros(4 * N, np.float32), np.zeros(N, np.uint8), np.zeros(N, np.float32),
            np.zeros(8, np.int32)]


def results(outs, k, N):
    """Arrays in the order of sfm_fuse_out -> the dict cuda_sfm_amd.fuse_chain returns."""
    import cuda_sfm_amd as S
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = outs
    T, M = int(counts[0]), int(counts[1])
    return dict(frames=frames.reshape(k, 13), root=root, cams=cams.reshape(k, 2, 12), track=track, track_offset=off[:T + 1].copy(),
                obs_cam=ocam[:M].copy(), obs_record=orec[:M].copy(), points=pts.reshape(4, N)[:, :T].copy(), flags=flags[:T].copy(),
                err=err[:T].copy(), counts={name: int(counts[i]) for i, name in enumerate(S.FUSE_COUNTS)})


def run_host(HL, S, chain, **kw):
    """The host build over a chain with FuseParams fields kw: the dict cuda_sfm_amd.fuse_chain returns."""
    p = S.fuse_params(**kw)
    pairs, links = chain["pairs"], chain["links"]
    k = len(pairs)
    N = sum(P["n"] for P in pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = dict(points=[f32(P["points"]) for P in pairs], valid=[np.ascontiguousarray(P["valid"], np.uint8) for P in pairs],
                X0=[f32(P["X0"]) for P in pairs], X1=[f32(P["X1"]) for P in pairs], K=[f32(P.get("K", chain["K"])) for P in pairs],
                pose=[f32(P["pose"]) for P in pairs], index=[np.ascontiguousarray(L["index"], np.int32) for L in links],
                sim=[f32(L["sim"]) for L in links], inlier=[np.ascontiguousarray(L["inlier"], np.uint8) for L in links],
                err=[f32(L["err"]) for L in links])
    ptrs = lambda arrs: (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    tables = {name: ptrs(arrs) for name, arrs in keep.items()}
    n = np.array([P["n"] for P in pairs], np.int32); ld = np.array([P["ld"] for P in pairs], np.int32)
    status = np.array([L["status"] for L in links] + [0], np.int32)
    outs = empty_outputs(k, N)
    o = S.FuseOut(*[a.ctypes.data for a in outs])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    tp = lambda name: C.cast(tables[name], C.c_void_p)
    HL.fuse_run(k, vp(n), vp(ld), tp("points"), tp("valid"), tp("X0"), tp("X1"), tp("K"), tp("pose"), tp("index"), tp("sim"), tp("inlier"),
                tp("err"), vp(status), C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(o), C.c_void_p))
    return results(outs, k, N)


def truth_in_pair0(sc, chain, res):
    """The true position, in pair 0's frame, of the feature every track of the FIRST segment starts with (T x 3, nan for the
    tracks of later segments): pair 0's frame is view 0's frame divided by pair 0's baseline."""
    out = np.full((len(res["flags"]), 3), np.nan)
    for t in range(len(res["flags"])):
        o = res["track_offset"][t]
        pair, rec = res["obs_cam"][o] >> 1, res["obs_record"][o]
        if res["root"][pair] == 0:
            out[t] = sc["P"][sc["perm"][pair][rec]] / sc["pairs"][0]["baseline"]
    return out
