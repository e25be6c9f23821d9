"""Inputs of the sfm_fuse_ring tests (helper, not a test): ring_scene.build(..., pairs="all") as a ring chain -- k pairs and k links
in fuse_scene's chain form, link k - 1 carrying pair k - 1 onto pair 0 -- and the wrapper around the host build
(tests/hostcheck/libfuseringcheck.so).

links[i] (pair i -> pair i + 1 mod k): index (int32 n), sim (the TRUE link, 13 float32), inlier = the index is the right one & both
records' own matches are good & align_scene.candidates, err drawn per record (uniform 0.05 .. 1 px from a generator of its own),
so that contests between proposers are decided by the key's error bits and not by the record number alone; status 0."""
import ctypes as C
import os

import numpy as np

import align_scene as AS
import fuse_scene as FS
import ring_scene as RS

ROOT = AS.ROOT
RINGS = [(3, 257, 7), (4, 257, 7), (6, 257, 7), (6, 1024, 61), (5, 65, 5), (36, 65, 3)]      # (k, n, seed) of the checked inputs
# seam_proposals, seam_ineligible, seam_tracks of the rule prototyped on these inputs
EXPECTED = {(3, 257, 7): (172, 141, 31), (4, 257, 7): (162, 110, 52), (6, 257, 7): (160, 74, 86), (6, 1024, 61): (686, 337, 349),
            (5, 65, 5): (43, 26, 17), (36, 65, 3): (44, 0, 44)}


def chain_from_ring(sc, seed):
    k = sc["k"]
    pairs = [dict(n=P["n"], ld=P["ld"], points=P["points"].copy(), valid=P["valid"].copy(), X0=P["X0"], X1=P["X1"], pose=P["pose"].copy(),
                  sift=P["sift"]) for P in (sc["pairs"][v] for v in range(k))]
    links = []
    for v in range(k):
        w = (v + 1) % k
        A, B = sc["pairs"][v], sc["pairs"][w]
        index = sc["index"][v]
        right = index == sc["inv"][w][sc["perm"][v]]
        inl = right & A["good"] & B["good"][np.clip(index, 0, B["n"] - 1)] & AS.candidates(A, B, index)
        err = np.random.default_rng([seed, v, 2]).uniform(0.05, 1.0, A["n"]).astype(np.float32)
        links.append(dict(index=index.copy(), sim=sc["sims"][v].copy(), inlier=inl.astype(np.uint8), err=err, status=0))
    return dict(K=sc["K"], Kinv=sc["Kinv"], pairs=pairs, links=links)


def build(k, n, seed, **kw):
    """(scene, ring chain) of ring_scene.build(k, n, seed, pairs="all", **kw)."""
    sc = RS.build(k, n, seed, pairs="all", **kw)
    return sc, chain_from_ring(sc, seed)


def open_chain(ring):
    """The ring's k pairs and first k - 1 links: what sfm_fuse_chain takes."""
    return dict(ring, links=ring["links"][:-1])


def truncated(ring, sizes):
    """The ring with pair i cut to its first sizes[i] records (ld kept): indices that now point past the end stay as they are."""
    pairs = [dict(P, n=m, points=np.ascontiguousarray(P["points"][:, :m]), valid=P["valid"][:m].copy(), sift=P["sift"][:m])
             for P, m in zip(ring["pairs"], sizes)]
    links = [dict(L, index=L["index"][:m].copy(), inlier=L["inlier"][:m].copy(), err=L["err"][:m].copy()) for L, m in zip(ring["links"], sizes)]
    return dict(ring, pairs=pairs, links=links)


def feature(sc, pair, rec):
    """The scene point that record `rec` of pair `pair` observes in its first view."""
    return int(sc["perm"][pair][rec])


def truth_in_pair0(sc, feat):
    """Scene points `feat` in pair 0's frame: view 0's frame divided by pair 0's baseline."""
    return (sc["P"][feat] - sc["C"][0]) @ sc["R"][0].T / sc["baseline"][0]


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libfuseringcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.fuse_ring_run.restype = None
    h.fuse_ring_run.argtypes = [C.c_int] + [C.c_void_p] * 16
    h.fuse_ring_layout.argtypes = [C.c_int, C.c_void_p]
    return h


def run_host(HL, S, ring, **kw):
    """The host build over a ring chain with fuse_ring_params' names kw: the dict cuda_sfm_amd.fuse_ring returns."""
    p = S.fuse_ring_params(**kw)
    pairs, links = ring["pairs"], ring["links"]
    k = len(pairs)
    assert len(links) == k
    N = sum(P["n"] for P in pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = dict(points=[f32(P["points"]) for P in pairs], valid=[np.ascontiguousarray(P["valid"], np.uint8) for P in pairs],
                X0=[f32(P["X0"]) for P in pairs], X1=[f32(P["X1"]) for P in pairs], K=[f32(P.get("K", ring["K"])) for P in pairs],
                pose=[f32(P["pose"]) for P in pairs], index=[np.ascontiguousarray(L["index"], np.int32) for L in links],
                sim=[f32(L["sim"]) for L in links], inlier=[np.ascontiguousarray(L["inlier"], np.uint8) for L in links],
                err=[f32(L["err"]) for L in links])
    tables = {name: (C.c_void_p * k)(*[a.ctypes.data for a in arrs]) for name, arrs in keep.items()}
    n = np.array([P["n"] for P in pairs], np.int32); ld = np.array([P["ld"] for P in pairs], np.int32)
    status = np.array([L["status"] for L in links], np.int32)
    outs = FS.empty_outputs(k, N)
    o = S.FuseOut(*[a.ctypes.data for a in outs])
    rep = S.FuseRingReport()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    tp = lambda name: C.cast(tables[name], C.c_void_p)
    HL.fuse_ring_run(k, vp(n), vp(ld), tp("points"), tp("valid"), tp("X0"), tp("X1"), tp("K"), tp("pose"), tp("index"), tp("sim"), tp("inlier"),
                     tp("err"), vp(status), C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(o), C.c_void_p), C.cast(C.byref(rep), C.c_void_p))
    out = FS.results(outs, k, N)
    out["report"] = {f: getattr(rep, f) for f, _ in S.FuseRingReport._fields_}
    out["raw"] = outs                                      # the whole arrays in the order of sfm_fuse_out, for byte comparisons
    return out
