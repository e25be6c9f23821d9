"""Inputs of the sfm_match_guided tests (helper, not a test): two feature sets over the geometry of synth.two_view_scene whose
descriptors repeat, the true fundamental matrix, and the wrapper around the host build
(tests/hostcheck/libmatchguidedcheck.so).

scene(n1, n2, seed): m = max(n1, n2) scene points are projected into both views (synth.two_view_scene: 0.5 px of noise, no
outliers).  Feature i of view 1 is point i (i < n1); view 2 holds points 0 .. n2 - 1 in a seeded permuted order.  GROUP_SHARE of
the points (the first half) come in groups of GROUP consecutive points that share one base descriptor; every feature's
descriptor is its point's base descriptor plus NOISE of per-feature, per-view noise, clipped and normalised as
synth.descriptors does.  Over the whole other image a grouped feature has four near-equal candidates (the plain match's
ambiguity gate rejects it); the epipolar band leaves the one that fits the geometry."""
import ctypes as C
import functools
import os

import numpy as np

import cuda_sfm_amd as S
from cuda_sfm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = 4
GROUP_SHARE = 0.5
NOISE = 0.05
MIN_SCORE, MAX_AMBIGUITY = 0.85, 0.95          # the gates FindHomography, sfm_align_index_from_matches and the registration apply
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def _finish(d):
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d = np.minimum(d, 0.2)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def true_F(sc):
    """K^-T [t]x R K^-1 in fp64, unit Frobenius norm: u2^T F u1 = 0 for u1 in view 1 (xpos, ypos) and u2 in view 2."""
    K = sc["K"].astype(np.float64)
    t = sc["t"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ sc["R"] @ Ki
    return F / np.linalg.norm(F)


@functools.lru_cache(maxsize=None)
def scene(n1, n2, seed):
    """dict: sift1 (n1 records), sift2 (n2 records), F (3 x 3 fp64, unit norm), truth (int32[n1]: the row of sift2 that shows
    feature i's point, -1 if none), grouped (bool[n1])."""
    m = max(n1, n2)
    sc = synth.two_view_scene(m, seed=seed, noise_px=0.5, outlier_frac=0.0)
    ngrouped = int(m * GROUP_SHARE) // GROUP * GROUP
    base_of = np.arange(m)
    base_of[:ngrouped] = (np.arange(ngrouped) // GROUP) * GROUP               # the group's first point lends its descriptor
    base = np.abs(synth.normal(seed, m * 128, 70).reshape(m, 128))[base_of]
    d1 = _finish(np.abs(_finish(base) + NOISE * synth.normal(seed, m * 128, 71).reshape(m, 128)))
    d2 = _finish(np.abs(_finish(base) + NOISE * synth.normal(seed, m * 128, 72).reshape(m, 128)))
    perm = np.argsort(synth.splitmix64(seed, n2, 73), kind="stable")          # row j of view 2 shows point perm[j]
    s1 = np.zeros(n1, S.SIFT_DTYPE)
    s1["xpos"], s1["ypos"] = sc["sift"]["xpos"][:n1], sc["sift"]["ypos"][:n1]
    s1["data"] = d1[:n1].astype(np.float32)
    s1["match"] = -1
    s2 = np.zeros(n2, S.SIFT_DTYPE)
    s2["xpos"], s2["ypos"] = sc["sift"]["match_xpos"][perm], sc["sift"]["match_ypos"][perm]
    s2["data"] = d2[perm].astype(np.float32)
    s2["match"] = -1
    row_of = np.full(m, -1, np.int32)
    row_of[perm] = np.arange(n2, dtype=np.int32)
    for a in (s1, s2):
        a.flags.writeable = False
    return {"sift1": s1, "sift2": s2, "F": true_F(sc), "truth": row_of[:n1].copy(), "grouped": np.arange(n1) < ngrouped,
            "K": sc["K"], "Kinv": sc["Kinv"]}


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libmatchguidedcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.mg_run.restype = None
    h.mg_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int]
    for f in (h.mg_line, h.mg_line_t):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    h.mg_limit.restype = C.c_float; h.mg_limit.argtypes = [C.c_void_p, C.c_float]
    h.mg_residual.restype = C.c_float; h.mg_residual.argtypes = [C.c_void_p, C.c_float, C.c_float]
    h.mg_pass.argtypes = [C.c_float, C.c_float, C.c_float]
    h.mg_finite.argtypes = [C.c_void_p]
    h.mg_gate.argtypes = [C.c_void_p, C.c_float] + [C.c_float] * 4
    h.mg_fundamental.restype = None
    h.mg_fundamental.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return h


def host_run(sift1, sift2, F, band, gated=True):
    """The host build's sfm_match_guided (gated=False: its sfm_match) -> a copy of sift1 with the five match fields written."""
    out = np.array(sift1, copy=True)
    s2 = np.ascontiguousarray(sift2)
    f = np.ascontiguousarray(np.asarray(F, np.float32).reshape(9))
    if len(out) and len(s2):
        host_lib().mg_run(vp(out), len(out), vp(s2), len(s2), vp(f), C.c_float(band), 1 if gated else 0)
    return out


def host_fundamental(E, Kinv, refined):
    F = np.empty(9, np.float32)
    e = np.ascontiguousarray(np.asarray(E, np.float32).reshape(9)); k = np.ascontiguousarray(np.asarray(Kinv, np.float32).reshape(9))
    host_lib().mg_fundamental(vp(e), vp(k), 1 if refined else 0, vp(F))
    return F


FIELDS = ("score", "match", "match_xpos", "match_ypos", "ambiguity")


def fields_equal(a, b):
    """the five match fields, bit for bit"""
    return all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in FIELDS)


def accepted(rec, truth):
    """(correct, wrong): the records that pass MIN_SCORE / MAX_AMBIGUITY, by whether `match` is the true row"""
    ok = (rec["match"] >= 0) & (rec["score"] > MIN_SCORE) & (rec["ambiguity"] < MAX_AMBIGUITY)
    right = ok & (rec["match"] == truth) & (truth >= 0)
    return int(right.sum()), int((ok & ~right).sum())
