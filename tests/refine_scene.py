"""Inputs of the sfm_refine_two_view host-build tests (helper, not a test): the cases at the block edges of csrc/refine.hip -- the
start block of 64, the finish block of 256, the compaction rounds and strided sums of 512, the degenerate boundary of 16 used
points -- on the synthetic camera and on skewed ones, under two motions, and the wrapper around the host build of the whole call
(rc_run of tests/hostcheck/librefinecheck.so).

A case's E and inlier mask are estimateE's (on the CPU: the oracle's winner, which the GPU tests pin bit for bit).  Its mask is a
caller mask built from the host build's own used flags of a probe run (design), so that the used count is exact; the GPU tests run
design over the pair's own buffers."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from cuda_sfm_amd_synth import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPS = 256                                           # hypotheses of a case's estimateE

# name; n; seed; cam: None = synth.camera(), or (skew, fy / fx); motion: 0 = synth.two_view_scene's, 1 = MOTION1;
# mask: "inliers" = every true inlier the start uses, "own" = estimateE's mask (no caller mask), ("first", m) = the first m
# of "inliers", ("upto", j) = those of "inliers" at records <= j, "ones" = every record; kw: RefineParams fields;
# special: "" | "unused" (two records with NaN pixels, one triangulated behind the cameras) | "z" (sfm_set_points, z != 1)
Case = namedtuple("Case", "name n seed cam motion mask kw special", defaults=(None, 0, "inliers", {}, ""))
CASES = [
    Case("start63", 63, 11), Case("start64", 64, 12), Case("start65", 65, 13),
    Case("finish255", 255, 30, mask="own"), Case("finish256", 256, 30, mask="own"), Case("finish257", 257, 29, mask="own"),
    Case("finish255b", 255, 31, mask="own"),         # the scene whose start vote picks candidate 0
    Case("round511", 511, 31), Case("round512", 512, 32), Case("round513", 513, 33), Case("round1025", 1025, 34),
    Case("used0", 257, 41, mask=("first", 0)), Case("used15", 257, 41, mask=("first", 15)),
    Case("used16", 257, 41, mask=("first", 16)), Case("used17", 257, 41, mask=("first", 17)),
    Case("used511", 1025, 34, mask=("first", 511)), Case("used512", 1025, 34, mask=("first", 512)),
    Case("used513", 1025, 34, mask=("first", 513)),
    Case("last511", 1024, 53, mask=("upto", 511)), Case("last512", 1024, 53, mask=("upto", 512)),
    Case("unused", 257, 61, mask="ones", special="unused"),
    Case("unusedls", 257, 61, mask="ones", special="unused", kw=dict(huber_px=0.0)),     # plain least squares over the outliers
    Case("skew35", 257, 71, cam=(35.0, 0.93), motion=1, mask="own"),
    Case("skew-120", 513, 72, cam=(-120.0, 0.93), motion=1, mask="own"),
    Case("skew35m0", 257, 73, cam=(35.0, 0.93)),     # a poor E: the vote picks candidate 2, 90 of 177 true inliers are used
    Case("skew35m0b", 257, 77, cam=(35.0, 0.93)),    # every step accepted
    Case("iter0", 257, 29, mask="own", kw=dict(max_iterations=0)), Case("iter1", 257, 29, mask="own", kw=dict(max_iterations=1)),
    Case("iter20", 257, 29, mask="own", kw=dict(max_iterations=20)),
    Case("huber0", 257, 29, mask="own", kw=dict(huber_px=0.0)), Case("huber1", 257, 29, mask="own", kw=dict(huber_px=1.0)),
    Case("genericz", 257, 91, special="z"),
]
DEGENERATE = ("used0", "used15")
# the used count a row of the table states outright
EXACT = dict(used0=0, used15=15, used16=16, used17=17, used511=511, used512=512, used513=513)


def _rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    return {"y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]),
            "x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]])}[axis]


MOTION1 = (_rot("y", -8.0) @ _rot("z", 12.0), np.array([-0.2, 0.1, 1.0]) / np.linalg.norm([-0.2, 0.1, 1.0]))


def camera(skew, fy_ratio, width=720, height=576, focal=2360.0):
    """K with skew and fy != fx in float32, Kinv the fp64 inverse of that K rounded to float32."""
    K = np.array([[focal, skew, width / 2.0], [0, fy_ratio * focal, height / 2.0], [0, 0, 1]], np.float64).astype(np.float32)
    return K, np.linalg.inv(K.astype(np.float64)).astype(np.float32)


def two_view_variant(n, seed, K, Kinv, R, t, noise_px=0.5, outlier_frac=0.3, width=720, height=576):
    """synth.two_view_scene with the camera and the motion given: the same streams of the same generator."""
    u = lambda k: synth.uniform01(seed, n, k)
    g = lambda k: synth.normal(seed, n, k)
    K64 = K.astype(np.float64)
    P = np.stack([2 * u(1) - 1, 2 * u(2) - 1, 4 + 4 * u(3)], 1)
    p1 = P @ K64.T
    p2 = (P @ R.T + t) @ K64.T
    x1 = p1[:, :2] / p1[:, 2:] + noise_px * np.stack([g(4), g(5)], 1)
    x2 = p2[:, :2] / p2[:, 2:] + noise_px * np.stack([g(6), g(7)], 1)
    is_out = u(8) < outlier_frac
    x2 = np.where(is_out[:, None], np.stack([width * u(9), height * u(10)], 1), x2)
    sift = np.zeros(n, synth.SIFT_DTYPE)
    sift["xpos"], sift["ypos"] = x1[:, 0].astype(np.float32), x1[:, 1].astype(np.float32)
    sift["match_xpos"], sift["match_ypos"] = x2[:, 0].astype(np.float32), x2[:, 1].astype(np.float32)
    sift["match"] = np.arange(n, dtype=np.int32)
    return {"K": K, "Kinv": Kinv, "sift": sift, "R": R, "t": t, "points3d": P, "outlier": is_out}


UNUSED_NAN, UNUSED_BEHIND = (40, 200), 77            # the records the "unused" case spoils


def scene_of(case):
    """The case's scene; sc["valid"]: the records a mask of true inliers may hold; sc["zscale"]: the z of the "z" case's points."""
    if case.cam is None and case.motion == 0:
        sc = synth.two_view_scene(case.n, seed=case.seed, noise_px=0.5, outlier_frac=0.3)
    else:
        K, Kinv = synth.camera() if case.cam is None else camera(*case.cam)
        R, t = MOTION1 if case.motion == 1 else (synth._rot_y(np.deg2rad(10.0)) @ synth._rot_x(np.deg2rad(3.0)), np.array([1.0, 0.1, 0.2]) / np.linalg.norm([1.0, 0.1, 0.2]))
        sc = two_view_variant(case.n, case.seed, K, Kinv, R, t)
    sc["valid"] = ~sc["outlier"]
    if case.special == "unused":
        s = sc["sift"]
        s["xpos"][UNUSED_NAN[0]] = np.nan
        s["match_ypos"][UNUSED_NAN[1]] = np.nan
        # the match of one record moved past the image of its ray's point at infinity, against the parallax: the two rays
        # diverge and the DLT's point lies behind the cameras
        j = UNUSED_BEHIND
        K64 = sc["K"].astype(np.float64)
        X = sc["points3d"][j]
        far = K64 @ (sc["R"] @ X); far = far[:2] / far[2]
        near = K64 @ (sc["R"] @ X + sc["t"]); near = near[:2] / near[2]
        s["match_xpos"][j], s["match_ypos"][j] = (far - 2.0 * (near - far)).astype(np.float32)
        sc["valid"] = sc["valid"].copy()
        sc["valid"][[*UNUSED_NAN, UNUSED_BEHIND]] = False
    if case.special == "z":
        sc["zscale"] = (0.5 + 1.5 * synth.uniform01(case.seed, case.n, 70)).astype(np.float32), (0.5 + 1.5 * synth.uniform01(case.seed, case.n, 71)).astype(np.float32)
    return sc


def points_cpu(sc):
    """The pair's normalised points as fillXU computes them (oracle.fill_xu; 3 x n each); the "z" case's scaled to its z."""
    import oracle as O
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    if "zscale" in sc:
        X0, X1 = (X0 * sc["zscale"][0]).astype(np.float32), (X1 * sc["zscale"][1]).astype(np.float32)
    return np.ascontiguousarray(X0), np.ascontiguousarray(X1)


def estimate_cpu(case, X0, X1):
    """estimateE(default_params(n, num_hypotheses=HYPS, seed=case.seed)) on the CPU: (E 3 x 3, inlier mask)."""
    import oracle as O
    key, _, Ec = O.ransac_range(X0, X1, 0, HYPS, np.float32(1e-6), 0, seed=case.seed, want_E=True)
    _, hyp = O.unpack_key(key)
    E = Ec[hyp].reshape(3, 3).copy()
    return E, O.count_inliers(E, X0, X1, np.float32(1e-6))[1]


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "librefinecheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.rc_run.restype = None
    h.rc_run.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 12
    h.rc_sum512.restype = C.c_double
    h.rc_sum512.argtypes = [C.c_void_p]
    return h


def run_host(HL, S, X0, X1, E, K, mask, **kw):
    """The host build over 3 x n points, E, K and a mask (n) with RefineParams fields kw: a dict with pose (4 x 4), E (3 x 3),
    points (4 x n), err, used, report (dict) and trace (cur, failed solves, rejected steps, 0, votes 4)."""
    n = X0.shape[1]
    assert X0.shape == (3, n) and X1.shape == (3, n) and len(mask) == n
    p = S.refine_params(**kw)
    keep = [np.ascontiguousarray(X0, np.float32), np.ascontiguousarray(X1, np.float32), np.ascontiguousarray(E, np.float32).reshape(9),
            np.ascontiguousarray(K, np.float32).reshape(9), np.ascontiguousarray(mask, np.uint8)]
    pose = np.empty(25, np.float32); pts = np.empty((4, n), np.float32); err = np.empty(n, np.float32); used = np.empty(n, np.uint8)
    trace = np.zeros(8, np.int32)
    rep = S.RefineReport()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    HL.rc_run(n, n, *[vp(a) for a in keep], C.cast(C.byref(p), C.c_void_p), vp(pose), vp(pts), vp(err), vp(used),
              C.cast(C.byref(rep), C.c_void_p), vp(trace))
    return dict(pose=pose[:16].reshape(4, 4).copy(), E=pose[16:].reshape(3, 3).copy(), points=pts, err=err, used=used,
                report={f: getattr(rep, f) for f, _ in S.RefineReport._fields_}, trace=trace)


def design(HL, S, case, sc, X0, X1, E, inliers):
    """The case's mask over the given buffers: (mask uint8[n], caller: whether the call passes it -- False: estimateE's own)."""
    n = case.n
    if case.mask == "own":
        return np.ascontiguousarray(inliers, np.uint8), False
    if case.mask == "ones":
        return np.ones(n, np.uint8), True
    probe = run_host(HL, S, X0, X1, E, sc["K"], sc["valid"].astype(np.uint8), max_iterations=0)
    used = probe["used"].copy()
    if case.mask == "inliers":
        return used, True
    kind, arg = case.mask
    at = np.flatnonzero(used)
    mask = np.zeros(n, np.uint8)
    mask[at[:arg] if kind == "first" else at[at <= arg]] = 1
    return mask, True


def build_cpu(HL, S, case):
    """Everything of a case on the CPU: dict(sc, X0, X1, E, inliers, mask, caller)."""
    sc = scene_of(case)
    X0, X1 = points_cpu(sc)
    E, inl = estimate_cpu(case, X0, X1)
    mask, caller = design(HL, S, case, sc, X0, X1, E, inl)
    return dict(case=case, sc=sc, X0=X0, X1=X1, E=E, inliers=inl, mask=mask, caller=caller)


GENERIC_Z_FIXTURE = os.path.join(ROOT, "tests", "golden", "refine_generic_z_case.npz")


def unit_z(X):
    """The same rays at z = 1: (x / z, y / z, 1), the divisions in float32 as the kernels do them."""
    X = np.ascontiguousarray(X, np.float32)
    return np.stack([X[0] / X[2], X[1] / X[2], np.ones_like(X[2])])


def obs_of(X0, X1):
    return np.stack([X0[0] / X0[2], X0[1] / X0[2], X1[0] / X1[2], X1[1] / X1[2]], 1)


def cam_of(K):
    return (float(K[0, 0]), float(K[0, 1]), float(K[1, 1]))
