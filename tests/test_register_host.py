"""CPU: the view registration's arithmetic without a GPU -- csrc/register_math.hpp host-compiled into
tests/hostcheck/libregistercheck.so: Lambda Twist against ground truth and an independent fp64 P3P (tests/register_reference.py),
degenerate samples, the 4th point's choice, the sampler, the inlier test against the fp64 pixel error, the pose Jacobian against
finite differences, the numpy LM twin, and the ctypes mirrors of the new structs."""
import ctypes as C
import os

import numpy as np
import pytest

import register_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hostcheck", "libregistercheck.so")
f32p = C.POINTER(C.c_float)
CAM = (2360.0, 0.0, 2360.0)


@pytest.fixture(scope="module")
def L():
    h = C.CDLL(LIB)
    h.rg_sample4.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    h.rg_p3p.argtypes = [f32p, f32p, f32p]
    h.rg_inlier.argtypes = [f32p, C.c_float, f32p, f32p, C.c_float, C.c_float]
    h.rg_sq_error.argtypes = [f32p, f32p, f32p, C.c_float, C.c_float]
    h.rg_sq_error.restype = C.c_float
    h.rg_hypothesis.argtypes = [C.c_uint32, C.c_uint32, C.c_int, f32p, f32p, f32p, f32p]
    h.rg_jacobian.argtypes = [f32p, f32p, f32p, C.c_float, C.c_float, f32p]
    h.rg_solve6.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    h.rg_layout.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    return h


def fp(a):
    return a.ctypes.data_as(f32p)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def well_conditioned_triple(rng):
    """Three points around the optical axis of a camera inside their circumscribed cylinder (far from P3P's danger cylinder),
    in a random world frame: (R, t, camera-frame points, world points)."""
    a = 2 * np.pi * np.arange(3) / 3 + rng.uniform(-0.3, 0.3, 3)
    r = rng.uniform(0.8, 1.2, 3)
    Xc = np.column_stack([r * np.cos(a) + rng.uniform(-0.3, 0.3), r * np.sin(a) + rng.uniform(-0.3, 0.3), rng.uniform(2.5, 3.5, 3)])
    u = rng.standard_normal(3)
    R, t = random_rotation(rng), 2.0 * u / np.linalg.norm(u)
    return R, t, Xc, (Xc - t) @ R


def solutions(L, y, Xw):
    out = np.zeros(48, np.float32)
    n = L.rg_p3p(fp(f32(y)), fp(f32(Xw)), fp(out))
    return [(out[12 * k:12 * k + 9].reshape(3, 3).astype(np.float64), out[12 * k + 9:12 * k + 12].astype(np.float64)) for k in range(n)]


def rot_err(A, B):
    return np.linalg.norm(A - B) / np.sqrt(2.0)          # ~ the rotation angle for small errors, also for a slightly skew A


def test_p3p_recovers_the_true_pose_and_the_fp64_solution_set(L):
    rng = np.random.default_rng(7)
    errs, matched = [], 0
    for _ in range(300):
        R, t, Xc, Xw = well_conditioned_triple(rng)
        y = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
        sols = solutions(L, y, Xw)
        assert 1 <= len(sols) <= 4
        e = [max(rot_err(Rk, R), np.linalg.norm(tk - t) / np.linalg.norm(t)) for Rk, tk in sols]
        errs.append(min(e))
        # the independent fp64 solver on the same fp32 inputs finds the same set
        ref = GR.p3p(f32(y).astype(np.float64), f32(Xw).astype(np.float64))
        if len(ref) == len(sols) and all(min(rot_err(Rk, Rr) for Rr, _ in ref) < 1e-3 for Rk, _ in sols):
            matched += 1
    # fp32 bearings: a few triples lose digits to the conditioning of the distance equations
    errs = np.array(errs)
    assert np.median(errs) < 1e-5 and np.mean(errs < 1e-4) >= 0.95 and np.mean(errs < 1e-2) >= 0.99, np.quantile(errs, [0.5, 0.95, 0.99])
    assert matched >= 0.95 * len(errs), matched


def test_degenerate_samples_score_nothing(L):
    cam = f32(CAM)
    rng = np.random.default_rng(3)
    Xline = np.stack([np.linspace(-1, 1, 8), 0.5 * np.linspace(-1, 1, 8), 5.0 + np.linspace(0, 1, 8)], 1)   # collinear
    Xsame = np.tile([[0.2, -0.1, 5.0]], (8, 1))                                                              # coincident
    Xback = np.column_stack([rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8), -rng.uniform(4, 8, 8)])          # behind camera 3
    for X in (Xline, Xsame, Xback):
        obs = X[:, :2] / np.abs(X[:, 2:])
        Xc = f32(np.column_stack([X, np.zeros(8)]))
        for h in range(64):
            P = np.full(12, np.nan, np.float32)
            ok = L.rg_hypothesis(11, h, 8, fp(cam), fp(Xc), fp(f32(obs)), fp(P))
            assert np.isfinite(P).all()
            if not ok:
                assert not P.any()
                count = sum(L.rg_inlier(fp(cam), 4.0, fp(P), fp(f32(X[k])), float(obs[k, 0]), float(obs[k, 1])) for k in range(8))
                assert count == 0
            else:       # (a behind-camera sample can only win with a pose that puts the points in front of it)
                assert X is Xback
    # fewer than four candidates: no sample at all
    P = np.ones(12, np.float32)
    assert L.rg_hypothesis(1, 0, 3, fp(cam), fp(f32(np.zeros((3, 4)))), fp(f32(np.zeros((3, 2)))), fp(P)) == 0 and not P.any()


def test_fourth_point_picks_the_true_pose(L):
    rng = np.random.default_rng(5)
    cam = f32(CAM)
    picked = 0
    for _ in range(200):
        R, t, Xc, Xw = well_conditioned_triple(rng)
        y = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
        sols = solutions(L, y, Xw)
        if len(sols) < 2:
            continue
        X4c = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2.5, 3.5)])
        X4w = (X4c - t) @ R
        cands = f32(np.column_stack([np.vstack([Xw, X4w]), np.zeros(4)]))
        obs = f32(np.vstack([Xc[:, :2] / Xc[:, 2:], X4c[:2] / X4c[2]]))
        # the sampler's order for m = 4 is a permutation: feed the points in that order so that the 4th sample is X4
        idx = (C.c_int * 4)()
        L.rg_sample4(9, 0, 4, idx)
        order = np.empty(4, int)
        order[list(idx)] = [0, 1, 2, 3]
        P = np.zeros(12, np.float32)
        assert L.rg_hypothesis(9, 0, 4, fp(cam), fp(f32(cands[order])), fp(f32(obs[order])), fp(P)) == 1
        e = [rot_err(P[:9].reshape(3, 3).astype(np.float64), Rk) for Rk, _ in sols]
        assert min(e) < 1e-3                                # one of the solutions (bearings rounded the solver's way)
        k = int(np.argmin([rot_err(Rk, R) for Rk, _ in sols]))
        picked += int(np.argmin(e)) == k
    assert picked >= 190, picked


def test_sample4_distinct_and_pure(L):
    for m in (4, 5, 37, 1000, 4096):
        for h in range(200):
            a = (C.c_int * 4)(); b = (C.c_int * 4)()
            L.rg_sample4(0x5EED5F3D, h, m, a)
            L.rg_sample4(0x5EED5F3D, h, m, b)
            assert list(a) == list(b) and len(set(a)) == 4 and all(0 <= v < m for v in a)
    seen = set()
    for h in range(50):
        a = (C.c_int * 4)()
        L.rg_sample4(1, h, 1000, a)
        seen.add(tuple(a))
    assert len(seen) == 50


def test_inlier_test_agrees_with_fp64_pixel_error(L):
    rng = np.random.default_rng(2)
    cam = np.array(CAM, np.float32); cam[1] = 3.0
    R, t = random_rotation(rng) * 0 + np.eye(3), np.array([0.1, -0.2, 0.3])
    P = f32(np.concatenate([R.ravel(), t]))
    thr = 4.0
    disagree = 0
    for _ in range(4000):
        X = f32(np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 6)]))
        Y = P[:9].reshape(3, 3).astype(np.float64) @ X + P[9:]
        obs = f32(Y[:2] / Y[2] + rng.uniform(-6, 6, 2) / np.array([cam[0], cam[2]]))
        e = GR.pixel_error(tuple(map(float, cam)), P[:9].reshape(3, 3), P[9:], X[None].astype(np.float64), obs[None].astype(np.float64))[0]
        got = L.rg_inlier(fp(cam), thr, fp(P), fp(X), float(obs[0]), float(obs[1]))
        if abs(e - thr) > 1e-3:
            assert got == (e < thr), (e, got)
        else:
            disagree += 1
    # behind the camera: never an inlier
    X = f32([0.0, 0.0, -5.0])
    assert L.rg_inlier(fp(cam), 1e6, fp(P), fp(X), 0.0, 0.0) == 0
    assert L.rg_sq_error(fp(cam), fp(P), fp(X), 0.0, 0.0) == np.inf


def test_pose_jacobian_matches_finite_differences(L):
    rng = np.random.default_rng(4)
    cam = (2360.0, 2.0, 2350.0)
    for _ in range(50):
        R = GR.expso3(rng.normal(0, 0.3, 3)); t = rng.normal(0, 1, 3)
        X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
        obs = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        out = np.zeros(15, np.float32)
        L.rg_jacobian(fp(f32(cam)), fp(f32(np.concatenate([R.ravel(), t]))), fp(f32(X)), float(obs[0]), float(obs[1]), fp(out))
        r64, J64 = GR.jacobian(cam, R, t, X[None], obs[None])
        assert np.allclose(out[:2], r64[0], rtol=1e-4, atol=1e-2)
        num = np.zeros((2, 6))
        for k in range(6):
            d = np.zeros(6); d[k] = 1e-6
            rp, _ = GR.pixel_residual(cam, GR.expso3(d[:3]) @ R, t + d[3:], X[None], obs[None])
            rm, _ = GR.pixel_residual(cam, GR.expso3(-d[:3]) @ R, t - d[3:], X[None], obs[None])
            num[:, k] = (rp[0] - rm[0]) / 2e-6
        assert np.allclose(J64[0], num, rtol=1e-5, atol=1e-3)
        assert np.allclose(out[2:14].reshape(2, 6), num, rtol=2e-3, atol=0.5)


def test_solve6_against_numpy(L):
    rng = np.random.default_rng(8)
    A = rng.standard_normal((6, 6)); A = A @ A.T + 6 * np.eye(6)
    b = rng.standard_normal(6)
    S = (C.c_double * 21)(*[A[i, j] for i in range(6) for j in range(i, 6)])
    x = (C.c_double * 6)(*b)
    assert L.rg_solve6(S, x) == 1
    assert np.allclose(np.array(x), np.linalg.solve(A, b), rtol=1e-12)
    S = (C.c_double * 21)(*([-1.0] * 21))
    assert L.rg_solve6(S, (C.c_double * 6)()) == 0


def test_numpy_lm_twin_converges_on_noisy_scenes():
    rng = np.random.default_rng(6)
    cam = CAM
    for seed in range(3):
        X = np.column_stack([rng.uniform(-1, 1, 400), rng.uniform(-1, 1, 400), rng.uniform(4, 8, 400)])
        R, t = GR.expso3(rng.normal(0, 0.3, 3)), np.array([2.0, 0.2, 0.4])
        Y = X @ R.T + t
        obs = Y[:, :2] / Y[:, 2:] + rng.normal(0, 0.5, (400, 2)) / cam[0]
        R0, t0 = GR.expso3(rng.normal(0, 2e-3, 3)) @ R, t + rng.normal(0, 2e-2, 3)
        out = GR.refine_pose(cam, R0, t0, X, obs, max_iterations=30)
        assert out["final_rms_px"] < out["initial_rms_px"] and out["final_rms_px"] < 0.6
        assert rot_err(out["R"], R) < 1e-3 and np.linalg.norm(out["t"] - t) < 1e-2 * np.linalg.norm(t)


def test_ctypes_mirrors_equal_sizeof_and_offsetof(L):
    """A C build of include/sfm_amd.h reports sizeof / offsetof of sfm_register_params and sfm_register_report; the ctypes
    mirrors agree field by field, and the header's new constants have their Python mirrors."""
    import cuda_sfm_amd as S
    for which, cls in ((0, S.RegisterParams), (1, S.RegisterReport)):
        out = (C.c_int64 * 32)()
        n = L.rg_layout(which, out)
        assert n == len(cls._fields_)
        assert out[0] == C.sizeof(cls), cls
        assert [out[1 + k] for k in range(n)] == [getattr(cls, f).offset for f, _ in cls._fields_], cls
    txt = open(os.path.join(ROOT, "include", "sfm_amd.h")).read()
    for name, val in (("SFM_BUF_VIEW_POSE", S.BUF_VIEW_POSE), ("SFM_BUF_VIEW_COUNTS", S.BUF_VIEW_COUNTS),
                      ("SFM_BUF_VIEW_REPROJ", S.BUF_VIEW_REPROJ)):
        assert f"#define {name}" in txt and int(txt.split(f"#define {name}")[1].split()[0]) == val
    p = S.register_params()
    assert (p.num_hypotheses, p.threshold_px, p.max_iterations) == (4096, 4.0, 10) and not any(p.reserved)
