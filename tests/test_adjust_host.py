"""CPU: sfm_adjust_view / sfm_adjust_views without a device -- the header's Jacobians against central differences, one point's
88 Schur values against the twin's dense normal equations for each view class, the fp64 twin (tests/adjust_reference.py) against
ground truth, the host build (tests/hostcheck/libadjustcheck.so: the header's functions, serial fp64 sums) against the twin on
the checked scenes, struct layouts, header / exports / Python mirror, the argument checks that precede the device, and the
compiler's resource report of adjust.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adjust_reference as AR
import adjust_scene as AS
import refine_reference as RR
import view_points_scene as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sfm_adjust_default_params", "sfm_adjust_view", "sfm_adjust_views"]
f32p = C.POINTER(C.c_float)
# host build against the twin, DESIGN 6b's bars: poses within 2e-5 rad / 2e-5 in t, rms within 1e-4 px, either stop status.  The
# looser pair (1e-4, 1e-3) is not needed: largest differences on the three scenes 1.0e-6 rad, 7.4e-6 in t (camera 3 of scene
# (1024, 61), which only 12 records see), 6.8e-7 px.
ROT_BAR, T_BAR, RMS_BAR = 2e-5, 2e-5, 1e-4


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def AL():
    h = AS.host_lib()
    h.adj_jacobian.argtypes = [f32p] * 4 + [C.c_int, f32p]
    h.adj_terms.argtypes = [f32p] * 4 + [C.c_int, C.c_float, C.c_float, f32p, f32p]
    return h


@pytest.fixture(scope="module")
def runs(S, AL):
    """Per checked scene: the inputs at the perturbed start, the twin's result and the host build's, computed once."""
    HL = VS.host_lib()
    out = []
    for n, seed in AS.SCENES:
        s = AS.start(n, seed, HL, S)
        out.append((s, AS.run_twin(AR, s), AS.run_host(AL, S, s)))
    return out


def fp(a):
    return a.ctypes.data_as(f32p)


def case(n=64, seed=3):
    """Exact cameras slightly off the truth, points 1 % off, observations with 0.5 px of noise: cam, state pieces, obs (n x 6), X."""
    import register_scene as RS
    from cuda_sfm_amd_synth import synth
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.0)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=0.5)
    K = sc["K"].astype(np.float64)
    cam = np.array([K[0, 0], K[0, 1], K[1, 1]], np.float32)
    X0, X1 = synth.normalized_points(sc)
    obs = AR.observations(sc["Kinv"], rec, X0, X1).astype(np.float32)
    R2 = sc["R"] @ RR.expso3(np.array([1e-3, -2e-3, 5e-4]))
    t2 = sc["t"] + np.array([0.01, -0.02, 0.005]); t2 /= np.linalg.norm(t2)
    R3 = truth["R3"] @ RR.expso3(np.array([-1e-3, 1e-3, 2e-3]))
    t3 = truth["t3"] + np.array([0.01, 0.02, -0.01])
    X = (sc["points3d"] * 1.01).astype(np.float32)
    return cam, R2, t2, R3, t3, obs, X


def state30(R2, t2, R3, t3, basis_of=None):
    b1, b2 = RR.tangent_basis(np.asarray(t2 if basis_of is None else basis_of, np.float64))
    return np.concatenate([np.asarray(R2).ravel(), t2, b1, b2, np.asarray(R3).ravel(), t3]).astype(np.float32)


def lib_jac(AL, cam, state, o, X, bits):
    out = np.zeros(46, np.float32)
    AL.adj_jacobian(fp(cam), fp(state), fp(np.ascontiguousarray(o, np.float32)), fp(np.ascontiguousarray(X, np.float32)), int(bits), fp(out))
    return out[:6].astype(np.float64), out[6:24].reshape(6, 3).astype(np.float64), out[24:34].reshape(2, 5).astype(np.float64), \
        out[34:46].reshape(2, 6).astype(np.float64)


@pytest.mark.parametrize("bits", [3, 5, 7])
def test_jacobians_match_central_differences(AL, bits):
    """Steps and bars of tests/test_refine_host.py: points 1e-3, cameras 1e-4, 1e-3 of the block's largest entry."""
    cam, R2, t2, R3, t3, obs, X = case()
    b1, b2 = RR.tangent_basis(t2)
    st = state30(R2, t2, R3, t3)
    rows = [v for v in range(3) if bits & (1 << v)]
    for j in range(0, 64, 7):
        r, Jp, Jc2, Jc3 = lib_jac(AL, cam, st, obs[j], X[j], bits)
        for v in range(3):
            if v not in rows:                                                  # a view that does not see the point: zeros
                assert not r[2 * v:2 * v + 2].any() and not Jp[2 * v:2 * v + 2].any()
        assert (bits & 2) or not Jc2.any()
        assert (bits & 4) or not Jc3.any()
        h = 1e-3
        for c in range(3):
            d = np.zeros(3); d[c] = h
            fd = (lib_jac(AL, cam, st, obs[j], X[j] + d, bits)[0] - lib_jac(AL, cam, st, obs[j], X[j] - d, bits)[0]) / (2 * h)
            assert np.abs(fd - Jp[:, c]).max() <= 1e-3 * np.abs(Jp).max(), (j, c, fd, Jp[:, c])
        hh = 1e-4
        for c in range(11):
            def at(sgn):
                dc = np.zeros(11); dc[c] = sgn * hh
                R2p = RR.expso3(dc[:3]) @ R2
                t2p = t2 + b1 * dc[3] + b2 * dc[4]; t2p /= np.linalg.norm(t2p)
                R3p = RR.expso3(dc[5:8]) @ R3
                return lib_jac(AL, cam, state30(R2p, t2p, R3p, t3 + dc[8:11], basis_of=t2), obs[j], X[j], bits)[0]
            fd = (at(1) - at(-1)) / (2 * hh)
            assert np.abs(fd[:2]).max() == 0.0                                 # camera 1 is fixed
            if c < 5:
                assert np.abs(fd[4:]).max() == 0.0                             # view 3 does not see camera 2
                assert np.abs(fd[2:4] - Jc2[:, c]).max() <= 1e-3 * max(np.abs(Jc2).max(), 1e-30), (j, c, fd, Jc2[:, c])
            else:
                assert np.abs(fd[2:4]).max() == 0.0
                assert np.abs(fd[4:] - Jc3[:, c - 5]).max() <= 1e-3 * max(np.abs(Jc3).max(), 1e-30), (j, c, fd, Jc3[:, c - 5])


@pytest.mark.parametrize("huber", [0.0, 1.0, 0.2])
@pytest.mark.parametrize("bits", [3, 5, 7])
def test_schur_terms_match_the_twins_dense_system(AL, bits, huber):
    """rtol / atol of tests/test_refine_host.py's Schur test, on the 11-wide system."""
    cam, R2, t2, R3, t3, obs, X = case()
    st = state30(R2, t2, R3, t3)
    lam = 1e-2
    f = lambda a: a.astype(np.float64)
    Rf2, tf2, Rf3, tf3 = f(st[:9]).reshape(3, 3), f(st[9:12]), f(st[18:27]).reshape(3, 3), f(st[27:30])
    m = 16
    sy = AR.system(tuple(float(c) for c in cam), Rf2, tf2, Rf3, tf3, f(X[:m]), f(obs[:m]), np.full(m, bits), huber, lam)
    iu3, iu11 = np.triu_indices(3), np.triu_indices(11)
    dc = np.array([1e-4, -2e-4, 3e-5, 1e-3, -1e-3, 2e-4, 1e-4, -3e-4, 1e-3, 2e-3, -1e-3], np.float32)
    for j in range(m):
        out = np.zeros(136, np.float32)
        AL.adj_terms(fp(cam), fp(st), fp(obs[j].copy()), fp(X[j].copy()), bits, C.c_float(huber), C.c_float(lam), fp(dc), fp(out))
        w, Vi, Wm, gp, sys_, dp = out[:3], out[3:9], out[9:42].reshape(11, 3), out[42:45], out[45:133], out[133:136]
        Uj, Sj = sy["U_pt"][j], sy["S_pt"][j]
        assert np.allclose(w, sy["w"][j], rtol=1e-4, atol=1e-6)
        assert np.allclose(Vi, sy["Vi"][j][iu3], rtol=1e-4, atol=1e-4 * np.abs(sy["Vi"][j]).max())
        assert np.allclose(Wm, sy["Wm"][j], rtol=1e-4, atol=1e-5 * np.abs(sy["Wm"][j]).max())
        assert np.allclose(gp, sy["gp"][j], rtol=1e-3, atol=1e-4 * np.abs(sy["gp"][j]).max() + 1e-3)
        assert np.allclose(sys_[:66], Sj[iu11], rtol=1e-3, atol=2e-3 * np.abs(Uj).max())
        assert np.allclose(sys_[77:88], np.diag(Uj), rtol=1e-4, atol=1e-6 * np.abs(Uj).max())
        assert np.allclose(sys_[66:77], sy["b_pt"][j], rtol=1e-3, atol=2e-3 * np.abs(sy["b_pt"][j]).max() + 1e-2)
        # the block of camera 2 x camera 3: zero unless both see the point
        S11 = np.zeros((11, 11)); S11[iu11] = sys_[:66]
        cross = S11[:5, 5:]
        if bits == 7:
            assert np.abs(cross).max() > 1e-3 * np.abs(S11).max() and np.abs(Sj[:5, 5:]).max() > 0
        else:
            assert not cross.any() and not Sj[:5, 5:].any()
        want = -sy["Vi"][j] @ (sy["gp"][j] + sy["Wm"][j].T @ dc.astype(np.float64))
        assert np.allclose(dp, want, rtol=1e-3, atol=1e-3 * np.abs(want).max() + 1e-7)


def test_twin_recovers_noise_free_ground_truth():
    """No noise, no outliers, exact fp64 observations; the start 2e-3 rad and 1 % off in t2, R3 and t3, the points triangulated at
    the perturbed pair.  The bars of test_reference_recovers_noise_free_ground_truth."""
    import register_scene as RS
    from cuda_sfm_amd_synth import synth
    sc = synth.two_view_scene(512, seed=5, noise_px=0.0, outlier_frac=0.0)
    K = sc["K"].astype(np.float64)
    G = sc["points3d"]
    R3, t3 = RS.R3_DEFAULT, RS.T3_DEFAULT
    Y2, Y3 = G @ sc["R"].T + sc["t"], G @ R3.T + t3
    obs = np.stack([G[:, 0] / G[:, 2], G[:, 1] / G[:, 2], Y2[:, 0] / Y2[:, 2], Y2[:, 1] / Y2[:, 2], Y3[:, 0] / Y3[:, 2], Y3[:, 1] / Y3[:, 2]], 1)
    rng = np.random.default_rng(0)
    R2s = RR.expso3(AS.ROT * AS._unit(rng)) @ sc["R"]
    t2s = sc["t"] + AS.REL * AS._unit(rng); t2s /= np.linalg.norm(t2s)
    R3s = RR.expso3(AS.ROT * AS._unit(rng)) @ R3
    t3s = t3 + AS.REL * np.linalg.norm(t3) * AS._unit(rng)
    x = np.ones((3, 512)); x[:2] = obs[:, 0:2].T
    y = np.ones((3, 512)); y[:2] = obs[:, 2:4].T
    Xs = VS.two_view_points(x, y, R2s, t2s)
    bits = np.where(np.arange(512) % 3 == 0, 7, np.where(np.arange(512) % 3 == 1, 3, 5))     # all three view classes
    rep = AR.adjust((K[0, 0], K[0, 1], K[1, 1]), R2s, t2s, R3s, t3s, Xs, obs, bits, max_iterations=100, min_rel_decrease=1e-12)
    assert RR.rotation_angle(rep["R2"], sc["R"]) < 1e-9 and np.abs(rep["t2"] - sc["t"]).max() < 1e-9
    assert RR.rotation_angle(rep["R3"], R3) < 1e-9 and np.abs(rep["t3"] - t3).max() < 1e-9
    assert rep["final_rms_px"] < 1e-4


def test_view_bits_are_equal_on_every_record(runs):
    for s, (_, _, tv, _, tr), (_, _, hv, _, hr) in runs:
        assert np.array_equal(tv, hv)
        assert (hr["num_points"], hr["num_view2"], hr["num_view3"]) == (tr["num_points"], tr["num_view2"], tr["num_view3"])
        assert hr["num_points"] == int((hv != 0).sum()) and hr["num_view2"] == int(((hv & 2) != 0).sum())
        assert set(np.unique(hv)) <= {0, 3, 5, 7}
        assert ((hv & 4) != 0).sum() == np.isin(s["vp_flags"][hv != 0], (AR.NEW, AR.REFINED)).sum()


def test_host_build_agrees_with_the_fp64_twin(runs):
    for s, (tp, tpts, tv, terr, tr), (hp, hpts, hv, herr, hr) in runs:
        print(s["n"], "start", AS.pose_errors(s["poses"], s), "twin", AS.pose_errors(tp, s), "host", AS.pose_errors(hp, s),
              "rms", tr["initial_rms_px"], tr["final_rms_px"], hr["final_rms_px"], "iterations", tr["iterations"], hr["iterations"])
        assert hr["status"] in (AR.CONVERGED, AR.MAX_ITER) and tr["status"] in (AR.CONVERGED, AR.MAX_ITER)
        assert RR.rotation_angle(hp[:9].reshape(3, 3), tp[:9].reshape(3, 3)) <= ROT_BAR
        assert RR.rotation_angle(hp[12:21].reshape(3, 3), tp[12:21].reshape(3, 3)) <= ROT_BAR
        assert np.abs(hp[9:12] - tp[9:12]).max() <= T_BAR and np.abs(hp[21:24] - tp[21:24]).max() <= T_BAR
        assert abs(hr["final_rms_px"] - tr["final_rms_px"]) <= RMS_BAR and abs(hr["initial_rms_px"] - tr["initial_rms_px"]) <= RMS_BAR
        u = hv != 0
        assert np.array_equal(hpts[:, ~u], s["vp_points"][:, ~u]) and np.isinf(herr[~u]).all()
        assert (hpts[3, u] == 1.0).all() and np.isfinite(herr[u]).all()


def test_host_build_improves_what_the_twin_improves(runs):
    """Against the start, per scene and quantity: where the twin's error is below the start's, the host build's is within 1.25 x
    the twin's; where the twin does not improve a quantity, nothing is asserted about it (camera 3 of scene (1024, 61): at the
    perturbed start only 12 of its records pass sfm_triangulate_view's 4 px test, and the twin's camera 3 ends further from the
    truth than it started).  The rms always falls."""
    for s, (tp, _, _, _, tr), (hp, _, _, _, hr) in runs:
        e0, et, eh = AS.pose_errors(s["poses"], s), AS.pose_errors(tp, s), AS.pose_errors(hp, s)
        improved = [k for k in range(4) if et[k] < e0[k]]
        assert {0, 1} <= set(improved), (s["n"], e0, et)                       # camera 2 improves on every scene
        for k in improved:
            assert eh[k] <= 1.25 * et[k], (s["n"], k, e0[k], et[k], eh[k])
        assert tr["final_rms_px"] < tr["initial_rms_px"] and hr["final_rms_px"] <= 1.25 * tr["final_rms_px"]


def test_zero_iterations_and_degenerate_inputs_return_the_start(S, AL):
    HL = VS.host_lib()
    s = AS.start(257, 7, HL, S)
    hp, hpts, hv, herr, hr = AS.run_host(AL, S, s, max_iterations=0)
    assert hr["status"] == AR.MAX_ITER and hr["iterations"] == 0 and hr["final_rms_px"] == hr["initial_rms_px"]
    assert np.array_equal(hp, s["poses"])
    u = hv != 0
    assert np.allclose(hpts[:3, u], s["vp_points"][:3, u] / s["vp_points"][3, u], rtol=1e-6) and (hpts[3, u] == 1).all()
    # 15 records in view 2: degenerate; 16: not
    for keep, status in ((15, AR.DEGENERATE), (16, None)):
        used2 = np.zeros(s["n"], np.uint8)
        used2[np.flatnonzero((hv & 2) != 0)[:keep]] = 1
        p, pts, v, err, r = AS.run_host(AL, S, s, used2=used2)
        tw = AS.run_twin(AR, s, used2=used2)
        assert r["num_view2"] == keep and np.array_equal(v, tw[2])
        if status is not None:
            assert r["status"] == status == tw[4]["status"] and np.array_equal(p, s["poses"]) and np.array_equal(pts, s["vp_points"])
            assert np.isfinite(err[v != 0]).all() and np.isinf(err[v == 0]).all()
        else:
            assert r["status"] != AR.DEGENERATE
    for keep, status in ((5, AR.DEGENERATE), (6, None)):
        flags = s["vp_flags"].copy()
        see3 = np.flatnonzero((hv & 4) != 0)
        flags[see3[keep:]] = AR.KEPT
        p, pts, v, err, r = AS.run_host(AL, S, s, flags=flags)
        assert r["num_view3"] == keep and np.array_equal(v, AS.run_twin(AR, s, flags=flags)[2])
        assert (r["status"] == AR.DEGENERATE) == (status is not None)
    # no used record; a W = 0 column and a NaN column among used ones
    p, pts, v, err, r = AS.run_host(AL, S, s, used2=np.zeros(s["n"], np.uint8), flags=np.zeros(s["n"], np.uint8))
    assert not v.any() and r["status"] == AR.DEGENERATE and r["num_points"] == 0 and r["final_rms_px"] == 0 and np.array_equal(pts, s["vp_points"])
    pts_in = s["vp_points"].copy()
    a, b = np.flatnonzero(hv != 0)[:2]
    pts_in[3, a] = 0.0; pts_in[1, b] = np.nan
    p, pts, v, err, r = AS.run_host(AL, S, s, points=pts_in)
    assert v[a] == 0 and v[b] == 0 and r["num_points"] == hr["num_points"] - 2 and np.array_equal(v, AS.run_twin(AR, s, points=pts_in)[2])
    assert np.array_equal(pts[:, [a, b]].view(np.uint32), pts_in[:, [a, b]].view(np.uint32)) and np.isfinite(p).all()


def test_header_exports_wrapper_and_integration_md_agree(S):
    hdr = open(os.path.join(ROOT, "include", "sfm_amd.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    facade = open(os.path.join(ROOT, "cuda-sfm_amd", "host", "sfm.h")).read()
    for name in NAMES:
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
    assert "sfm_adjust_view" in facade and "sfm_adjust_views" in facade
    assert S.lib().sfm_abi_version() == 3 and S.ABI_VERSION == 3
    assert (S.ADJ_VIEW1, S.ADJ_VIEW2, S.ADJ_VIEW3) == (1, 2, 4)
    for fn in ("adjust_params", "adjust_views_enqueue", "adjust_views"):
        assert callable(getattr(S, fn))
    for fn in ("adjust_view_enqueue", "adjust_view"):
        assert callable(getattr(S.ImagePair, fn))
    p = S.adjust_params()
    assert np.allclose((p.max_iterations, p.huber_px, p.min_rel_decrease, p.initial_lambda), (20, 1.0, 1e-6, 1e-3), rtol=1e-6)
    assert not p.d_used2 and not p.d_poses and list(p.reserved) == [0] * 4
    assert (AR.MIN_VIEW2, AR.MIN_VIEW3) == (16, 6) and AR.DEFAULTS == dict(max_iterations=20, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3)
    with pytest.raises(TypeError):
        S.adjust_params(max_iteration=0)


def test_ctypes_mirrors_equal_sizeof_and_offsetof_of_the_header(S, AL, tmp_path):
    structs = (("sfm_adjust_params", S.AdjustParams), ("sfm_adjust_in", S.AdjustIn), ("sfm_adjust_report", S.AdjustReport), ("sfm_adjust_out", S.AdjustOut))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sfm_amd.h"', 'int main(void) {']
    for st, cls in structs:
        lines.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{st}.{f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st} *)0)->{f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = tuple(int(x) for x in v)
    for which, (st, cls) in enumerate(structs):
        assert got[st] == (C.sizeof(cls),), (st, got[st], C.sizeof(cls))
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert got[f"{st}.{f}"] == (d.offset, d.size), (st, f, got[f"{st}.{f}"], d.offset, d.size)
        lay = (C.c_int64 * 16)()                       # the host build of the same header (HIP host compiler)
        k = AL.adj_layout(which, lay)
        assert k == len(cls._fields_) and lay[0] == C.sizeof(cls)
        assert [lay[1 + i] for i in range(k)] == [getattr(cls, f).offset for f, _ in cls._fields_]


def test_argument_checks_answer_before_any_device_call(S):
    """Every pointer below is a made-up address: a check that came after a dereference or a device call would not return."""
    L = S.lib()
    vp = C.c_void_p
    B = 0x100000
    fake_pair = vp(0x1000)
    good_in = S.AdjustIn(0x2000, 1 * B, 2 * B)
    good_out = S.AdjustOut(3 * B, 4 * B, 5 * B, 6 * B, 7 * B)
    ok = S.adjust_params()
    ref = lambda x: C.byref(x) if x is not None else None
    single = lambda p=ok, i=good_in, o=good_out, pair=fake_pair: L.sfm_adjust_view(pair, ref(i), ref(p), ref(o))
    assert single(pair=None) == S.E_INVALID and single(i=None) == S.E_INVALID and single(p=None) == S.E_INVALID and single(o=None) == S.E_INVALID
    nan, inf = float("nan"), float("inf")
    bad = (dict(reserved=[0, 0, 0, 1]), dict(reserved=[1, 0, 0, 0]), dict(max_iterations=-1), dict(max_iterations=201), dict(huber_px=-1.0),
           dict(huber_px=inf), dict(min_rel_decrease=-1.0), dict(min_rel_decrease=nan), dict(initial_lambda=-1.0), dict(initial_lambda=inf))
    for kw in bad:
        assert single(p=S.adjust_params(**kw)) == S.E_INVALID, kw
        assert L.sfm_adjust_views(None, 0, None, C.byref(S.adjust_params(**kw)), None) == S.E_INVALID, kw
    for k in range(3):                                                         # required inputs
        a = [0x2000, 1 * B, 2 * B]; a[k] = None
        assert single(i=S.AdjustIn(*a)) == S.E_INVALID
    for k in (0, 1, 2, 4):                                                     # required outputs (d_err is optional)
        a = [3 * B, 4 * B, 5 * B, 6 * B, 7 * B]; a[k] = None
        assert single(o=S.AdjustOut(*a)) == S.E_INVALID
    assert single(i=S.AdjustIn(0x2008, 1 * B, 2 * B)) == S.E_INVALID and b"16-byte aligned" in L.sfm_last_error()
    # an output on an input, on a parameter's array, or on another output
    for k in range(5):
        for target in (0x2000, 1 * B, 2 * B):
            a = [3 * B, 4 * B, 5 * B, 6 * B, 7 * B]; a[k] = target
            assert single(o=S.AdjustOut(*a)) == S.E_INVALID and b"overlaps" in L.sfm_last_error(), (k, target)
        for q in range(k + 1, 5):
            a = [3 * B, 4 * B, 5 * B, 6 * B, 7 * B]; a[q] = a[k]
            assert single(o=S.AdjustOut(*a)) == S.E_INVALID and b"overlaps" in L.sfm_last_error(), (k, q)
        a = [3 * B, 4 * B, 5 * B, 6 * B, 7 * B]
        assert single(p=S.adjust_params(used2=a[k], poses=8 * B)) == S.E_INVALID and single(p=S.adjust_params(used2=8 * B, poses=a[k])) == S.E_INVALID
    assert single(p=S.adjust_params(used2=8 * B, poses=9 * B), o=S.AdjustOut(9 * B + 92, 4 * B, 5 * B, 6 * B, 7 * B)) == S.E_INVALID    # inside the 96 bytes
    assert single(o=S.AdjustOut(7 * B + 36, 4 * B, 5 * B, 6 * B, 7 * B)) == S.E_INVALID                                                  # inside the report
    # the batched call
    many = lambda pairs, n, ins, p, outs: L.sfm_adjust_views(pairs, n, ins, ref(p), outs)
    pairs2 = (vp * 2)(0x1000, None)
    ins2 = (S.AdjustIn * 2)(good_in, good_in)
    outs2 = (S.AdjustOut * 2)(good_out, S.AdjustOut(13 * B, 14 * B, 15 * B, 16 * B, 17 * B))
    assert many(None, 0, None, ok, None) == S.OK and many(pairs2, 0, ins2, ok, outs2) == S.OK      # an empty list
    assert many(pairs2, 2, ins2, None, outs2) == S.E_INVALID
    assert many(pairs2, -1, ins2, ok, outs2) == S.E_INVALID and many(pairs2, 65536, ins2, ok, outs2) == S.E_INVALID
    assert many(None, 2, ins2, ok, outs2) == S.E_INVALID and many(pairs2, 2, None, ok, outs2) == S.E_INVALID and many(pairs2, 2, ins2, ok, None) == S.E_INVALID
    assert many(pairs2, 2, ins2, ok, outs2) == S.E_INVALID and b"pairs[1] is null" in L.sfm_last_error()
    assert many((vp * 2)(None, 0x1000), 2, ins2, ok, outs2) == S.E_INVALID and b"pairs[0] is null" in L.sfm_last_error()
    one = (vp * 1)(0x1000)
    assert many(one, 1, (S.AdjustIn * 1)(S.AdjustIn(0x2004, 1 * B, 2 * B)), ok, outs2) == S.E_INVALID and b"pairs[0]: d_sift must be 16-byte aligned" in L.sfm_last_error()
    assert many(one, 1, (S.AdjustIn * 1)(S.AdjustIn(0x2000, None, 2 * B)), ok, outs2) == S.E_INVALID and b"pairs[0]: " in L.sfm_last_error()
    assert many(one, 1, ins2, ok, (S.AdjustOut * 1)(S.AdjustOut(3 * B, 4 * B, 4 * B, None, 7 * B))) == S.E_INVALID and b"pairs[0]: out.d_points overlaps out.d_views" in L.sfm_last_error()
    for kw in (dict(used2=8 * B), dict(poses=8 * B), dict(used2=8 * B, poses=9 * B)):
        assert many(one, 1, ins2, S.adjust_params(**kw), outs2) == S.E_INVALID, kw
        assert many(None, 0, None, S.adjust_params(**kw), None) == S.E_INVALID, kw


def usage_of(path):
    """kernel name -> {field: int} from the compiler's resource-usage remarks."""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_kernels_use_no_scratch_and_the_batched_ones_have_their_twins_registers():
    path = os.path.join(ROOT, "build", "adjust.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it next to build/adjust.o"
    u = usage_of(path)
    kern = {k: v for k, v in u.items() if "adjust_" in k and "kernel" in k}
    assert len(kern) == 6, sorted(kern)
    for k, v in kern.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["AGPRs"] == 0, (k, v)
    find = lambda frag: next(v for k, v in kern.items() if frag in k)
    # the solve and scatter kernels: the same count as their twins.  The gather kernel: the single-pair one holds its argument's
    # fields in one more vector register than the batched one (46 against 45); both far below any occupancy step.
    assert find("adjust_solve_kernel")["VGPRs"] == find("adjust_solve_views_kernel")["VGPRs"] <= 256
    assert find("adjust_scatter_kernel")["VGPRs"] == find("adjust_scatter_views_kernel")["VGPRs"]
    assert 0 <= find("adjust_gather_kernel")["VGPRs"] - find("adjust_gather_views_kernel")["VGPRs"] <= 1
    assert find("adjust_gather_kernel")["VGPRs"] <= 64
    assert find("adjust_solve_kernel")["LDS Size"] == find("adjust_solve_views_kernel")["LDS Size"] <= 8192
