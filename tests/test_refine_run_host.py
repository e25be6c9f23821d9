"""CPU: sfm_refine_two_view without a device -- the host build of the whole call (rc_run of tests/hostcheck/librefinecheck.so: the
three kernel bodies of csrc/refine.hip through refine_math.hpp's functions and LmControl, the fp64 sums in the block's own order)
over the cases of tests/refine_scene.py: the block sum's order against the butterfly written out lane by lane, the conditions the
cases were designed for, the start against the oracle's SFM_POSE_CORRECT chain bit for bit, the degenerate rows, and the LM
against the fp64 twin (tests/refine_reference.py) at DESIGN 6b's bars; and the per-point tests of tests/test_refine_host.py -- the
Jacobians against central differences, the Schur terms against numpy -- run again, body and bars as they stand there, on cameras
with skew and fy != fx (there they run on the synthetic camera (fx, 0, fx)): refine_view's skew terms feed every LM stage."""
import ctypes as C

import numpy as np
import pytest

import cuda_sfm_amd as S
import oracle as O
from helpers import same_bits
import refine_reference as RR
import refine_scene as RS
import test_refine_host as TR
from test_adjust_host import ROT_BAR, T_BAR, RMS_BAR
from test_refine_host import L                       # the fixture of the per-point functions' ctypes signatures

SKEWED = [(35.0, 0.93), (-120.0, 0.93)]              # (skew, fy / fx)


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


@pytest.fixture(scope="module")
def runs(HL):
    """name -> (inputs of the case, its host run, the host run with max_iterations = 0), computed once."""
    out = {}
    for case in RS.CASES:
        c = RS.build_cpu(HL, S, case)
        args = (c["X0"], c["X1"], c["E"], c["sc"]["K"], c["mask"])
        out[case.name] = (c, RS.run_host(HL, S, *args, **case.kw), RS.run_host(HL, S, *args, **dict(case.kw, max_iterations=0)))
    return out


def test_block_sum_is_the_butterfly_and_the_wave_order(HL):
    """rc_sum512 against block_sum's shuffles written out: every lane of a wave adds the value of lane ^ off for off = 32 .. 1,
    lane 0's result is the wave's partial, and the eight partials are added in wave order.  The values span 40 binary orders of
    magnitude, so another order gives another double (the sequential sum does)."""
    rng = np.random.default_rng(5)
    differs = 0
    for _ in range(20):
        v = rng.standard_normal(512) * 2.0 ** rng.integers(-20, 20, 512)
        x = v.reshape(8, 64).copy()
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            x = x + x[:, lanes ^ off]
        want = x[0, 0]
        for w in range(1, 8):
            want = want + x[w, 0]
        got = HL.rc_sum512(np.ascontiguousarray(v).ctypes.data_as(C.c_void_p))
        assert got == want
        seq = 0.0
        for a in v:
            seq += a
        differs += seq != got
    assert differs > 0


def test_cases_are_what_the_table_says(runs):
    """The used count of every row, the last used record of the rows that end on a compaction round, the masked records that are
    not used, and between the cases: two pose indices, an odd and an even number of committed steps (the committed points in Xb,
    copied back, and in Xa), a rejected step and a failed solve."""
    for name, (c, r, _) in runs.items():
        case, rep = c["case"], r["report"]
        print(f"{name}: n={case.n} mask={int(c['mask'].sum())} m={rep['num_used']} pose_index={rep['pose_index']} status={rep['status']} "
              f"iterations={rep['iterations']} accepted={rep['accepted']} cur={r['trace'][0]} failed={r['trace'][1]} rejected={r['trace'][2]} "
              f"votes={r['trace'][4:].tolist()} rms {rep['initial_rms_px']:.4f} -> {rep['final_rms_px']:.4f}")
        assert r["used"].sum() == rep["num_used"] and not (r["used"].astype(bool) & (c["mask"] == 0)).any()
        assert r["trace"][0] == rep["accepted"] % 2 and rep["iterations"] == rep["accepted"] + r["trace"][1] + r["trace"][2]
        if name in RS.EXACT:
            assert rep["num_used"] == RS.EXACT[name]
        if case.mask != "own" and case.mask != "ones":
            assert rep["num_used"] == c["mask"].sum()                        # a caller mask of records the start uses: m is exact
        if name not in RS.DEGENERATE:
            assert rep["num_used"] >= 16 and rep["status"] != S.REFINE_DEGENERATE, name
    for name, last in (("last511", 511), ("last512", 512)):
        used = np.flatnonzero(runs[name][1]["used"])
        assert used[-1] == last and len(used) > 256
    assert runs["last511"][1]["report"]["num_used"] + 1 == runs["last512"][1]["report"]["num_used"]
    for name in ("unused", "unusedls"):
        c, r, _ = runs[name]
        spoiled = [*RS.UNUSED_NAN, RS.UNUSED_BEHIND]
        assert c["mask"].all() and not r["used"][spoiled].any() and c["sc"]["outlier"][r["used"].astype(bool)].any()
        assert np.isposinf(r["err"][list(RS.UNUSED_NAN)]).all()                  # a NaN pixel: no point, no error
        X = r["points"][:3, RS.UNUSED_BEHIND].astype(np.float64)
        assert np.isfinite(X).all() and (X[2] <= 0 or (r["pose"][:3, :3].astype(np.float64) @ X + r["pose"][:3, 3])[2] <= 0)
        assert np.isposinf(r["err"][RS.UNUSED_BEHIND])
    live = [v for k, v in runs.items() if k not in RS.DEGENERATE]
    assert {r["report"]["pose_index"] for _, r, _ in live} == {0, 1, 2, 3}     # every candidate wins somewhere
    assert any(r["trace"][0] == 1 and r["report"]["accepted"] > 0 for _, r, _ in live)
    assert any(r["trace"][0] == 0 and r["report"]["accepted"] > 0 for _, r, _ in live)
    assert any(r["trace"][2] > 0 for _, r, _ in live) and any(r["trace"][1] > 0 for _, r, _ in live)
    for cam in ("skew35", "skew-120", "skew35m0", "skew35m0b"):
        assert runs[cam][0]["sc"]["K"][0, 1] != 0 and runs[cam][0]["sc"]["K"][1, 1] != runs[cam][0]["sc"]["K"][0, 0]
    z = runs["genericz"][0]
    assert (np.abs(z["X0"][2] - 1) > 0.01).mean() > 0.9 and (np.abs(z["X1"][2] - 1) > 0.01).mean() > 0.9


def test_zero_iterations_return_the_dlt_start(runs):
    """max_iterations = 0: the pose is the voted SFM_POSE_CORRECT candidate of E and every point its DLT, bit for bit, as the
    oracle computes them; E = [t]x R of that pose; nothing was iterated."""
    for name, (c, _, r0) in runs.items():
        rep = r0["report"]
        assert (rep["iterations"], rep["accepted"]) == (0, 0) and same_bits([rep["initial_rms_px"]], [rep["final_rms_px"]])
        P = O.pose_candidates(c["E"], O.POSE_CORRECT)[rep["pose_index"]]
        assert same_bits(r0["pose"], P), name
        U0, U1 = RS.unit_z(c["X0"]), RS.unit_z(c["X1"])                     # the DLT runs on x / z, y / z (z = 1 but in genericz)
        pts = O.triangulate(U0, U1, P, 8)
        assert same_bits(r0["points"], pts), name
        votes = []                                                          # in front of both cameras, over the masked records
        for Q in O.pose_candidates(c["E"], O.POSE_CORRECT):
            Xq = O.triangulate(U0, U1, Q, 8).astype(np.float64)
            votes.append(int(((Xq[2] > 0) & (Q[2].astype(np.float64) @ Xq > 0) & (c["mask"] != 0)).sum()))
        assert votes == r0["trace"][4:].tolist() and rep["pose_index"] == int(np.argmax(votes)), (name, votes, r0["trace"][4:])
        t = P[:3, 3]
        Tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)
        assert np.allclose(r0["E"], Tx @ P[:3, :3].astype(np.float64), atol=1e-6)
        u = r0["used"].astype(bool)
        assert (r0["points"][2, u] > 0).all() and np.isfinite(r0["points"][:, u]).all()


def test_generic_z_points_give_what_the_same_rays_at_unit_z_give(HL, runs):
    """tests/golden/refine_generic_z_case.npz: the points and E of the genericz case, on which the start and the finish body, which
    triangulated on x, y as given while the residuals divided by z, took the DLT of other rays (rms 245 px at the start, 10.7 px
    after 20 iterations, four failed solves), and the mask the corrected start designs.  Every read of the points is x / z, y / z now, so the call
    depends on the rays alone: with the same E and mask the rays rescaled to z = 1 give every output bit for bit.  The bar is
    equality, by that argument; (x / z) / 1 is x / z exactly."""
    g = np.load(RS.GENERIC_Z_FIXTURE)
    c = runs["genericz"][0]
    for k in ("X0", "X1", "E", "mask"):                                     # the fixture is the case
        assert np.array_equal(g[k].view(np.uint8), np.ascontiguousarray(c[k]).view(np.uint8)), k
    assert (np.abs(g["X0"][2] - 1) > 0.01).mean() > 0.9
    for kw in (dict(), dict(max_iterations=0), dict(huber_px=0.0)):
        a = RS.run_host(HL, S, g["X0"], g["X1"], g["E"], g["K"], g["mask"], **kw)
        b = RS.run_host(HL, S, RS.unit_z(g["X0"]), RS.unit_z(g["X1"]), g["E"], g["K"], g["mask"], **kw)
        assert a["report"] == b["report"] and np.array_equal(a["used"], b["used"]) and np.array_equal(a["trace"], b["trace"])
        for k in ("pose", "E", "points", "err"):
            assert same_bits(a[k], b[k]), (kw, k)
        print("generic z", kw, a["report"], a["trace"].tolist())
    assert a["report"]["num_used"] == g["mask"].sum() and a["trace"][1] == 0


def test_degenerate_rows(runs):
    for name in RS.DEGENERATE:
        c, r, r0 = runs[name]
        rep = r["report"]
        assert rep["status"] == S.REFINE_DEGENERATE and rep["iterations"] == 0 and rep["accepted"] == 0
        assert np.isfinite(r["pose"]).all() and np.isfinite(r["E"]).all()
        assert r["used"].sum() == rep["num_used"] == RS.EXACT[name]
        assert same_bits(r["pose"], r0["pose"]) and same_bits(r["points"], r0["points"])
    assert runs["used16"][1]["report"]["status"] != S.REFINE_DEGENERATE and runs["used16"][1]["report"]["iterations"] > 0


def test_host_build_against_the_fp64_twin(runs):
    """The twin from the host build's own start, on every non-degenerate case with at least 257 used points (fewer make too flat a
    problem for a tolerance: those cases are for the byte comparison on the device): DESIGN 6b's bars."""
    checked = []
    for name, (c, r, r0) in runs.items():
        rep = r["report"]
        if rep["num_used"] < 257:
            continue
        kw = dict(dict(max_iterations=20, huber_px=1.0), **c["case"].kw)
        u = r0["used"].astype(bool)
        R0, t0 = r0["pose"][:3, :3].astype(np.float64), r0["pose"][:3, 3].astype(np.float64)
        ref = RR.refine(RS.cam_of(c["sc"]["K"]), R0, t0, r0["points"][:3, u].T.astype(np.float64), RS.obs_of(c["X0"], c["X1"])[u].astype(np.float64), **kw)
        X = r["points"][:3, u].T.astype(np.float64)
        fig = (RR.rotation_angle(r["pose"][:3, :3], ref["R"]), float(np.abs(r["pose"][:3, 3] - ref["t"]).max()),
               abs(rep["final_rms_px"] - ref["final_rms_px"]), abs(rep["initial_rms_px"] - ref["initial_rms_px"]),
               float(np.median(np.linalg.norm(X - ref["X"], axis=1) / ref["X"][:, 2])))
        print(f"{name}: m={rep['num_used']} host {rep['status']} {rep['iterations']}/{rep['accepted']} twin {ref['status']} {ref['iterations']}/{ref['accepted']} "
              f"rot {fig[0]:.2e} t {fig[1]:.2e} rms {fig[2]:.2e} / {fig[3]:.2e} points {fig[4]:.2e}")
        assert rep["status"] in (S.REFINE_CONVERGED, S.REFINE_MAX_ITER) and ref["status"] in (RR.CONVERGED, RR.MAX_ITER)
        assert rep["num_used"] == ref["num_used"]
        assert fig[0] <= ROT_BAR and fig[1] <= T_BAR and fig[2] <= RMS_BAR and fig[3] <= RMS_BAR, (name, fig)
        assert fig[4] < 1e-4, (name, fig)
        checked.append(name)
    assert len(checked) >= 8 and "skew-120" in checked, checked


@pytest.fixture
def skewed_scene_case(monkeypatch, camera):
    """test_refine_host.scene_case on a skewed camera: the same scene (seed, motion, noise) seen through K = (fx, s | 0, fy)."""
    plain = TR.scene_case

    def scene_case(n=64, seed=3):
        sc, _, _, R, t, X = plain(n, seed)
        K, Kinv = RS.camera(*camera)
        sk = RS.two_view_variant(n, seed, K, Kinv, sc["R"], sc["t"], noise_px=0.5, outlier_frac=0.0)
        X0, X1 = synth_normalized(sk)
        obs = np.stack([X0[0] / X0[2], X0[1] / X0[2], X1[0] / X1[2], X1[1] / X1[2]], 1).astype(np.float32)
        cam = np.array([K[0, 0], K[0, 1], K[1, 1]], np.float32)
        assert cam[1] == np.float32(camera[0]) and cam[2] == np.float32(camera[1] * 2360.0)
        calls.append(camera)
        return sk, cam, obs, R, t, X

    calls = []
    monkeypatch.setattr(TR, "scene_case", scene_case)
    yield calls
    assert calls, "test_refine_host's test no longer builds its inputs through scene_case: the camera was not the skewed one"


def synth_normalized(sc):
    from cuda_sfm_amd_synth import synth
    return synth.normalized_points(sc)


@pytest.mark.parametrize("camera", SKEWED, ids=["skew35", "skew-120"])
def test_jacobians_match_central_differences_on_skewed_cameras(L, camera, skewed_scene_case):
    TR.test_jacobians_match_central_differences(L)


@pytest.mark.parametrize("camera", SKEWED, ids=["skew35", "skew-120"])
@pytest.mark.parametrize("huber", [0.0, 1.0, 0.2])
def test_schur_terms_match_numpy_on_skewed_cameras(L, huber, camera, skewed_scene_case):
    TR.test_schur_terms_match_numpy(L, huber)
