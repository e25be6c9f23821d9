"""CPU: the arithmetic of sfm_adjust_chain (csrc/chain_adjust_math.hpp) through its host build (tests/hostcheck/
libchainadjustcheck.so) against the fp64 twin (tests/chain_adjust_reference.py): Jacobians against central differences, one
track's terms against the dense Schur complement, the banded factor and solve against numpy, the twin on an exact and on noisy
chains, the host build against the twin, the used flags, block indices and degenerate decisions, and the documents."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cuda_sfm_amd as S
import chain_adjust_reference as CR
import chain_adjust_scene as CS
import fuse_scene as FS

FIXED, ROOTK, FREE = 0, 1, 2
vp = lambda a: a.ctypes.data_as(C.c_void_p)
# Banded factor and solve against numpy.linalg.solve on random SPD block-banded systems (1, 2, 7, 70 blocks x W = 2, 3, 8): the
# largest relative residual |A x - b| / (|A| |x| + |b|) MEASURED over the twelve systems is 2.75e-16; the bar is 4 x that.
BAND_MEASURED = 2.75e-16
# Host build against the twin over the noisy six-view chains (257, 7) and (1024, 61) at 10 iterations, per camera and per
# track.  MEASURED: rotation 1.1e-7 / 2.9e-5 rad, t 2.0e-6 / 1.5e-4 (the root pair's baseline is the unit), points
# 4.2e-6 / 8.5e-5 of the depth, rms 5.0e-6 / 2.2e-6 px, track errors 1.1e-3 / 2.2e-3 px.  6b's bars for two views (2e-5 rad, 2e-5
# in t) hold on the first chain and not on the second, where the minimum is flat (the rms falls by 7e-4 px) and the fp32 costs of
# the host build accept and reject other steps than the twin's: six views need the project's looser pair, 1e-4 rad and 1e-3 in t.
BAR_ROT, BAR_T, BAR_RMS = 1e-4, 1e-3, 1e-4


@pytest.fixture(scope="module")
def HL():
    return CS.host_lib()


@functools.lru_cache(maxsize=None)
def fused_scene(n, seed, exact=False):
    """(scene, chain, fuse's results by its host build) of a six-view chain."""
    kw = dict(noise_px=0.0, wrong_match=0.0, wrong_index=0.0) if exact else {}
    sc, ch = FS.build(n, seed, **kw)
    return sc, ch, FS.run_host(FS.host_lib(), S, ch)


def arrays(ch, res):
    return CS.fused_arrays(res, len(ch["pairs"]), sum(P["n"] for P in ch["pairs"]))


# ---- documents -----------------------------------------------------------------------------------------------------------------
def test_header_exports_python_mirror_and_integration_agree(HL):
    hdr = open(os.path.join(CS.ROOT, "include", "sfm_amd.h")).read()
    doc = open(os.path.join(CS.ROOT, "INTEGRATION.md")).read()
    emap = open(os.path.join(CS.ROOT, "cuda-sfm_amd", "csrc", "exports.map")).read()
    assert "global: sfm_*;" in emap
    for name in ("sfm_adjust_chain_default_params", "sfm_adjust_chain"):
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
    assert "#define SFM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    for which, T in enumerate((S.AdjustChainParams, S.AdjustChainIn, S.AdjustChainReport, S.AdjustChainOut)):
        o = np.zeros(16, np.int64)
        n = HL.chain_adjust_layout(which, vp(o))
        assert n == len(T._fields_) and o[0] == C.sizeof(T), T
        assert [int(x) for x in o[1:n + 1]] == [getattr(T, f).offset for f, _ in T._fields_], T
        for f, _ in T._fields_:
            assert re.search(rf"\b{f.rstrip('_')}\b", hdr), f
    p = S.adjust_chain_params()
    assert (p.max_iterations, p.max_track_views, list(p.reserved)) == (10, 8, [0, 0, 0, 0])
    assert abs(p.huber_px - 1.0) < 1e-7 and abs(p.min_rel_decrease - 1e-6) < 1e-12 and abs(p.initial_lambda - 1e-3) < 1e-10
    with pytest.raises(TypeError):
        S.adjust_chain_params(no_such_field=1)


# ---- Jacobians -----------------------------------------------------------------------------------------------------------------
def _state(HL, kind, R, t):
    s = np.zeros(18, np.float32)
    HL.chain_adjust_start_state(kind, vp(np.concatenate([R.ravel(), t]).astype(np.float32)), vp(s))
    return s


def _residual(HL, kind, K, s, x, y, X):
    r = np.zeros(2, np.float32)
    HL.chain_adjust_residual(kind, vp(K), vp(np.ascontiguousarray(s, np.float32)), x, y, vp(np.ascontiguousarray(X, np.float32)), vp(r))
    return r.astype(np.float64)


@pytest.mark.parametrize("kind", [FIXED, ROOTK, FREE])
def test_jacobians_match_central_differences(HL, kind):
    """6b's steps (1e-3 on the point, 1e-4 on the camera) and bar (1e-3 of the largest entry)."""
    rng = np.random.default_rng(3 + kind)
    K = np.array([1000.0, 2.0, 320.0, 0.0, 990.0, 240.0, 0.0, 0.0, 1.0], np.float32)
    for trial in range(8):
        R = CR.expso3(rng.normal(0, 0.1, 3))
        t = rng.normal(0, 0.5, 3)
        s = _state(HL, kind, R, t)
        if kind == ROOTK:
            assert abs(np.linalg.norm(s[9:12].astype(np.float64)) - 1.0) < 1e-6 and abs(s[12:15] @ s[9:12]) < 1e-6 and abs(s[15:18] @ s[12:15]) < 1e-6
        X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)], np.float32)
        x, y = float(X[0] / X[2] + rng.normal(0, 1e-3)), float(X[1] / X[2] + rng.normal(0, 1e-3))
        out = np.zeros(20, np.float32)
        HL.chain_adjust_jacobian(kind, vp(K), vp(s), x, y, vp(X), vp(out))
        r, Jp, Jc = out[:2], out[2:8].reshape(2, 3).astype(np.float64), out[8:].reshape(2, 6).astype(np.float64)
        assert np.abs(r - _residual(HL, kind, K, s, x, y, X)).max() <= 1e-3          # the same residual (the orders of two sums differ)
        for c in range(3):
            h = np.zeros(3); h[c] = 1e-3
            fd = (_residual(HL, kind, K, s, x, y, X + h) - _residual(HL, kind, K, s, x, y, X - h)) / 2e-3
            assert np.abs(fd - Jp[:, c]).max() <= 1e-3 * np.abs(Jp).max(), (kind, trial, c, fd, Jp[:, c])
        if kind == FIXED:
            assert not Jc.any()
            continue
        dof = 5 if kind == ROOTK else 6
        assert kind == FREE or not Jc[:, 5].any()
        for c in range(dof):
            fd = []
            for sign in (1.0, -1.0):
                dc = np.zeros(6); dc[c] = sign * 1e-4
                o = np.zeros(18, np.float32)
                HL.chain_adjust_camera_step(kind, vp(dc), vp(s), vp(o))
                fd.append(_residual(HL, kind, K, o, x, y, X))
            fd = (fd[0] - fd[1]) / 2e-4
            assert np.abs(fd - Jc[:, c]).max() <= 1e-3 * np.abs(Jc).max(), (kind, trial, c, fd, Jc[:, c])


# ---- one track's terms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("huber", [0.0, 1.0, 0.2])
@pytest.mark.parametrize("count", [2, 3, 8])
def test_one_tracks_terms_against_the_dense_schur_complement(HL, count, huber):
    """Views: the fixed camera, the 5-dof root block, then 6-dof blocks; 6b's rtol / atol; unspanned block pairs exactly zero."""
    W, lam = 8, 1e-2
    rng = np.random.default_rng(100 * count + int(10 * huber))
    K9 = np.array([1000.0, 2.0, 320.0, 0.0, 990.0, 240.0, 0.0, 0.0, 1.0], np.float32)
    X = np.array([0.3, -0.2, 6.0], np.float32)
    kinds = np.array([FIXED, ROOTK] + [FREE] * (count - 2), np.int32)
    states, xy = np.zeros((count, 18), np.float32), np.zeros((count, 2), np.float32)
    R, t = np.zeros((count, 3, 3)), np.zeros((count, 3))
    for v in range(count):
        Rv, tv = (np.eye(3), np.zeros(3)) if v == 0 else (CR.expso3(rng.normal(0, 0.05, 3)), np.array([0.3 * v, 0.02, -0.01]) + rng.normal(0, 0.02, 3))
        if v == 1:
            tv /= np.linalg.norm(tv)
        states[v] = _state(HL, int(kinds[v]), Rv, tv)
        R[v], t[v] = states[v][:9].reshape(3, 3), states[v][9:12]
        Y = R[v] @ X + t[v]
        xy[v] = Y[:2] / Y[2] + rng.normal(0, 1.5e-3, 2)           # about 1.5 px: some views above both Huber thresholds
    part = np.zeros(HL.chain_adjust_part_values(W))
    HL.chain_adjust_track_terms(count, 1, W, vp(kinds), vp(np.tile(K9, count)), vp(states), vp(xy), vp(X), huber, lam, vp(part))
    # the twin: blocks 0 .. count - 2 are views 1 .. count - 1
    ob = np.array([[0, 0, v - 1, xy[v, 0], xy[v, 1], 1000.0, 2.0, 990.0] for v in range(count)], np.float64)
    basis = (states[1][12:15].astype(np.float64), states[1][15:18].astype(np.float64))
    r, Jp, Jc, w, rho, _ = CR.terms(ob, X[None].astype(np.float64), R[1:], t[1:], basis, huber, 0)
    V = sum(w[m] * Jp[m].T @ Jp[m] for m in range(count))
    gp = sum(w[m] * Jp[m].T @ r[m] for m in range(count))
    Vi = np.linalg.inv(V + lam * np.diag(np.diag(V)))
    Wm = [w[m] * Jc[m].T @ Jp[m] for m in range(count)]
    scale = max(np.abs(w[m] * Jc[m].T @ Jc[m]).max() for m in range(1, count))
    b0, u0 = 36 * (W * (W + 1) // 2), 36 * (W * (W + 1) // 2) + 6 * W
    for a in range(W):
        for b in range(a, W):
            got = part[HL.chain_adjust_part_block(W, a, b):][:36].reshape(6, 6)
            if a == 0 or b >= count:
                assert not got.any(), (a, b)                      # exactly zero: the fixed camera, and what the track does not span
                continue
            want = (w[a] * Jc[a].T @ Jc[a] if a == b else 0.0) - Wm[a] @ Vi @ Wm[b].T
            assert np.allclose(got, want, rtol=1e-3, atol=2e-3 * scale), (a, b, np.abs(got - want).max(), scale)
        gb, gu = part[b0 + 6 * a:b0 + 6 * a + 6], part[u0 + 6 * a:u0 + 6 * a + 6]
        if a == 0 or a >= count:
            assert not gb.any() and not gu.any()
            continue
        wb = w[a] * Jc[a].T @ r[a] - Wm[a] @ Vi @ gp
        assert np.allclose(gb, wb, rtol=1e-3, atol=2e-3 * np.abs(wb).max() + 1e-2), (a, gb, wb)
        assert np.allclose(gu, np.diag(w[a] * Jc[a].T @ Jc[a]), rtol=1e-4, atol=1e-6 * scale), a


# ---- the banded factor and solve -----------------------------------------------------------------------------------------------
def _band_system(HL, rng, nb, W):
    """A random SPD block-banded matrix (dense, fp64), its band in the solver's layout and a right-hand side."""
    N = 6 * nb
    A = np.zeros((N, N))
    for p in range(nb):
        for q in range(p, min(nb, p + W)):
            A[6 * p:6 * p + 6, 6 * q:6 * q + 6] = rng.normal(0, 1, (6, 6))
    A = np.triu(A) + np.triu(A, 1).T
    A += np.eye(N) * (np.abs(A).sum(1).max() + 1.0)                # diagonally dominant: positive definite
    B = np.zeros(36 * W * nb)
    for j in range(N):
        for r in range(j, min(N, 6 * (j // 6 + W))):
            B[HL.chain_adjust_band_at(W, r, j)] = A[r, j]
    return A, B, rng.normal(0, 1, N)


def test_banded_factor_and_solve_against_numpy(HL):
    rng = np.random.default_rng(11)
    worst = 0.0
    for nb in (1, 2, 7, 70):
        for W in (2, 3, 8):
            A, B, b = _band_system(HL, rng, nb, W)
            x = b.copy()
            assert HL.chain_adjust_band_solve(vp(B), W, nb, vp(x)) == 1
            res = np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())
            assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12), (nb, W)
            worst = max(worst, res)
    print(f"banded solve: largest relative residual {worst:.3g}")
    assert worst <= 4.0 * BAND_MEASURED, worst
    A, B, b = _band_system(HL, rng, 7, 3)
    B[HL.chain_adjust_band_at(3, 20, 20)] = -1.0                   # not positive definite: reported, as refine_cholesky does
    assert HL.chain_adjust_band_solve(vp(B), 3, 7, vp(b)) == 0


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def camera_errors(cams, truth):
    """Per pair: rotation (rad) and t error of camera 2 against the truth in the root pair's gauge."""
    return [(CS.rotation_angle(cams[p, 1, :9], R), float(np.abs(cams[p, 1, 9:] - t).max())) for p, (R, t) in enumerate(truth)]


def test_twin_recovers_the_exact_chain():
    """Six views, n = 512, no noise, exact float64 observations; start cameras turned 2e-3 rad and t 1 % off: 6f's bars.  The host
    build runs on the same chain (its observations float32, so it is held to 6b's host-build bars against the truth, not to 1e-9)."""
    sc, ch, res = fused_scene(512, 5, exact=True)
    truth = CS.true_cameras(sc)
    b0 = sc["pairs"][0]["baseline"]
    views = [(np.eye(3), np.zeros(3))] + truth
    pairs = []
    for q, P in enumerate(ch["pairs"]):
        Pw = sc["P"][sc["perm"][q][:P["n"]]] / b0
        cols = []
        for Rv, tv in (views[q], views[q + 1]):
            Y = Pw @ Rv.T + tv
            X = np.ones((3, P["ld"])); X[:2, :P["n"]] = (Y[:, :2] / Y[:, 2:]).T
            cols.append(X)
        pairs.append(dict(P, X0=cols[0], X1=cols[1]))
    rng = np.random.default_rng(1)
    start = dict(res, cams=np.asarray(res["cams"], np.float64).copy())
    for p, (R, t) in enumerate(truth):
        w = rng.normal(0, 1, 3); w *= 2e-3 / np.linalg.norm(w)
        d = rng.normal(0, 1, 3); d *= 0.01 * np.linalg.norm(t) / np.linalg.norm(d)
        start["cams"][p, 1] = np.concatenate([(CR.expso3(w) @ R).ravel(), t + d])
    out = CR.adjust_chain(pairs, ch["K"], start, max_iterations=100, min_rel_decrease=1e-12)
    rep = out["reports"][0]
    assert rep["num_cameras"] == 5 and rep["status"] != CR.DEGENERATE and rep["num_tracks"] > 400
    errs = camera_errors(out["cams"], truth)
    print("exact chain:", rep, errs)
    assert max(e[0] for e in errs) < 1e-9 and max(e[1] for e in errs) < 1e-9
    assert rep["final_rms_px"] < 1e-4 and rep["initial_rms_px"] > 1.0
    # the host build from the same start on the scene's float32 observations: the host-build pair of bars against the truth; its rms
    # is what fp32 leaves of an exact fit: residuals formed from pixel-sized quantities (up to 360 px x 2^-24 = 2e-5 px per rounding,
    # some ten roundings per residual) -- 1e-3 px is fifty of them
    HL = CS.host_lib()
    hstart = dict(res, cams=start["cams"].astype(np.float32))
    host = CS.run_host(HL, S, ch, arrays(ch, hstart), max_iterations=50, min_rel_decrease=1e-12)
    herrs = camera_errors(host["cams"].astype(np.float64), truth)
    hrep = host["reports"][0]
    print("exact chain, host build:", hrep, herrs)
    assert hrep["num_tracks"] == rep["num_tracks"] and hrep["initial_rms_px"] > 1.0
    assert max(e[0] for e in herrs) <= BAR_ROT and max(e[1] for e in herrs) <= BAR_T and hrep["final_rms_px"] < 1e-3


@pytest.mark.parametrize("n,seed", [(257, 7), (1024, 61)])
def test_noisy_chains_twin_and_host_build(HL, n, seed):
    sc, ch, res = fused_scene(n, seed)
    truth = CS.true_cameras(sc)
    twin = CR.adjust_chain(ch["pairs"], ch["K"], res)
    host = CS.run_host(HL, S, ch, arrays(ch, res))
    rt, rh = twin["reports"][0], host["reports"][0]
    # the rms falls in every segment (one here)
    assert rt["final_rms_px"] < rt["initial_rms_px"] and rh["final_rms_px"] < rh["initial_rms_px"]
    # the counts; the accept sequences are printed, not compared: where the fp64 twin meets min_rel_decrease the fp32 costs of the host
    # build still fall by rounding, or the other way round (the device is held to the host build's sequence, tests/test_gpu_chain_adjust.py)
    for f in ("num_cameras", "num_tracks", "num_observations", "num_over_long"):
        assert rh[f] == rt[f], (f, rh[f], rt[f])
    assert rh["status"] != CR.DEGENERATE and rt["status"] != CR.DEGENERATE
    print(f"accepts: twin {twin['accepts'][0]}, host build {[int(x) for x in host['accepts'][0][:rh['iterations']]]}")
    assert np.array_equal(host["used"] != 0, twin["used"])
    # host build against the twin
    cams = host["cams"].astype(np.float64)
    drot = max(CS.rotation_angle(cams[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(5))
    dt = float(np.abs(cams[:, 1, 9:] - twin["cams"][:, 1, 9:]).max())
    u = twin["used"]
    dpts = float((np.abs(host["points"][:3, u] - twin["points"][:3, u]).max(0) / twin["points"][2, u]).max())
    drms = abs(float(rh["final_rms_px"]) - rt["final_rms_px"])
    fin = np.isfinite(twin["err"])
    assert np.array_equal(np.isfinite(host["err"]), fin)
    derr = float(np.abs(host["err"][fin] - twin["err"][fin]).max())
    print(f"chain ({n}, {seed}): rms {rt['initial_rms_px']:.4f} -> {rt['final_rms_px']:.4f} px, {rt['iterations']} iterations, {rt['accepted']} accepted; "
          f"host - twin: rot {drot:.3g} rad, t {dt:.3g}, points {dpts:.3g}, rms {drms:.3g} px, err {derr:.3g} px")
    assert drot <= BAR_ROT and dt <= BAR_T and drms <= BAR_RMS and derr <= 1e-2
    # against the truth, start -> twin (recorded in DESIGN 6i); the host build within 1.25 x the twin where the twin improves
    e0, et, eh = camera_errors(np.asarray(res["cams"], np.float64), truth), camera_errors(twin["cams"], truth), camera_errors(cams, truth)
    for p in range(5):
        print(f"  camera {p + 1}: rot {e0[p][0]:.3g} -> {et[p][0]:.3g} rad, t {e0[p][1]:.3g} -> {et[p][1]:.3g}" +
              ("" if et[p][0] < e0[p][0] and et[p][1] < e0[p][1] else "   (the twin does not improve both)"))
        for c in range(2):
            if et[p][c] < e0[p][c]:
                assert eh[p][c] <= 1.25 * et[p][c] + 1e-7, (p, c, eh[p][c], et[p][c])
    # the unification: camera 1 of pair p + 1 is the bytes of camera 2 of pair p
    for p in range(4):
        assert host["cams"][p + 1, 0].tobytes() == host["cams"][p, 1].tobytes()


def test_one_segment_of_70_cameras(HL):
    """chain_adjust_scene.strip: 70 cameras in ONE segment, 65 records per pair, tracks of 2 .. 8 views, the start cameras 1e-3 rad
    and 0.5 % off: the banded factor over 420 columns end to end, in the host build and (dense) in the twin.  The t bar is the six-view
    one per unit of |t|: a camera 70 baselines from the root moves by 70 x what a rotation difference moves one at 1."""
    ch, fused, truth = CS.strip()
    twin = CR.adjust_chain(ch["pairs"], ch["K"], fused)
    host = CS.run_host(HL, S, ch, CS.fused_arrays(fused, 70, 70 * 65))
    rt, rh = twin["reports"][0], host["reports"][0]
    assert np.array_equal(host["used"] != 0, twin["used"]) and twin["used"].all()
    for f in ("num_cameras", "num_tracks", "num_observations", "num_over_long"):
        assert rh[f] == rt[f], (f, rh[f], rt[f])
    assert rh["num_cameras"] == 70 and rh["status"] != CR.DEGENERATE and rt["status"] != CR.DEGENERATE
    assert rt["final_rms_px"] < 0.1 * rt["initial_rms_px"] and rh["final_rms_px"] < 0.1 * rh["initial_rms_px"]
    cams = host["cams"].astype(np.float64)
    drot = [CS.rotation_angle(cams[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(70)]
    dt = [float(np.abs(cams[p, 1, 9:] - twin["cams"][p, 1, 9:]).max() / max(1.0, np.linalg.norm(twin["cams"][p, 1, 9:]))) for p in range(70)]
    drms = abs(float(rh["final_rms_px"]) - rt["final_rms_px"])
    print(f"one segment of 70: rms {rt['initial_rms_px']:.4f} -> {rt['final_rms_px']:.4f} px; accepts twin {twin['accepts'][0]}, host build "
          f"{[int(x) for x in host['accepts'][0][:rh['iterations']]]}; host - twin: rot {max(drot):.3g} rad, t / |t| {max(dt):.3g}, "
          f"t {np.abs(cams[:, 1, 9:] - twin['cams'][:, 1, 9:]).max():.3g}, rms {drms:.3g} px")
    assert max(drot) <= BAR_ROT and max(dt) <= BAR_T and drms <= BAR_RMS
    for p in range(69):
        assert host["cams"][p + 1, 0].tobytes() == host["cams"][p, 1].tobytes()


def test_kernels_use_no_scratch():
    """The compiler's resource report of chain_adjust.hip (build/chain_adjust.usage.txt, written by the Makefile's object rule): no
    kernel uses scratch; the system kernel fits its 256 registers, the factor (solve) kernel is recorded in DESIGN 6i."""
    path = os.path.join(CS.ROOT, "build", "chain_adjust.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    kernels = ("chain_init_kernel", "chain_used_kernel", "chain_cost_kernel", "chain_open_kernel", "chain_system_kernel", "chain_solve_kernel",
               "chain_accept_kernel", "chain_finish_kernel")
    assert len(names) == len(scratch) == len(vgprs) == len(kernels)
    for name, kernel, sc, v in zip(names, kernels, scratch, vgprs):
        assert kernel in name and sc == 0 and v <= 256, (name, sc, v)
    print({k: v for k, v in zip(kernels, vgprs)})


# ---- used flags, block indices, degenerate decisions ---------------------------------------------------------------------------
def _decisions(HL, ch, res, **kw):
    twin = CR.adjust_chain(ch["pairs"], ch["K"], res, **kw)
    host = CS.run_host(HL, S, ch, arrays(ch, res), **kw)
    assert np.array_equal(host["used"] != 0, twin["used"])
    root = np.asarray(res["root"])
    assert np.array_equal(host["reports"]["root"], root)
    for p in range(len(root)):
        rep = host["reports"][p]
        if root[p] != p:
            assert all(rep[f] == 0 for f in rep.dtype.names if f != "root"), p
            continue
        for f in ("num_cameras", "num_tracks", "num_observations", "num_over_long"):
            assert rep[f] == twin["reports"][p][f], (p, f, rep[f], twin["reports"][p][f])
        assert (rep["status"] == CR.DEGENERATE) == (twin["reports"][p]["status"] == CR.DEGENERATE), p
    blocks = [HL.chain_adjust_block(int(c), int(root[c >> 1])) for c in res["obs_cam"]]
    assert blocks == twin["blocks"].tolist()
    return host, twin


def _only(res, keep):
    """The fused model with every track outside `keep` flagged KEPT (so not used)."""
    flags = np.full_like(res["flags"], 2)
    flags[list(keep)] = 1
    return dict(res, flags=flags)


def test_used_flags_blocks_and_degenerate_decisions_equal_the_twins(HL):
    sc, ch, res = fused_scene(257, 7)
    host, twin = _decisions(HL, ch, res)
    assert host["reports"][0]["status"] != CR.DEGENERATE and twin["used"].sum() > 300
    # a cut: two segments, each with a report of its own
    cut = dict(ch, links=[dict(L, status=S.REFINE_DEGENERATE) if i == 2 else L for i, L in enumerate(ch["links"])])
    rc = FS.run_host(FS.host_lib(), S, cut)
    assert rc["root"].tolist() == [0, 0, 0, 3, 3]
    host, twin = _decisions(HL, cut, rc)
    assert host["reports"][0]["num_cameras"] == 3 and host["reports"][3]["num_cameras"] == 2
    assert host["cams"][3, 0].tobytes() == np.asarray(rc["cams"], np.float32)[3, 0].tobytes()          # a root's camera 1: as it came in
    # a segment's bytes do not depend on the other segment: the first three pairs alone
    first = FS.head(ch, 3)
    alone = CS.run_host(HL, S, first, arrays(first, FS.run_host(FS.host_lib(), S, first)))
    assert alone["cams"].tobytes() == host["cams"][:3].tobytes() and alone["reports"][0] == host["reports"][0]
    # a one-pair chain
    one = FS.head(ch, 1)
    host, twin = _decisions(HL, one, FS.run_host(FS.host_lib(), S, one))
    assert host["reports"][0]["num_cameras"] == 1 and host["reports"][0]["final_rms_px"] < host["reports"][0]["initial_rms_px"]
    # two pairs: tracks of pair 0 alone give block 0 one observation, tracks over both pairs one to each block
    two = FS.head(ch, 2)
    r2 = FS.run_host(FS.host_lib(), S, two)
    lens, heads = np.diff(r2["track_offset"]), r2["obs_cam"][r2["track_offset"][:-1]] >> 1
    usable = CR.adjust_chain(two["pairs"], two["K"], r2, max_iterations=0)["used"]
    short = [t for t in np.flatnonzero(usable & (lens == 2) & (heads == 0))]
    long = [t for t in np.flatnonzero(usable & (lens == 3))]
    for n_short, n_long, degenerate in ((16, 5, True), (16, 6, False), (9, 6, True), (10, 6, False)):
        sub = _only(r2, short[:n_short] + long[:n_long])
        host, twin = _decisions(HL, two, sub)
        assert twin["blockobs"].tolist() == [n_short + n_long, n_long]
        assert (host["reports"][0]["status"] == CR.DEGENERATE) == degenerate, (n_short, n_long)
        if degenerate:                                             # cameras (both slots) and columns as they came in
            assert host["cams"].tobytes() == np.asarray(sub["cams"], np.float32).tobytes()
            assert host["points"].tobytes() == np.asarray(sub["points"], np.float32).tobytes()
            assert host["reports"][0]["iterations"] == 0
    # a track of W + 1 views is not used and counted; a NaN column is not used
    longest = int(np.diff(res["track_offset"]).max())
    host, twin = _decisions(HL, ch, res, max_track_views=longest - 1)
    over = int((np.diff(res["track_offset"]) == longest).sum())
    assert over > 0 and host["reports"][0]["num_over_long"] == over and not host["used"][np.diff(res["track_offset"]) == longest].any()
    bad = dict(res, points=res["points"].copy())
    victim = int(np.flatnonzero(twin["used"])[3])
    bad["points"][1, victim] = np.nan
    host, twin = _decisions(HL, ch, bad)
    assert not host["used"][victim] and np.isnan(host["points"][1, victim]) and np.isinf(host["err"][victim])
