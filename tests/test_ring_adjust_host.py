"""CPU: the arithmetic of sfm_adjust_ring (csrc/ring_adjust_math.hpp) through its host build (tests/hostcheck/
libringadjustcheck.so) against the fp64 twin (tests/ring_adjust_reference.py): the documents, the band claim of DESIGN 6l on the
twin's dense reduced system, the host build's reduction, factor and solve against numpy, one seam track's and one full-cycle
track's terms against the dense Schur complement, the twin and the host build on an exact ring and on the noisy rings of
fuse_ring_scene.RINGS, the gain from the loop, the decisions (k = 3, over-long tracks, NaN columns, degenerate and not-CLOSED
rings), and the no-scratch pin of ring_adjust.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cuda_sfm_amd as S
import chain_adjust_reference as CR
import chain_adjust_scene as CS
import fuse_ring_scene as FRS
import ring_adjust_reference as RR
import ring_adjust_scene as RAS

FIXED, ROOTK, FREE = 0, 1, 2
vp = lambda a: a.ctypes.data_as(C.c_void_p)
# 6i measured a largest relative residual |A x - b| / (|A| |x| + |b|) of 2.75e-16 on its banded systems.  The folded systems of the
# seven (ring, W) cases below, measured the same way on the host build's first system (damping 1e-3): the largest is 3.25e-17
# ((70, 65, 3) at W = 16); the bar is 4 x that.
FOLDED_MEASURED = 3.25e-17
# host build against the twin: 6i's six-view pair of bars
BAR_ROT, BAR_T, BAR_RMS = 1e-4, 1e-3, 1e-4
BAND_CASES = [(6, 257, 7, 3), (6, 257, 7, 8), (6, 257, 7, 16), (36, 65, 3, 8), (36, 65, 3, 16), (70, 65, 3, 8), (70, 65, 3, 16)]
# the issue's table: used tracks, used seam tracks, over-long tracks, degenerate
TABLE = {(3, 257, 7, 8): (283, 31, 0, False), (4, 257, 7, 8): (303, 52, 0, False), (6, 257, 7, 8): (364, 86, 0, False),
         (6, 1024, 61, 8): (1406, 349, 0, False), (5, 65, 5, 8): (84, 17, 0, False), (36, 65, 3, 8): (337, 20, 85, False),
         (36, 65, 3, 16): (411, 40, 11, False), (70, 65, 3, 8): (604, 15, 164, False), (70, 65, 3, 16): (740, 35, None, False),
         (6, 257, 7, 3): (124, 6, 240, False), (36, 65, 3, 3): (172, 0, None, True), (5, 65, 5, 3): (32, 1, None, True)}


@pytest.fixture(scope="module")
def HL():
    return RAS.host_lib()


def arrays(ring, res, status=None):
    return RAS.fused_arrays(S, res, len(ring["pairs"]), sum(P["n"] for P in ring["pairs"]), status)


def start_state(ring, res, W):
    """The twin's used observations, start points and start cameras."""
    ob = RR.observations(ring["pairs"], ring["K"], res)
    R, t = RR.start_cameras(res)
    used, X = RR.used_tracks(res, ob, R, t, W)
    return ob[used[ob[:, 0].astype(int)]], X, R, t, used


# ---- documents -----------------------------------------------------------------------------------------------------------------
def test_header_exports_python_mirror_and_integration_agree(HL):
    hdr = open(os.path.join(CS.ROOT, "include", "sfm_amd.h")).read()
    doc = open(os.path.join(CS.ROOT, "INTEGRATION.md")).read()
    emap = open(os.path.join(CS.ROOT, "cuda-sfm_amd", "csrc", "exports.map")).read()
    assert "global: sfm_*;" in emap
    for name in ("sfm_adjust_ring_default_params", "sfm_adjust_ring"):
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
    assert "#define SFM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    for which, T in enumerate((S.AdjustRingParams, S.AdjustRingIn, S.AdjustRingReport, S.AdjustRingOut)):
        o = np.zeros(16, np.int64)
        n = HL.ring_adjust_layout(which, vp(o))
        assert n == len(T._fields_) and o[0] == C.sizeof(T), T
        assert [int(x) for x in o[1:n + 1]] == [getattr(T, f).offset for f, _ in T._fields_], T
        for f, _ in T._fields_:
            assert re.search(rf"\b{f.rstrip('_')}\b", hdr), f
    assert hdr.count("sfm_adjust_ring") >= 12 and "sfm_adjust_ring (below)" in hdr and "sfm_adjust_ring uses them" in hdr
    p = S.adjust_ring_params()
    assert (p.max_iterations, p.max_track_views, list(p.reserved)) == (10, 8, [0, 0, 0, 0])
    assert abs(p.huber_px - 1.0) < 1e-7 and abs(p.min_rel_decrease - 1e-6) < 1e-12 and abs(p.initial_lambda - 1e-3) < 1e-10
    with pytest.raises(TypeError):
        S.adjust_ring_params(no_such_field=1)
    for c, k in ((0, 5), (1, 5), (8, 5), (9, 5), (2 * 69 + 1, 70)):
        assert HL.ring_adjust_view(c, k) == RR.view_of(c, k)
    for nb in (2, 3, 5, 35, 69):
        assert [HL.ring_adjust_fold_block(HL.ring_adjust_fold_pos(b, nb), nb) for b in range(nb)] == list(range(nb))
        assert [HL.ring_adjust_fold_pos(b, nb) for b in range(nb)] == [RR.fold_pos(b, nb) for b in range(nb)]
        assert [HL.ring_adjust_fold_block(q, nb) for q in range(min(nb, 4))] == [0, nb - 1, 1, nb - 2][:min(nb, 4)]


# ---- the band claim ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,seed,W", BAND_CASES)
def test_band_claim_on_the_twins_dense_system(k, n, seed, W):
    """Every block of the twin's dense reduced system (no band assumed in its assembly) that is not exactly zero lies within
    min(2 W, k - 1) of the diagonal under the fold.  Where the unfolded matrix has a corner at all (k - 1 > W) some non-zero block
    lies in it, further than W - 1 blocks from the diagonal: the test cannot pass on a chain."""
    sc, ring, res = RAS.fused_ring(k, n, seed)
    uob, X, R, t, used = start_state(ring, res, W)
    Sd, b, U = RR.dense_system(uob, X, R, t, 1.0, 1e-3)
    inside, corner = RR.band_check(Sd, W)
    nb = k - 1
    far = max(abs(RR.fold_pos(P, nb) - RR.fold_pos(Q, nb)) for P in range(nb) for Q in range(nb) if Sd[6 * P:6 * P + 6, 6 * Q:6 * Q + 6].any())
    print(f"ring ({k}, {n}, {seed}) W = {W}: {int(used.sum())} used tracks, folded band {RR.band_width(W, nb)} of {nb} block diagonals, "
          f"farthest non-zero block {far} positions from the diagonal, corner {corner}")
    assert inside
    if nb > W:
        assert corner


# ---- reduction, factor and solve of the host build -----------------------------------------------------------------------------
def test_reduction_factor_and_solve_against_numpy(HL):
    worst = 0.0
    for k, n, seed, W in BAND_CASES:
        sc, ring, res = RAS.fused_ring(k, n, seed)
        A, b, x, info = RAS.first_system(HL, S, ring, arrays(ring, res), 1e-3, max_track_views=W)
        assert info[0] == 1 and info[1] == 1 and info[2] == RR.band_width(W, k - 1), info
        off = np.kron(1 - np.eye(k - 1), np.ones((6, 6))).astype(bool)
        assert np.array_equal(A[off], A.T[off])                         # the transposed reads of the reduction mirror exactly
        A = np.triu(A) + np.triu(A, 1).T                                # a diagonal block: its upper triangle is what the factor reads
        uob, X, R, t, used = start_state(ring, res, W)
        assert info[3] == used.sum()
        Sd, bd, U = RR.dense_system(uob, X, R, t, 1.0, 1e-3)
        scale = np.abs(U).max()
        assert np.allclose(A, Sd, rtol=1e-3, atol=2e-3 * scale), (k, W, np.abs(A - Sd).max(), scale)
        assert np.array_equal(A != 0, Sd != 0) or RR.band_check(A, W)[0]
        assert np.allclose(b, bd, rtol=1e-3, atol=2e-3 * np.abs(bd).max() + 1e-2)
        res_rel = np.abs(A @ x - b).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())
        want = np.linalg.solve(A, b)
        assert np.allclose(x, want, rtol=1e-6, atol=1e-9 * np.abs(want).max()), (k, W, np.abs(x - want).max())
        print(f"ring ({k}, {n}, {seed}) W = {W}: folded solve, relative residual {res_rel:.3g}, |x - numpy| {np.abs(x - want).max():.3g}")
        worst = max(worst, res_rel)
    print(f"folded solves: largest relative residual {worst:.3g}")
    assert worst <= 4.0 * FOLDED_MEASURED, worst


# ---- one track's terms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,h,count", [("seam track", 6, 4, 4), ("full-cycle track", 3, 0, 4), ("seam track headed in the last pair", 5, 4, 3)])
def test_one_tracks_terms_against_the_dense_schur_complement(HL, name, k, h, count):
    """A track headed in pair h whose local view v is ring view (h + v) mod k: view 0 in the middle (a seam track) or at both ends
    (the full-cycle track).  6i's rtol 1e-3 and atol 2e-3 of the largest U entry; blocks against the fixed view exactly zero."""
    W, lam, huber = 8, 1e-2, 1.0
    rng = np.random.default_rng(7 * k + h)
    K9 = np.array([1000.0, 2.0, 320.0, 0.0, 990.0, 240.0, 0.0, 0.0, 1.0], np.float32)
    X = np.array([0.3, -0.2, 6.0], np.float32)
    views = [(h + v) % k for v in range(count)]
    HC = CS.host_lib()
    states, xy = np.zeros((count, 18), np.float32), np.zeros((count, 2), np.float32)
    Rk, tk = np.tile(np.eye(3), (k - 1, 1, 1)), np.zeros((k - 1, 3))
    for v, view in enumerate(views):
        if view == 0:
            Rv, tv = np.eye(3), np.zeros(3)
        else:
            Rv, tv = CR.expso3(rng.normal(0, 0.05, 3)), np.array([0.3 * view, 0.02, -0.01]) + rng.normal(0, 0.02, 3)
            if view == 1:
                tv /= np.linalg.norm(tv)
            s = np.zeros(18, np.float32)
            HC.chain_adjust_start_state(ROOTK if view == 1 else FREE, vp(np.concatenate([Rv.ravel(), tv]).astype(np.float32)), vp(s))
            states[v] = s
            Rv, tv = s[:9].reshape(3, 3).astype(np.float64), s[9:12].astype(np.float64)
            Rk[view - 1], tk[view - 1] = Rv, tv
        Y = Rv @ X + tv
        xy[v] = Y[:2] / Y[2] + rng.normal(0, 1.5e-3, 2)
    part = np.zeros(HC.chain_adjust_part_values(W))
    HL.ring_adjust_track_terms(count, h, k, W, vp(np.tile(K9, count)), vp(states), vp(xy), vp(X), huber, lam, vp(part))
    ob = np.array([[0, 0, view - 1, xy[v, 0], xy[v, 1], 1000.0, 2.0, 990.0] for v, view in enumerate(views)], np.float64)
    i1 = views.index(1) if 1 in views else None
    basis = (states[i1][12:15].astype(np.float64), states[i1][15:18].astype(np.float64)) if i1 is not None else CR.tangent_basis(np.array([1.0, 0, 0]))
    r, Jp, Jc, w, rho, _ = CR.terms(ob, X[None].astype(np.float64), Rk, tk, basis, huber, 0)
    V = sum(w[m] * Jp[m].T @ Jp[m] for m in range(count))
    gp = sum(w[m] * Jp[m].T @ r[m] for m in range(count))
    Vi = np.linalg.inv(V + lam * np.diag(np.diag(V)))
    Wm = [w[m] * Jc[m].T @ Jp[m] for m in range(count)]
    scale = max(np.abs(w[m] * Jc[m].T @ Jc[m]).max() for m in range(count))
    b0, u0 = 36 * (W * (W + 1) // 2), 36 * (W * (W + 1) // 2) + 6 * W
    fixed = [v for v, view in enumerate(views) if view == 0]
    assert len(fixed) == (2 if name.startswith("full") else 1)
    for a in range(W):
        for b in range(a, W):
            got = part[HC.chain_adjust_part_block(W, a, b):][:36].reshape(6, 6)
            if a in fixed or b in fixed or b >= count:
                assert not got.any(), (a, b)                          # exactly zero: the fixed view, and what the track does not span
                continue
            want = (w[a] * Jc[a].T @ Jc[a] if a == b else 0.0) - Wm[a] @ Vi @ Wm[b].T
            assert np.allclose(got, want, rtol=1e-3, atol=2e-3 * scale), (a, b, np.abs(got - want).max(), scale)
        gb, gu = part[b0 + 6 * a:b0 + 6 * a + 6], part[u0 + 6 * a:u0 + 6 * a + 6]
        if a in fixed or a >= count:
            assert not gb.any() and not gu.any()
            continue
        wb = w[a] * Jc[a].T @ r[a] - Wm[a] @ Vi @ gp
        assert np.allclose(gb, wb, rtol=1e-3, atol=2e-3 * np.abs(wb).max() + 1e-2), (a, gb, wb)
        assert np.allclose(gu, np.diag(w[a] * Jc[a].T @ Jc[a]), rtol=1e-4, atol=1e-6 * scale), a
    # the reduction carries the local block (a, b) to the global block pair both ways round, transposed the other way
    parts = np.zeros((k, len(part))); parts[h] = part
    out, outT = np.zeros(36), np.zeros(36)
    free = [v for v in range(count) if v not in fixed]
    for a in free:
        for b in free:
            HL.ring_adjust_reduce_block(vp(parts), W, k, views[a] - 1, views[b] - 1, vp(out))
            HL.ring_adjust_reduce_block(vp(parts), W, k, views[b] - 1, views[a] - 1, vp(outT))
            lo, hi = min(a, b), max(a, b)
            blk = part[HC.chain_adjust_part_block(W, lo, hi):][:36].reshape(6, 6)
            assert np.array_equal(out.reshape(6, 6), blk if a <= b else blk.T), (a, b)
            assert a == b or np.array_equal(outT.reshape(6, 6), out.reshape(6, 6).T), (a, b)      # (a diagonal block is kept as it was formed)


# ---- the twin and the host build on rings --------------------------------------------------------------------------------------
def true_cameras(sc):
    """View v >= 1 of the ring as (R, t) in pair 0's gauge: view 0's frame divided by pair 0's baseline."""
    R0, C0, b0 = sc["R"][0], sc["C"][0], sc["baseline"][0]
    return [(sc["R"][v] @ R0.T, sc["R"][v] @ (C0 - sc["C"][v]) / b0) for v in range(1, sc["k"])]


def camera_errors(cams, truth):
    """Per view v >= 1 (camera 2 of pair v - 1): rotation (rad) and t error per unit of |t|."""
    return [(CS.rotation_angle(cams[p, 1, :9], R), float(np.abs(cams[p, 1, 9:] - t).max() / max(1.0, np.linalg.norm(t)))) for p, (R, t) in enumerate(truth)]


def test_exact_ring_twin_and_host_build(HL):
    """6k's exact ring (6 x 512, no noise, no wrong matches, a fifth of every link's matches dropped), the start cameras turned 2e-3
    rad and t 1 % off.  The twin on exact float64 observations: 6i's exact bars (1e-9, 1e-4 px); the host build on the scene's
    float32 observations: 6i's host-build bars (1e-4 rad, 1e-3 in t per unit of |t|, 1e-3 px)."""
    k = 6
    sc, ring = FRS.build(k, 512, 11, noise_px=0.0, wrong_match=0.0, wrong_index=0.0)
    rng = np.random.default_rng(11)
    for L in ring["links"]:
        L["inlier"][rng.random(len(L["inlier"])) < 0.2] = 0
    res = FRS.run_host(FRS.host_lib(), S, ring)
    assert res["report"]["status"] == RR.CLOSED and res["report"]["seam_refined"] >= 100
    truth = true_cameras(sc)
    views = [(np.eye(3), np.zeros(3))] + truth
    pairs = []
    for q, P in enumerate(ring["pairs"]):
        Pw = (sc["P"][sc["perm"][q][:P["n"]]] - sc["C"][0]) @ sc["R"][0].T / sc["baseline"][0]
        cols = []
        for Rv, tv in (views[q], views[(q + 1) % k]):
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
    out = RR.adjust_ring(pairs, ring["K"], start, max_iterations=100, min_rel_decrease=1e-12)
    rep = out["report"]
    errs = camera_errors(out["cams"], truth)
    print("exact ring:", rep, errs)
    assert rep["num_cameras"] == 5 and rep["status"] != RR.DEGENERATE and rep["num_tracks"] > 400 and rep["num_seam_tracks"] >= 100
    assert max(e[0] for e in errs) < 1e-9 and max(e[1] for e in errs) < 1e-9
    assert rep["final_rms_px"] < 1e-4 and rep["initial_rms_px"] > 1.0
    hstart = dict(res, cams=start["cams"].astype(np.float32))
    host = RAS.run_host(HL, S, ring, arrays(ring, hstart), max_iterations=50, min_rel_decrease=1e-12)
    herrs = camera_errors(host["cams"].astype(np.float64), truth)
    hrep = host["report"]
    print("exact ring, host build:", hrep, herrs)
    assert host["band"] and hrep["num_tracks"] == rep["num_tracks"] and hrep["num_seam_tracks"] == rep["num_seam_tracks"] and hrep["initial_rms_px"] > 1.0
    assert max(e[0] for e in herrs) <= BAR_ROT and max(e[1] for e in herrs) <= BAR_T and hrep["final_rms_px"] < 1e-3


def compare(ring, host, twin, what, bars=True):
    """Used flags, counts and the degenerate decision equal; cameras, points and rms within 6i's six-view pair (bars: on the rings
    the pair was set for; elsewhere the differences are printed); the rms falls in the host build where it falls in the twin."""
    k = len(ring["pairs"])
    rt, rh = twin["report"], host["report"]
    assert host["band"] and twin["band"] is not False
    assert np.array_equal(host["used"] != 0, twin["used"]), what
    for f in ("ring_status", "num_cameras", "num_tracks", "num_seam_tracks", "num_observations", "num_over_long"):
        assert rh[f] == rt[f], (what, f, rh[f], rt[f])
    assert (rh["status"] == RR.DEGENERATE) == (rt["status"] == RR.DEGENERATE), what
    cams = host["cams"].astype(np.float64)
    drot = max(CS.rotation_angle(cams[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(k - 1))
    dt = max(float(np.abs(cams[p, 1, 9:] - twin["cams"][p, 1, 9:]).max() / max(1.0, np.linalg.norm(twin["cams"][p, 1, 9:]))) for p in range(k - 1))
    drms = abs(float(rh["final_rms_px"]) - rt["final_rms_px"])
    u = twin["used"]
    dpts = float((np.abs(host["points"][:3, u] - twin["points"][:3, u]).max(0) / np.abs(twin["points"][2, u])).max()) if u.any() else 0.0
    print(f"ring {what}: rms {rt['initial_rms_px']:.4f} -> {rt['final_rms_px']:.4f} px (host build {rh['initial_rms_px']:.4f} -> {rh['final_rms_px']:.4f}), "
          f"{rt['num_tracks']} tracks, {rt['num_seam_tracks']} seam; accepts twin {twin['accepts']}, host build "
          f"{[int(x) for x in host['accepts'][:rh['iterations']]]}; host - twin: rot {drot:.3g} rad, t / |t| {dt:.3g}, points {dpts:.3g}, rms {drms:.3g} px")
    assert not bars or (drot <= BAR_ROT and dt <= BAR_T and drms <= BAR_RMS), what
    if rt["status"] != RR.DEGENERATE and rt["final_rms_px"] < rt["initial_rms_px"]:
        assert rh["final_rms_px"] < rh["initial_rms_px"], what
    # one camera per view
    for p in range(k - 1):
        assert host["cams"][p + 1, 0].tobytes() == host["cams"][p, 1].tobytes()
    assert host["cams"][k - 1, 1].tobytes() == host["cams"][0, 0].tobytes() == np.asarray(host["cams"][0, 0]).tobytes()


@pytest.mark.parametrize("key", FRS.RINGS)
def test_noisy_rings_twin_and_host_build(HL, key):
    sc, ring, res = RAS.fused_ring(*key)
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res)
    host = RAS.run_host(HL, S, ring, arrays(ring, res))
    compare(ring, host, twin, key)
    tracks, seam, over, deg = TABLE[key + (8,)]
    assert (twin["report"]["num_tracks"], twin["report"]["num_seam_tracks"], twin["report"]["num_over_long"]) == (tracks, seam, over)
    # (the rms need not fall where the Huber cost does: on (6, 1024, 61) the twin's rises from 0.4314 to 0.4328 px; compare() holds
    # the host build to a falling rms only where the twin's falls)
    assert twin["report"]["status"] != RR.DEGENERATE and twin["report"]["accepted"] > 0
    assert host["cams"][0, 0].tobytes() == np.asarray(res["cams"], np.float32)[0, 0].tobytes()


@pytest.mark.parametrize("key", [(36, 65, 3, 16), (70, 65, 3, 8), (70, 65, 3, 16), (6, 257, 7, 3)])
def test_the_tables_other_rows(HL, key):
    sc, ring, res = RAS.fused_ring(*key[:3])
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res, max_track_views=key[3])
    host = RAS.run_host(HL, S, ring, arrays(ring, res), max_track_views=key[3])
    compare(ring, host, twin, key, bars=False)                        # the issue's table: counts and decisions
    tracks, seam, over, deg = TABLE[key]
    assert (twin["report"]["num_tracks"], twin["report"]["num_seam_tracks"]) == (tracks, seam) and twin["report"]["status"] != RR.DEGENERATE
    assert over is None or twin["report"]["num_over_long"] == over


@pytest.mark.parametrize("key", [(6, 257, 7), (6, 1024, 61), (36, 65, 3)])
def test_gain_from_the_loop(HL, key):
    """Measured in the twin first: how far sfm_adjust_chain leaves view 0's second copy (pair k - 1's camera 2) from [I|0], and
    the seam tracks' median distance to the truth before and after adjust_ring.  These rings start at the truth, so the twin may
    show no gain (6i found exactly that); the host build is held to 1.25 x the twin only where the twin improves."""
    k = key[0]
    sc, ring, res = RAS.fused_ring(*key)
    chain = CR.adjust_chain(ring["pairs"], ring["K"], res)
    copy = chain["cams"][k - 1, 1]
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res)
    host = RAS.run_host(HL, S, ring, arrays(ring, res))
    seam = np.flatnonzero(twin["used"] & (np.asarray(res["flags"]) == RR.SEAM_REFINED))
    feats = [FRS.feature(sc, res["obs_cam"][res["track_offset"][t]] >> 1, res["obs_record"][res["track_offset"][t]]) for t in seam]
    clean = np.array([all(FRS.feature(sc, res["obs_cam"][o] >> 1, res["obs_record"][o]) == f
                          for o in range(res["track_offset"][t], res["track_offset"][t + 1] - 1)) for t, f in zip(seam, feats)], bool)
    truth = FRS.truth_in_pair0(sc, feats)
    dist = lambda pts: float(np.median(np.linalg.norm(np.asarray(pts, np.float64)[:3, seam].T - truth, axis=1)[clean]))
    before, after_t, after_h = dist(res["points"]), dist(twin["points"]), dist(host["points"])
    print(f"ring {key}: adjust_chain leaves view 0's second copy {CS.rotation_angle(copy[:9], np.eye(3)):.3g} rad and {np.abs(copy[9:]).max():.3g} "
          f"from [I|0]; {int(clean.sum())} clean seam tracks, median distance to the truth {before:.4g} -> twin {after_t:.4g}, host build {after_h:.4g}" +
          ("" if after_t < before else "   (the twin shows no gain: nothing asserted)"))
    assert clean.sum() >= 8
    if after_t < before:
        assert after_h <= 1.25 * after_t


# ---- decisions -----------------------------------------------------------------------------------------------------------------
def test_decisions_equal_the_twins(HL):
    # k = 3: two blocks, the band is the whole matrix
    sc, ring, res = RAS.fused_ring(3, 257, 7)
    A, b, x, info = RAS.first_system(HL, S, ring, arrays(ring, res), 1e-3)
    assert info[2] == 2 and A.shape == (12, 12) and A[:6, 6:].any()
    # a track of W + 1 views is unused and counted; a seam track with a NaN column is unused
    sc, ring, res = RAS.fused_ring(6, 257, 7)
    lens = np.diff(res["track_offset"])
    longest = int(lens.max())
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res, max_track_views=longest - 1)
    host = RAS.run_host(HL, S, ring, arrays(ring, res), max_track_views=longest - 1)
    compare(ring, host, twin, "W = longest - 1")
    over = int((lens == longest).sum())
    assert over > 0 and host["report"]["num_over_long"] == over and not host["used"][lens == longest].any()
    full = RR.adjust_ring(ring["pairs"], ring["K"], res, max_iterations=0)
    victim = int(np.flatnonzero(full["used"] & (np.asarray(res["flags"]) == RR.SEAM_REFINED))[3])
    bad = dict(res, points=res["points"].copy())
    bad["points"][1, victim] = np.nan
    twin = RR.adjust_ring(ring["pairs"], ring["K"], bad)
    host = RAS.run_host(HL, S, ring, arrays(ring, bad))
    compare(ring, host, twin, "a NaN column")
    assert not host["used"][victim] and np.isnan(host["points"][1, victim]) and np.isinf(host["err"][victim])
    assert host["report"]["num_seam_tracks"] == full["report"]["num_seam_tracks"] - 1
    blocks = [HL.ring_adjust_view(int(c), 6) - 1 for c in res["obs_cam"]]
    assert blocks == twin["blocks"].tolist()


@pytest.mark.parametrize("key", [(36, 65, 3, 3), (5, 65, 5, 3)])
def test_degenerate_rings_return_every_input_bit(HL, key):
    sc, ring, res = RAS.fused_ring(*key[:3])
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res, max_track_views=key[3])
    host = RAS.run_host(HL, S, ring, arrays(ring, res), max_track_views=key[3])
    tracks, seam, over, deg = TABLE[key]
    assert twin["report"]["status"] == RR.DEGENERATE == host["report"]["status"] and host["report"]["iterations"] == 0
    assert (host["report"]["num_tracks"], host["report"]["num_seam_tracks"]) == (tracks, seam) == (twin["report"]["num_tracks"], twin["report"]["num_seam_tracks"])
    assert np.array_equal(host["used"] != 0, twin["used"])
    assert host["cams"].tobytes() == np.asarray(res["cams"], np.float32).tobytes()
    assert host["points"].tobytes() == np.asarray(res["points"], np.float32).tobytes()
    if key == (5, 65, 5, 3):
        assert twin["blockobs"][0] == 12                                # view 1 has 12 < 16


@pytest.mark.parametrize("status", [1, 2])
def test_not_closed_reports_return_every_input_bit(HL, status):
    sc, ring, res = RAS.fused_ring(5, 65, 5)
    twin = RR.adjust_ring(ring["pairs"], ring["K"], res, ring_status=status)
    host = RAS.run_host(HL, S, ring, arrays(ring, res, status))
    rep = host["report"]
    assert rep["ring_status"] == status and all(rep[f] == 0 for f in rep.dtype.names if f != "ring_status")
    assert not host["used"].any() and not twin["used"].any()
    assert host["cams"].tobytes() == np.asarray(res["cams"], np.float32).tobytes()
    assert host["points"].tobytes() == np.asarray(res["points"], np.float32).tobytes()
    fin = np.isfinite(twin["err"])
    assert np.array_equal(np.isfinite(host["err"]), fin) and np.abs(host["err"][fin] - twin["err"][fin]).max() <= 1e-2


def test_kernels_use_no_scratch():
    """The compiler's resource report of ring_adjust.hip (build/ring_adjust.usage.txt, written by the Makefile's object rule): no
    kernel uses scratch."""
    path = os.path.join(CS.ROOT, "build", "ring_adjust.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    kernels = ("ring_init_kernel", "ring_used_kernel", "ring_cost_kernel", "ring_open_kernel", "ring_system_kernel", "ring_solve_kernel",
               "ring_accept_kernel", "ring_finish_kernel")
    assert len(names) == len(scratch) == len(vgprs) == len(kernels)
    for name, kernel, sc, v in zip(names, kernels, scratch, vgprs):
        assert kernel in name and sc == 0 and v <= 256, (name, sc, v)
    print({k: v for k, v in zip(kernels, vgprs)})
