"""CPU: the arithmetic of sfm_intersect_tracks (csrc/intersect_math.hpp) through its host build (tests/hostcheck/
libintersectcheck.so) against the fp64 twin (tests/intersect_reference.py): the documents, the hand-built tables of
intersect_scene (tracks of 2 .. 131 views, exact; NaN and behind-camera columns; views that share one centre), classes and counts on
the chains of fuse_scene.SCENES and the rings of fuse_ring_scene.RINGS after the host builds of sfm_adjust_chain / sfm_adjust_ring,
the host build against the twin on all of them, what the call buys on the two rings with over-long tracks, and the pins."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cuda_sfm_amd as S
import chain_adjust_scene as CS
import fuse_ring_scene as FRS
import fuse_scene as FS
import intersect_reference as IR
import intersect_scene as IS
import ring_adjust_reference as RR
import ring_adjust_scene as RAS

vp = lambda a: a.ctypes.data_as(C.c_void_p)
EXACT_BAR = 1e-4                                       # a point against the truth, relative to its depth (test_fuse_host's bar)
# Host build against the twin over every listed input (the two hand-built tables, SCENES and RINGS after their adjustment, with and
# without d_skip), on the tracks both start from the same candidate.  MEASURED: the largest difference of a point relative to its
# depth and of d_err in px (relative above 1 px, as test_fuse_host compares it), both on ring (6, 1024, 61) without d_skip; the bars
# are 4 x that.
MEASURED_POINT, MEASURED_ERR = 1.35e-5, 2.13e-2
BAR_POINT, BAR_ERR = 4.0 * MEASURED_POINT, 4.0 * MEASURED_ERR
# A start choice may flip where the two candidates' costs tie.  A pixel coordinate of up to ~400 px carried through fp32 cameras and
# observations is good to a few ulps of it, TIE_PX = 2e-4 px; a cost c = sum of m squared residuals r therefore to about 2 m r TIE_PX =
# 2 TIE_PX sqrt(m c), plus m TIE_PX^2.  Flipped tracks are listed with their tie's size and left out of the comparison; at most
# TIE_CAP of an input's tracks may flip.
TIE_PX, TIE_CAP = 2e-4, 0.01
REFINED_CLASS, KEPT_CLASS = (1, 3), (2, 4)


@pytest.fixture(scope="module")
def HL():
    return IS.host_lib()


@functools.lru_cache(maxsize=None)
def adjusted_chain(n, seed):
    """(chain, sfm_fuse_chain's table, sfm_adjust_chain's results), both by their host builds."""
    sc, ch = FS.build(n, seed)
    res = FS.run_host(FS.host_lib(), S, ch)
    k, N = len(ch["pairs"]), sum(P["n"] for P in ch["pairs"])
    return ch, res, CS.run_host(CS.host_lib(), S, ch, CS.fused_arrays(res, k, N))


@functools.lru_cache(maxsize=None)
def adjusted_ring(k, n, seed, W=8):
    """(ring, sfm_fuse_ring's table, sfm_adjust_ring's results), both by their host builds."""
    sc, ring, res = RAS.fused_ring(k, n, seed)
    N = sum(P["n"] for P in ring["pairs"])
    return ring, res, RAS.run_host(RAS.host_lib(), S, ring, RAS.fused_arrays(S, res, k, N), max_track_views=W)


def adjusted_inputs():
    for n, seed in FS.SCENES:
        yield (f"chain ({n}, {seed})",) + adjusted_chain(n, seed)
    for k, n, seed in FRS.RINGS:
        yield (f"ring ({k}, {n}, {seed})",) + adjusted_ring(k, n, seed)


def host(HL, chain, table, cams=None, points=None, skip=None, **kw):
    k, N = len(chain["pairs"]), sum(P["n"] for P in chain["pairs"])
    return IS.run_host(HL, S, chain, IS.table_arrays(table, k, N, cams=cams, points=points, skip=skip), **kw)


def check_counts(got, T):
    c = got["counts"]
    assert c["tracks"] == T and c["intersected"] + c["copied"] == T and c["refined"] + c["kept"] + c["no_start"] == c["intersected"], c
    assert c["from_linear"] == (got["start"] == IR.FROM_L).sum() and c["no_start"] == (got["start"] == IR.NONE).sum()
    assert c["copied"] == (got["start"] == IR.COPIED).sum()


# ---- documents -----------------------------------------------------------------------------------------------------------------
def test_header_exports_python_mirror_and_documents_agree(HL):
    read = lambda *p: open(os.path.join(IS.ROOT, *p)).read()
    hdr, doc, design, readme = read("include", "sfm_amd.h"), read("INTEGRATION.md"), read("DESIGN.md"), read("README.md")
    assert "global: sfm_*;" in read("cuda-sfm_amd", "csrc", "exports.map")
    for name in ("sfm_intersect_default_params", "sfm_intersect_tracks"):
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
    assert "#define SFM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    assert "sfm_intersect_tracks" in readme and "6m" in design and "sfm_intersect_tracks" in design
    for which, T in enumerate((S.IntersectParams, S.IntersectIn, S.IntersectOut)):
        o = np.zeros(16, np.int64)
        n = HL.intersect_layout(which, vp(o))
        assert n == len(T._fields_) and o[0] == C.sizeof(T), T
        assert [int(x) for x in o[1:n + 1]] == [getattr(T, f).offset for f, _ in T._fields_], T
        for f, _ in T._fields_:
            assert re.search(rf"\b{f}\b", hdr), f
    p = S.intersect_params()
    assert (p.max_iterations, p.wave_min_views, list(p.reserved)) == (5, 0, [0, 0, 0, 0]) and p.threshold_px == 4.0
    assert abs(p.huber_px - 1.0) < 1e-7 and abs(p.min_rel_decrease - 1e-6) < 1e-12 and abs(p.initial_lambda - 1e-3) < 1e-10
    f = S.fuse_params()                                                        # sfm_fuse_params' fields with the same defaults
    for name, _ in S.FuseParams._fields_:
        if name != "reserved":
            assert getattr(p, name) == getattr(f, name), name
    with pytest.raises(TypeError):
        S.intersect_params(no_such_field=1)
    assert HL.intersect_check_wave_min_views() == 32 and S.INTERSECT_COUNTS[5:] == ("from_linear", "no_start", "promoted")


def test_the_headers_pieces(HL):
    for flag in range(7):
        for count in (0, 1, 2, 5):
            for skip in (0, 1):
                assert HL.intersect_check_copied(flag, count, skip) == int(not 1 <= flag <= 4 or count < 2 or skip == 1)
    assert [HL.intersect_check_class(f, a) for f in (1, 2, 3, 4) for a in (1, 0)] == [1, 2, 1, 2, 3, 4, 3, 4]
    ch = HL.intersect_check_choose
    assert (ch(1, 2.0, 1, 1.0), ch(1, 1.0, 1, 1.0), ch(1, 1.0, 1, 2.0)) == (IR.FROM_L, IR.FROM_C, IR.FROM_C)       # C on a tie
    assert (ch(0, 0.0, 1, 9.0), ch(1, 9.0, 0, 0.0), ch(0, 0.0, 0, 0.0)) == (IR.FROM_L, IR.FROM_C, IR.NONE)
    # the linear intersection of exact rays is the point; rays from one centre have none
    rng = np.random.default_rng(3)
    X = np.array([0.3, -0.2, 6.0])
    Ps, xy = np.zeros((5, 12), np.float32), np.zeros((5, 2), np.float32)
    for v in range(5):
        R, t = IS.AS.rot_y(0.05 * v) @ IS.AS.rot_x(-0.03 * v), np.array([0.4 * v, 0.02 * v, 0.0])
        Ps[v] = np.concatenate([R.ravel(), t])
        Y = Ps[v, :9].reshape(3, 3).astype(np.float64) @ X + Ps[v, 9:]
        xy[v] = Y[:2] / Y[2]
    L = np.zeros(3, np.float32)
    assert HL.intersect_check_linear(5, vp(Ps), vp(xy), vp(L)) == 1 and np.abs(L - X).max() <= 1e-5 * X[2]
    assert HL.intersect_check_linear(2, vp(Ps), vp(xy), vp(L)) == 1 and np.abs(L - X).max() <= 1e-4 * X[2]
    Ps[:, 9:] = 0.0
    for v in range(5):
        Y = Ps[v, :9].reshape(3, 3).astype(np.float64) @ X
        xy[v] = Y[:2] / Y[2]
    assert HL.intersect_check_linear(5, vp(Ps), vp(xy), vp(L)) == 0 and np.isnan(L).all()


# ---- hand-built tables ---------------------------------------------------------------------------------------------------------
def test_hand_built_table_exact_observations(HL):
    ch, tb, truth, depth = IS.hand_built()
    lens = np.diff(tb["track_offset"])
    assert sorted(set(lens.tolist())) == list(IS.LENGTHS) and len(ch["pairs"]) == 130 and lens.max() == 131
    seam = tb["obs_cam"][tb["track_offset"][:-1]] >> 1 > tb["obs_cam"][tb["track_offset"][1:] - 1] >> 1      # first pair larger than last
    assert seam.sum() >= 8 and np.isin(tb["flags"][seam], (3, 4)).all()
    moved = IS.displaced(tb, truth, depth, 0.05)
    got = host(HL, ch, moved)
    check_counts(got, len(lens))
    d = np.linalg.norm(got["points"][:3].T.astype(np.float64) - truth, axis=1) / depth
    print(f"intersect hand-built, columns 5 % off: {got['counts']}, largest |X - truth| / depth {d.max():.3g}, largest err {got['err'].max():.3g} px")
    assert (got["flags"] == np.where(np.isin(tb["flags"], (3, 4)), 3, 1)).all() and (got["points"][3] == 1.0).all()
    assert d.max() <= EXACT_BAR and got["err"].max() < 0.01
    assert got["counts"]["refined"] == len(lens) and got["counts"]["promoted"] == np.isin(tb["flags"], KEPT_CLASS).sum() > 0
    # the true columns come back within the bar too, whichever candidate starts
    same = host(HL, ch, tb)
    assert (np.linalg.norm(same["points"][:3].T.astype(np.float64) - truth, axis=1) / depth).max() <= EXACT_BAR
    # NaN columns and columns behind a camera: L is taken and counted
    bad = tb["points"].copy()
    bad[:, ::2] = np.nan
    for t in range(1, len(lens), 2):                                           # five units behind the track's first camera
        cam = tb["cams"][tb["obs_cam"][tb["track_offset"][t]] >> 1, 0].astype(np.float64)
        bad[:3, t] = cam[:9].reshape(3, 3).T @ (np.array([0.0, 0.0, -5.0]) - cam[9:])
    got = host(HL, ch, dict(tb, points=bad))
    assert got["counts"]["from_linear"] == len(lens) == got["counts"]["refined"] and (got["start"] == IR.FROM_L).all()
    assert (np.linalg.norm(got["points"][:3].T.astype(np.float64) - truth, axis=1) / depth).max() <= EXACT_BAR
    # skipped tracks, tracks of a flag outside 1..4: copied through with their error
    skip = np.zeros(len(lens), np.uint8); skip[::3] = 1
    flags = tb["flags"].copy(); flags[1] = 0; flags[4] = 5
    got = host(HL, ch, dict(moved, flags=flags), skip=skip)
    through = (skip != 0) | ~np.isin(flags, (1, 2, 3, 4))
    check_counts(got, len(lens))
    assert got["counts"]["copied"] == through.sum() and np.array_equal(got["flags"][through], flags[through])
    assert got["points"][:, through].tobytes() == moved["points"][:, through].tobytes() and (got["err"][through] > 1.0).all()


def test_views_that_share_one_centre(HL):
    ch, tb, truth = IS.shared_centre()
    T = len(tb["flags"])
    got = host(HL, ch, tb)                                                     # L is singular: the (true) column starts every track
    assert (got["start"] == IR.FROM_C).all() and np.isin(got["flags"], REFINED_CLASS).all() and got["counts"]["from_linear"] == 0
    bad = tb["points"].copy()
    bad[:, ::2] = np.nan
    bad[2, 1::2] = -10.0
    arrays = IS.table_arrays(dict(tb, points=bad), 3, 48)
    got = IS.run_host(HL, S, ch, arrays)
    assert got["counts"]["no_start"] == T == got["counts"]["intersected"] and got["counts"]["refined"] == got["counts"]["kept"] == 0
    assert np.isinf(got["err"]).all() and np.array_equal(got["flags"], tb["flags"])
    assert got["raw"][0].reshape(4, 48)[:, :T].tobytes() == arrays[4].reshape(4, 48)[:, :T].tobytes()      # the input bytes, NaNs included
    want = IR.intersect(ch["pairs"], ch["K"], dict(tb, points=bad))
    assert want["counts"] == got["counts"]


# ---- classes and counts after an adjustment -------------------------------------------------------------------------------------
def test_classes_counts_and_skipped_tracks_after_an_adjustment(HL):
    for name, ch, res, adj in adjusted_inputs():
        T = len(res["flags"])
        for skip in (None, adj["used"]):
            got = host(HL, ch, res, cams=adj["cams"], points=adj["points"], skip=skip)
            check_counts(got, T)
            seam_in, seam_out = np.isin(res["flags"], (3, 4)), np.isin(got["flags"], (3, 4))
            assert np.array_equal(seam_in, seam_out) and np.isin(got["flags"], (1, 2, 3, 4)).all(), name
            if skip is not None:
                s = skip != 0
                assert got["counts"]["copied"] == s.sum() and np.array_equal(got["flags"][s], res["flags"][s]), name
                assert got["points"][:, s].tobytes() == np.ascontiguousarray(adj["points"][:, s]).tobytes(), name
                assert got["err"][s].tobytes() == adj["err"][s].tobytes(), name           # the adjustment's own d_err, bit for bit
        print(f"intersect {name} with d_skip = d_used: {got['counts']}")


# ---- host build against the twin ------------------------------------------------------------------------------------------------
def compare_with_twin(name, got, want, lens, depth_of, capped=True):
    """Flags, counts and start choice equal but for listed near-ties; returns the largest point and err differences."""
    T = len(want["flags"])
    flipped = np.flatnonzero(got["start"] != want["start"])
    for t in flipped:
        c = want["costs"][t]
        tie = abs(c[0] - c[1])
        print(f"  {name}: track {t} starts from {got['start'][t]} in the host build, {want['start'][t]} in the twin; costs {c[0]:.9g} / {c[1]:.9g}")
        assert np.isfinite(tie) and tie <= 2.0 * TIE_PX * np.sqrt(lens[t] * max(c)) + lens[t] * TIE_PX ** 2, (name, t, c)
    assert not capped or len(flipped) <= TIE_CAP * T, (name, len(flipped), T)
    keep = np.ones(T, bool); keep[flipped] = False
    assert np.array_equal(got["flags"][keep], want["flags"][keep]), name
    for c in IR.COUNTS:
        assert abs(got["counts"][c] - want["counts"][c]) <= len(flipped), (name, c, got["counts"], want["counts"])
    if not keep.any():
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        a, b = got["points"].astype(np.float64), want["points"]
        d = np.linalg.norm(a[:3] / a[3] - b[:3] / b[3], axis=0) / depth_of(b[:3] / b[3])
        same_nan = np.isnan(a).any(0) == np.isnan(b).any(0)
    assert same_nan[keep].all(), name
    fin = keep & np.isfinite(d)
    assert np.array_equal(np.isinf(got["err"][keep]), np.isinf(want["err"][keep])), name
    fe = keep & np.isfinite(want["err"])
    de = np.abs(got["err"][fe].astype(np.float64) - want["err"][fe]) / np.maximum(1.0, want["err"][fe])
    return (float(d[fin].max()) if fin.any() else 0.0), (float(de.max()) if fe.any() else 0.0)


def test_host_build_against_the_twin(HL):
    """The inputs: the hand-built tables, and SCENES and RINGS after their adjustment with d_skip = d_used -- the call's use, where
    the stale tracks are re-intersected.  On these no start choice flips at all (cap: TIE_CAP of an input's tracks).
    The same tables WITHOUT d_skip are compared too, under every assertion but the cap: there the adjusted tracks go through the call
    as well, and for a track the adjustment has just refined the two candidates tie -- on a two-view track L is the LM optimum to
    ~1e-4 of its cost -- so the fp32 and fp64 costs order them differently on up to 3.4 % of an input's tracks (53 of 1567 on chain
    (1024, 61), 11 of 391 on chain (257, 7); every one within the tie bound, every one listed when the test runs with -s)."""
    worst_p = worst_e = 0.0
    ch, tb, truth, depth = IS.hand_built()
    cases = [("hand-built 5 % off", ch, IS.displaced(tb, truth, depth, 0.05), None, None, None, True)]
    ch3, tb3, truth3 = IS.shared_centre()
    cases.append(("one centre", ch3, tb3, None, None, None, True))
    for name, c, res, adj in adjusted_inputs():
        cases += [(name + ", d_skip = d_used", c, res, adj["cams"], adj["points"], adj["used"], True), (name + ", no d_skip", c, res, adj["cams"], adj["points"], None, False)]
    most = 0.0
    for name, c, table, cams, points, skip, capped in cases:
        got = host(HL, c, table, cams=cams, points=points, skip=skip)
        want = IR.intersect(c["pairs"], c["K"], table if points is None else dict(table, points=points), cams=cams, skip=skip)
        p, e = compare_with_twin(name, got, want, np.diff(table["track_offset"]), lambda X: np.abs(X[2]), capped)
        flips = int((got["start"] != want["start"]).sum())
        most = max(most, 0.0 if capped else flips / len(want["flags"]))
        print(f"intersect host build - twin, {name}: points {p:.3g} of the depth, err {e:.3g} px, {flips} of {len(want['flags'])} start choices flipped")
        worst_p, worst_e = max(worst_p, p), max(worst_e, e)
    print(f"intersect host build - twin over all inputs: points {worst_p:.3g} (bar {BAR_POINT:.3g}), err {worst_e:.3g} (bar {BAR_ERR:.3g}); "
          f"largest share of flipped start choices without d_skip {most:.3g}")
    assert worst_p <= BAR_POINT and worst_e <= BAR_ERR


# ---- what the feature buys ------------------------------------------------------------------------------------------------------
def stale_rms(pairs, K, table, cams, points, tracks):
    """rms pixel error of the given tracks' observations under `cams` at `points`, over the observations in front of their camera;
    and how many are not."""
    sq, n, behind = 0.0, 0, 0
    for t in tracks:
        v = IR.views_of(pairs, K, table, cams, t)
        with np.errstate(all="ignore"):
            r, _, z = IR.residuals(v, points[:3, t] / points[3, t])
        ok = (z > 0) & np.isfinite(r).all(1)
        sq += float((r[ok] ** 2).sum()); n += int(ok.sum()); behind += int((~ok).sum())
    return np.sqrt(sq / max(2 * n, 1)), behind


@pytest.mark.parametrize("k,n,seed,W,over_long", [(6, 257, 7, 3, 240), (36, 65, 3, 8, 85)])
def test_what_the_call_buys_on_stale_tracks(HL, k, n, seed, W, over_long):
    """After the twin's adjust_ring the tracks it did not use are re-intersected: their rms pixel error under the adjusted cameras
    must not rise in the twin, and the host build must move it the same way.  No bar on the distance to the truth: the free gauge
    moves it either way."""
    sc, ring, res = RAS.fused_ring(k, n, seed)
    adj = RR.adjust_ring(ring["pairs"], ring["K"], res, max_track_views=W)
    lens = np.diff(res["track_offset"])
    assert (lens > W).sum() == over_long and adj["report"]["status"] != RR.DEGENERATE
    cams32 = adj["cams"].astype(np.float32)
    stale = np.flatnonzero(~adj["used"] & np.isin(res["flags"], (1, 2, 3, 4)) & (lens >= 2))
    table = dict(res, points=adj["points"])
    twin = IR.intersect(ring["pairs"], ring["K"], table, cams=cams32, skip=adj["used"])
    got = host(HL, ring, res, cams=cams32, points=adj["points"], skip=adj["used"])
    before, b0 = stale_rms(ring["pairs"], ring["K"], res, cams32.astype(np.float64), adj["points"], stale)
    after_twin, b1 = stale_rms(ring["pairs"], ring["K"], res, cams32.astype(np.float64), twin["points"], stale)
    after_host, b2 = stale_rms(ring["pairs"], ring["K"], res, cams32.astype(np.float64), got["points"].astype(np.float64), stale)
    feat = np.array([FRS.feature(sc, res["obs_cam"][res["track_offset"][t]] >> 1, res["obs_record"][res["track_offset"][t]]) for t in stale])
    truth = FRS.truth_in_pair0(sc, feat)
    dist = lambda P: float(np.median(np.linalg.norm((P[:3, stale] / P[3, stale]).T - truth, axis=1)))
    print(f"intersect on ring ({k}, {n}, {seed}) at W = {W}: {len(stale)} stale tracks ({over_long} over-long), rms {before:.4g} px -> twin "
          f"{after_twin:.4g}, host build {after_host:.4g}; behind a camera {b0} -> {b1} / {b2}; promoted {twin['counts']['promoted']} / "
          f"{got['counts']['promoted']}; median distance to the truth {dist(np.asarray(adj['points'], np.float64)):.4g} -> {dist(twin['points']):.4g} / "
          f"{dist(got['points'].astype(np.float64)):.4g}")
    assert got["counts"]["intersected"] == twin["counts"]["intersected"] == len(stale)
    assert after_twin <= before and b1 <= b0
    assert (after_host <= before) == (after_twin <= before) and b2 <= b0


# ---- pins ---------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_little_lds():
    """build/intersect.usage.txt (written next to the object): no scratch in either kernel, VGPRs that keep at least four wavefronts
    per SIMD, the wavefront kernel's term buffer a few KB."""
    path = os.path.join(IS.ROOT, "build", "intersect.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it with the library"
    text = open(path).read()
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", text, re.S):
        found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    lane = [v for k, v in found.items() if "intersect_lane_kernel" in k]
    wave = [v for k, v in found.items() if "intersect_wave_kernel" in k]
    assert len(lane) == 1 and len(wave) == 1, found
    print(f"intersect.hip: lane kernel (VGPRs, scratch, LDS) {lane[0]}, wavefront kernel {wave[0]}")
    assert lane[0][1] == 0 and wave[0][1] == 0
    assert lane[0][0] <= 128 and wave[0][0] <= 128
    assert lane[0][2] == 0 and 0 < wave[0][2] <= 8192
