"""CPU: sfm_fuse_chain without a device -- the host build (tests/hostcheck/libfusecheck.so: fuse_math.hpp's functions, the nodes
visited serially) against cuda_sfm_amd.chain_links, against ground truth and against the fp64 twin (tests/fuse_reference.py) on
the checked six-view scenes: frames, cameras, the track table, the conflict rule, cuts, a ragged chain, exact and noisy points,
zero iterations; struct layouts, header / exports / Python mirror, the argument checks that precede the device, and the
compiler's resource report of fuse.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_reference as FR
import fuse_scene as FS
import refine_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "build", "fuse.usage.txt")
NAMES = ["sfm_fuse_default_params", "sfm_fuse_chain"]
# Frames of the host build (composed in fp64, rounded once to fp32) against cuda_sfm_amd.chain_links (fp64) over the four links of
# the scene: MEASURED largest relative difference in s, rotation angle (rad), |dt| / max(1, |t|).  What is left is the one
# rounding to fp32.  The bars are 4 x these.
FRAMES_MEASURED = dict(s=3.91e-8, rot=6.78e-9, t=2.84e-8)
FRAMES_BARS = {k: 4.0 * v for k, v in FRAMES_MEASURED.items()}
CAMERA_BAR_PX = 1e-3                                  # exact points through d_cams against the observations
EXACT_BAR = 1e-4                                      # fused point against the truth, relative to its depth (6c's bar)
BAND = 0.10                                           # flags are compared outside this share of the threshold ...
BAND_CAP = 0.01                                       # ... which at most this share of the tracks may lie in


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def HL():
    return FS.host_lib()


@pytest.fixture(scope="module")
def runs(S, HL):
    """Per checked scene: the scene, its chain, the host build's result and the twin's, computed once."""
    out = []
    for n, seed in FS.SCENES:
        sc, ch = FS.build(n, seed)
        out.append((sc, ch, FS.run_host(HL, S, ch), FR.fuse(ch)))
    return out


@pytest.fixture(scope="module")
def exact(S, HL):
    """512 records, no noise, no wrong matches, no wrong indices."""
    sc, ch = FS.build(512, 11, noise_px=0.0, wrong_match=0.0, wrong_index=0.0)
    return sc, ch, FS.run_host(HL, S, ch)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def structure_equal(got, want):
    for k in ("track", "track_offset", "obs_cam", "obs_record", "root"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("tracks", "observations", "segments", "longest_track"):
        assert got["counts"][k] == want["counts"][k], (k, got["counts"], want["counts"])


def offsets(chain):
    return np.concatenate([[0], np.cumsum([P["n"] for P in chain["pairs"]])]).astype(int)


def test_frames_equal_chain_links(S, runs):
    worst = dict.fromkeys(FRAMES_MEASURED, 0.0)
    for sc, ch, got, _ in runs:
        want = S.chain_links([L["sim"] for L in ch["links"]])
        assert np.array_equal(got["root"], np.zeros(len(ch["pairs"]), np.int32)) and got["counts"]["segments"] == 1
        assert np.array_equal(got["frames"][0], FS.sim13(1.0, np.eye(3), np.zeros(3)))
        for f, (s, R, t) in zip(got["frames"].astype(np.float64), want):
            worst["s"] = max(worst["s"], abs(f[0] - s) / s)
            worst["rot"] = max(worst["rot"], RR.rotation_angle(f[1:10].reshape(3, 3), R))
            worst["t"] = max(worst["t"], float(np.linalg.norm(f[10:13] - t) / max(1.0, np.linalg.norm(t))))
    print(f"fuse frames against chain_links: {worst}")
    for k, bar in FRAMES_BARS.items():
        assert worst[k] <= bar, (k, worst[k], bar)


def pixels(K, cam12, X):
    """Pixel position of X (3) under the camera [R|t] given as 12 floats."""
    Y = cam12[:9].reshape(3, 3) @ X + cam12[9:]
    p = K @ (Y / Y[2])
    return p[:2]


def test_cameras_reproduce_the_observations_of_the_exact_chain(exact):
    sc, ch, got = exact
    K = ch["K"].astype(np.float64)
    truth = FS.truth_in_pair0(sc, ch, got)
    worst = 0.0
    for t in range(got["counts"]["tracks"]):
        for o in range(got["track_offset"][t], got["track_offset"][t + 1]):
            pair, slot, rec = got["obs_cam"][o] >> 1, got["obs_cam"][o] & 1, got["obs_record"][o]
            x = ch["pairs"][pair]["X1" if slot else "X0"][:, rec].astype(np.float64)
            seen = (K @ (x / x[2]))[:2]
            worst = max(worst, float(np.linalg.norm(pixels(K, got["cams"][pair, slot].astype(np.float64), truth[t]) - seen)))
    print(f"fuse cameras, exact chain: largest reprojection difference {worst:.3g} px over {got['counts']['observations']} observations")
    assert got["counts"]["observations"] > 2000 and worst <= CAMERA_BAR_PX


@pytest.mark.parametrize("which", range(len(FS.SCENES)))
def test_track_structure_equals_the_twin(runs, which):
    sc, ch, got, want = runs[which]
    structure_equal(got, want)
    L = np.diff(got["track_offset"]) - 1
    print(f"fuse scene {FS.SCENES[which]}: {got['counts']}, tracks over 1..5 pairs {np.bincount(L, minlength=6)[1:].tolist()}")
    assert got["counts"]["tracks"] == {(257, 7): 391, (1024, 61): 1567, (64, 5): 90, (65, 5): 95}[FS.SCENES[which]]
    if FS.SCENES[which] == (257, 7):
        assert np.bincount(L, minlength=6)[1:].tolist() == [111, 73, 69, 37, 101]
    # the table is consistent in itself: every live node in exactly one track, observations ordered by view
    off = offsets(ch)
    seen = np.zeros(off[-1], int)
    for t in range(len(L)):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1])
        cam = got["obs_cam"][o]
        assert np.array_equal(cam[:-1], 2 * (cam[0] // 2 + np.arange(len(o) - 1))) and cam[-1] == cam[-2] + 1
        assert got["obs_record"][o[-1]] == got["obs_record"][o[-2]]
        nodes = off[cam[:-1] // 2] + got["obs_record"][o[:-1]]
        assert (got["track"][nodes] == t).all()
        seen[nodes] += 1
    live = np.concatenate([FR.live_nodes(P) for P in ch["pairs"]])
    assert np.array_equal(seen, live.astype(int)) and np.array_equal(got["track"] >= 0, live)
    assert got["counts"]["observations"] == live.sum() + got["counts"]["tracks"]


def test_conflicts_go_to_the_smallest_error_then_the_lowest_record(S, HL, runs):
    sc, ch, _, _ = runs[0]
    base = FS.head(ch, 2)
    L = base["links"][0]
    live0 = FR.live_nodes(base["pairs"][0])
    prop = np.flatnonzero(L["inlier"] != 0)
    m = int(L["index"][prop[5]])                             # a target one record already proposes
    others = [int(j) for j in np.flatnonzero(live0 & (L["inlier"] == 0))[:2]]
    first = int(prop[5])
    off = offsets(base)
    for name, recs, errs, winner in (("two, the later one better", [first, others[0]], [0.5, 0.25], others[0]),
                                     ("three, the middle one best", sorted([first] + others), [0.5, 0.125, 0.25], sorted([first] + others)[1]),
                                     ("two alike", [first, others[0]], [0.25, 0.25], min(first, others[0])),
                                     ("three alike", sorted([first] + others), [0.25, 0.25, 0.25], min([first] + others))):
        link = dict(L, index=L["index"].copy(), inlier=L["inlier"].copy(), err=L["err"].copy())
        for j, e in zip(recs, errs):
            link["index"][j] = m; link["inlier"][j] = 1; link["err"][j] = e
        chain = dict(base, links=[link])
        got = FS.run_host(HL, S, chain)
        structure_equal(got, FR.fuse(chain, max_iterations=0))
        t = got["track"][off[1] + m]
        assert t >= 0 and got["track"][winner] == t, name
        for j in recs:
            if j == winner:
                continue
            tj = got["track"][j]                             # a loser heads a track of its own: one pair, two observations
            assert tj >= 0 and tj != t and got["track_offset"][tj + 1] - got["track_offset"][tj] == 2, (name, j)
            assert got["obs_record"][got["track_offset"][tj]] == j


def test_an_invalid_link_cuts_the_chain(S, HL, runs):
    sc, ch, whole, _ = runs[0]
    off = offsets(ch)

    def cut(**change):
        return dict(ch, links=[dict(L, **change) if i == 2 else L for i, L in enumerate(ch["links"])])
    nan_t = ch["links"][2]["sim"].copy(); nan_t[11] = np.nan
    zero_s = ch["links"][2]["sim"].copy(); zero_s[0] = 0.0
    for name, chain in (("degenerate", cut(status=S.REFINE_DEGENERATE)), ("s = 0", cut(sim=zero_s)), ("NaN in t", cut(sim=nan_t))):
        got = FS.run_host(HL, S, chain)
        structure_equal(got, FR.fuse(chain, max_iterations=0))
        assert got["root"].tolist() == [0, 0, 0, 3, 3] and got["counts"]["segments"] == 2, name
        assert np.array_equal(got["frames"][3], FS.sim13(1.0, np.eye(3), np.zeros(3))), name
        assert np.array_equal(got["cams"][3, 0], np.concatenate([np.eye(3).ravel(), np.zeros(3)]).astype(np.float32)), name
        assert np.array_equal(got["cams"][3, 1], chain["pairs"][3]["pose"]), name
        assert np.array_equal(u8(got["frames"][:3]), u8(whole["frames"][:3])), name
        for t in range(got["counts"]["tracks"]):               # no track holds observations from both sides
            pairs = got["obs_cam"][got["track_offset"][t]:got["track_offset"][t + 1]] >> 1
            assert pairs.max() <= 2 or pairs.min() >= 3, (name, t)
        assert got["counts"]["tracks"] > whole["counts"]["tracks"] and got["counts"]["longest_track"] == 4
        assert np.array_equal(got["track"] >= 0, whole["track"] >= 0)
        assert np.isfinite(got["points"]).all() and np.isfinite(got["frames"]).all()
    assert off[-1] == 5 * 257


def test_ragged_chain(S, HL, runs):
    sc, ch, _, _ = runs[0]
    sizes = [65, 257, 64, 257, 1]
    chain = FS.truncated(ch, sizes)
    got = FS.run_host(HL, S, chain)
    want = FR.fuse(chain)
    structure_equal(got, want)
    off = offsets(chain)
    assert off[-1] == sum(sizes) and len(got["track"]) == off[-1]
    past = sum(int(((L["index"] >= chain["pairs"][i + 1]["n"]) & (L["inlier"] != 0)).sum()) for i, L in enumerate(chain["links"]))
    assert past > 50                                          # indices past the end of a cut pair are there, and give no edge
    for t in range(got["counts"]["tracks"]):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1])
        assert (got["obs_record"][o] < np.array(sizes)[got["obs_cam"][o] >> 1]).all()
    print(f"fuse ragged chain {sizes}: {got['counts']}, {past} inlier indices past the end")
    assert np.array_equal(got["flags"], want["flags"])


def test_exact_scene_recovers_the_points(exact):
    sc, ch, got = exact
    truth = FS.truth_in_pair0(sc, ch, got)
    assert got["counts"]["tracks"] >= 512 and (got["flags"] == FR.REFINED).all() and np.isfinite(truth).all()
    d = np.linalg.norm(got["points"][:3].T.astype(np.float64) - truth, axis=1) / truth[:, 2]
    print(f"fuse exact scene: {got['counts']}, largest |X - truth| / depth {d.max():.3g}, largest err {got['err'].max():.3g} px")
    assert (got["points"][3] == 1.0).all() and d.max() <= EXACT_BAR


@pytest.mark.parametrize("which", range(len(FS.SCENES)))
def test_noisy_scenes_against_the_twin(runs, which):
    sc, ch, got, want = runs[which]
    thr = 4.0
    band = np.abs(want["err"] - thr) <= BAND * thr
    print(f"fuse scene {FS.SCENES[which]}: refined / kept {got['counts']['refined']} / {got['counts']['kept']} (twin "
          f"{want['counts']['refined']} / {want['counts']['kept']}), {band.sum()} of {len(band)} tracks within {BAND:.0%} of the threshold")
    assert band.mean() <= BAND_CAP
    assert np.array_equal(got["flags"][~band], want["flags"][~band])
    assert got["counts"]["refined"] + got["counts"]["kept"] == got["counts"]["tracks"]
    assert got["counts"]["refined"] == (got["flags"] == FR.REFINED).sum() and set(np.unique(got["flags"])) <= {FR.REFINED, FR.KEPT}
    # kept tracks hold the start point, refined ones the LM result: both against the twin's (fp64)
    same = ~band
    scale = np.maximum(1.0, np.abs(want["points"][2]))
    d = np.abs(got["points"].astype(np.float64) - want["points"])[:3].max(0) / scale
    fin = np.isfinite(want["err"]) & same
    de = np.abs(got["err"][fin].astype(np.float64) - want["err"][fin]) / np.maximum(1.0, want["err"][fin])
    print(f"  against the twin: points {d[same].max():.3g} relative to depth, err {de.max():.3g}")
    # fp32 against fp64 over up to six views: 6c's bar for a point, a twentieth of a pixel (relative above 1 px) for the error
    assert d[same].max() <= EXACT_BAR * 10 and de.max() <= 0.05
    # fused against the mean of the pairs' own points, on tracks over at least three pairs of one true feature
    L = np.diff(got["track_offset"]) - 1
    truth = FS.truth_in_pair0(sc, ch, got)
    pure = np.zeros(len(L), bool)
    for t in np.flatnonzero(L >= 3):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1] - 1)
        ids = [sc["perm"][got["obs_cam"][q] >> 1][got["obs_record"][q]] for q in o]
        pure[t] = len(set(ids)) == 1 and all(sc["pairs"][got["obs_cam"][q] >> 1]["good"][got["obs_record"][q]] for q in o)
    pure &= got["flags"] == FR.REFINED
    twin_fused = np.linalg.norm(want["X"][pure] - truth[pure], axis=1)
    twin_mean = np.linalg.norm(want["start"][pure] - truth[pure], axis=1)
    fused = np.linalg.norm(got["points"][:3].T[pure].astype(np.float64) - truth[pure], axis=1)
    print(f"  {pure.sum()} clean tracks over >= 3 pairs: median distance to the truth fused {np.median(fused):.4g} (twin {np.median(twin_fused):.4g}), "
          f"mean of the pairs' points {np.median(twin_mean):.4g}")
    if pure.sum() >= 8 and np.median(twin_fused) < np.median(twin_mean):          # only where the twin shows it
        assert np.median(fused) < np.median(twin_mean)


def test_zero_iterations_return_the_mean(S, HL, runs):
    sc, ch, _, _ = runs[0]
    got = FS.run_host(HL, S, ch, max_iterations=0)
    f32 = np.float32
    for t in range(got["counts"]["tracks"]):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1] - 1)
        total = np.zeros(3, f32)
        for q in o:
            pair, rec = got["obs_cam"][q] >> 1, got["obs_record"][q]
            X = ch["pairs"][pair]["points"][:, rec].astype(f32)
            F = got["frames"][pair]
            x = X[:3] / X[3]
            Y = np.array([F[0] * ((F[1 + 3 * a] * x[0] + F[2 + 3 * a] * x[1]) + F[3 + 3 * a] * x[2]) + F[10 + a] for a in range(3)], f32)
            total = total + Y
        mean = total / f32(len(o))
        assert np.array_equal(u8(got["points"][:3, t]), u8(mean)), t
    assert (got["points"][3] == 1.0).all()
    again = FS.run_host(HL, S, ch, max_iterations=0)
    for k in ("points", "flags", "err", "frames", "cams"):
        assert np.array_equal(u8(got[k]), u8(again[k])), k


def test_one_pair_has_two_views_per_track(S, HL, runs):
    sc, ch, _, _ = runs[0]
    chain = FS.head(ch, 1)
    got = FS.run_host(HL, S, chain)
    live = FR.live_nodes(chain["pairs"][0])
    assert got["counts"]["tracks"] == live.sum() and got["counts"]["observations"] == 2 * live.sum() and got["counts"]["longest_track"] == 2
    assert np.array_equal(got["track_offset"], 2 * np.arange(live.sum() + 1)) and got["counts"]["segments"] == 1
    assert np.array_equal(got["obs_record"][0::2], np.flatnonzero(live)) and np.array_equal(got["obs_cam"], np.tile([0, 1], live.sum()))
    structure_equal(got, FR.fuse(chain))


def test_struct_layouts_match_the_header(S, HL):
    for which, T in enumerate((S.FuseParams, S.FusePairIn, S.FuseLinkIn, S.FuseOut)):
        out = (C.c_int64 * 16)()
        nf = HL.fuse_layout(which, out)
        assert nf == len(T._fields_) and out[0] == C.sizeof(T), T
        assert [out[1 + i] for i in range(nf)] == [getattr(T, f).offset for f, _ in T._fields_], T


def test_declared_exported_wrapped_and_documented(S):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_amd.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    for name in NAMES:
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
        assert name in exported, name
    assert re.search(r"#define\s+SFM_ABI_VERSION\s+3\b", hdr)
    for f in ("fuse_params", "fuse_chain", "fuse_chain_enqueue"):
        assert callable(getattr(S, f)), f
    assert (S.FUSE_REFINED, S.FUSE_KEPT) == (1, 2) == (FR.REFINED, FR.KEPT)
    p = S.fuse_params()
    assert (p.threshold_px, p.max_iterations, p.huber_px) == (4.0, 5, 1.0)
    assert p.initial_lambda == np.float32(1e-3) and p.min_rel_decrease == np.float32(1e-6) and not any(p.reserved)
    with pytest.raises(TypeError):
        S.fuse_params(num_hypotheses=4)


def test_argument_checks_come_before_any_device_call(S):
    call, ref = S.lib().sfm_fuse_chain, C.byref
    p = S.fuse_params()
    pin = (S.FusePairIn * 1)(S.FusePairIn(None, None, None, None))                 # a null pair: refused before any pair is read
    lin = (S.FuseLinkIn * 1)()
    out = S.FuseOut(*[0x1000 * (i + 2) for i in range(11)])
    ctx = C.c_void_p(0x7000)                                                      # never dereferenced
    assert call(ctx, pin, 1, lin, None, ref(out)) == S.E_INVALID
    assert call(ctx, pin, -1, lin, ref(p), ref(out)) == S.E_INVALID and call(ctx, pin, 4097, lin, ref(p), ref(out)) == S.E_INVALID
    assert call(None, pin, 1, lin, ref(p), ref(out)) == S.E_INVALID and call(ctx, None, 1, lin, ref(p), ref(out)) == S.E_INVALID
    assert call(ctx, pin, 1, lin, ref(p), None) == S.E_INVALID
    assert call(ctx, pin, 1, None, ref(p), ref(out)) == S.E_INVALID and b"pairs[0]" in S.lib().sfm_last_error()
    for i, (f, _) in enumerate(S.FuseOut._fields_):
        if f == "d_err":
            continue
        o = S.FuseOut(*[None if q == i else 0x1000 * (q + 2) for q in range(11)])
        assert call(ctx, pin, 1, lin, ref(p), ref(o)) == S.E_INVALID and b"required" in S.lib().sfm_last_error(), f
    for kw in (dict(threshold_px=0.0), dict(threshold_px=float("nan")), dict(max_iterations=-1), dict(max_iterations=51), dict(huber_px=-1.0),
               dict(min_rel_decrease=float("inf")), dict(initial_lambda=-1.0), dict(reserved=[0, 0, 1, 0])):
        assert call(ctx, pin, 1, lin, ref(S.fuse_params(**kw)), ref(out)) == S.E_INVALID, kw
        assert call(None, None, 0, None, ref(S.fuse_params(**kw)), None) == S.E_INVALID, kw


def test_zero_pairs_is_not_an_error(S):
    p = S.fuse_params()
    assert S.lib().sfm_fuse_chain(None, None, 0, None, C.byref(p), None) == S.OK
    assert S.lib().sfm_fuse_chain(None, None, 0, None, None, None) == S.E_INVALID    # the parameters are checked whatever the count
    assert S.fuse_chain([], [], [])["counts"]["tracks"] == 0


def kernel_usage():
    """{mangled kernel name: {field: value}} of build/fuse.usage.txt (-Rpass-analysis=kernel-resource-usage)."""
    assert os.path.exists(USAGE), "run `make`: the product build leaves the compiler's resource report next to the objects"
    out, cur = {}, None
    for line in open(USAGE):
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_resource_report():
    """Seven kernels, no scratch in any of them (the points kernel keeps no per-view array)."""
    usage = kernel_usage()
    assert len(usage) == 7, sorted(usage)
    for stage in ("frames", "edges", "links", "count", "scan", "fill", "points"):
        hits = [v for k, v in usage.items() if f"fuse_{stage}_kernel" in k]
        assert len(hits) == 1, (stage, sorted(usage))
        print(f"fuse_{stage}: {hits[0]['VGPRs']} VGPRs, LDS {hits[0]['LDS Size']}, scratch {hits[0]['ScratchSize']}")
        assert hits[0]["ScratchSize"] == 0, (stage, hits[0])
        # the frames kernel stages 256 inverse links (fp64) and 256 frames; the node kernels hold only their scan's wave sums
        assert hits[0]["VGPRs"] <= 128 and hits[0]["LDS Size"] <= (42 * 1024 if stage == "frames" else 128), (stage, hits[0])
