"""CPU: sfm_close_ring without a device -- the host build (tests/hostcheck/libringcheck.so: ring_math.hpp's functions, the links
and records visited serially) against the identity it must close to, against ground truth and against the fp64 twin
(tests/ring_reference.py) on the rings of tests/ring_scene.py: the rotation's logarithm and exponential, closure at 3 .. 630
links, an exact ring, one bad link, distributed drift, OPEN and REJECTED rings; struct layouts, header / Python mirror, the
argument checks that precede the device, and the compiler's resource report of ring.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuse_scene as FS
import refine_reference as RR
import ring_reference as RF
import ring_scene as RS

ROOT = RS.ROOT
USAGE = os.path.join(ROOT, "build", "ring.usage.txt")
CLOSURE_K = [3, 6, 70, 630]
# All MEASURED on the host build, rings of CLOSURE_K links whose every link carries a drift of 2e-3 rad, 1 % in s and 1 % in t
# (ring_scene.small_similarities); (s relative, rotation angle in rad, |dt| / max(1, |t|)).  The bars are 4 x these.
# CLOSURE: the k corrected fp32 links composed in fp64 against the identity.  The translation is the lever arm: at 630 views the
# baselines are 0.08 and the ring is 200 gauge units across, so one fp32 rounding of a link's rotation (6e-8) moves the far side
# by 1e-5, 630 times over.  The measured links composed the same way are off by the drift itself.
CLOSURE_MEASURED = dict(s=9.79e-8, rot=2.01e-8, t=2.41e-3)
# RECOMPOSED: libfusecheck's frames over the first k - 1 corrected links against the call's closed frames (the same lever arm).
RECOMPOSED_MEASURED = dict(s=5.29e-7, rot=6.12e-8, t=2.51e-3)
# ROUNDING: a corrected link against the link it should equal where nothing is to correct (an exact ring; the links of a one-bad-link
# ring that carry no weight): the one rounding to fp32, and on the exact ring the share of the drift that its fp32 links have.
# s: measured 0 everywhere; half a unit in the last place of fp32 stands in for it.
ROUNDING_MEASURED = dict(s=6.0e-8, rot=3.44e-8, t=1.29e-6)
# EXACT_DRIFT: the drift numbers of a ring of TRUE links rounded to fp32 (|ln s_D|, the angle of D, |t_D| relative to the largest
# translation component of a frame), largest over CLOSURE_K: what k fp32 roundings compose to.
EXACT_DRIFT_MEASURED = dict(s=1.57e-7, rot=2.24e-8, t=2.83e-7)
# max |R R^T - I| of the corrected links at 630 links (4.3e-7 at 3, 2.5e-6 at 70); the input links' own (rotations rounded to
# fp32) is 1.3e-7: a corrected link is F'_{i+1}^T F'_i, and the frames are products of up to 630 such rotations
DEFECT_MEASURED = 8.48e-6
# the host build against the twin: links, frames and the report's floats, over CLOSURE_K and the seam scenes
TWIN_MEASURED = dict(s=5.83e-8, rot=3.28e-8, t=5.49e-8, drift=1.46e-8, rms_px=2.79e-5, seam_px=1.61e-4)
EXACT_BAR = 1e-4                                      # 6g's exact-data bars: s, rad, relative t
BAND, BAND_CAP = 0.10, 0.01                           # seam flags are compared outside this share of the threshold; at most this share lies in it
DRIFT_SEEDS = {6: [1, 2, 3, 4], 36: [1, 2, 3, 4]}     # scenes on which the twin's closed centres beat its open ones (chosen on the CPU)
SEAM_SCENES = [(6, 1024, 3), (36, 257, 5), (5, 65, 9)]    # (k, n, seed): true links with a tenth of the drift above


def bars(measured):
    return {k: 4.0 * v for k, v in measured.items()}


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


@pytest.fixture(scope="module")
def FL():
    return FS.host_lib()


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def sim_diff(a, b):
    """(relative s, rotation angle, |dt| / max(1, |t|)) of two similarities given as 13 numbers."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return dict(s=abs(a[0] - b[0]) / b[0], rot=RR.rotation_angle(a[1:10].reshape(3, 3), b[1:10].reshape(3, 3)),
                t=float(np.linalg.norm(a[10:13] - b[10:13]) / max(1.0, np.linalg.norm(b[10:13]))))


def worst_of(pairs):
    out = dict(s=0.0, rot=0.0, t=0.0)
    for a, b in pairs:
        d = sim_diff(a, b)
        out = {k: max(out[k], d[k]) for k in out}
    return out


def defect(sims):
    R = np.asarray(sims, np.float64)[:, 1:10].reshape(-1, 3, 3)
    return float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())


def within(worst, bar, what):
    for k, b in bar.items():
        assert worst[k] <= b, (what, k, worst[k], b)


def drifting(k, n=64, scale=1.0):
    """A ring of k links, each composed with a small similarity of its own."""
    sc = RS.build(k, n, 100 + k)
    sims = RS.perturbed(sc["sims"], RS.small_similarities(k, 7 + k, rot=2e-3 * scale, scale=0.01 * scale, trans=0.01 * scale))
    return sc, RS.ring_input(sc, sims=sims)


def fuse_frames(FL, S, sims, status=None):
    """libfusecheck's d_frames for a chain of len(sims) + 1 pairs without records over the given links."""
    k = len(sims) + 1
    empty = dict(n=0, ld=0, points=np.zeros((4, 0), np.float32), valid=np.zeros(0, np.uint8), X0=np.zeros((3, 0), np.float32),
                 X1=np.zeros((3, 0), np.float32), pose=np.concatenate([np.eye(3).ravel(), np.zeros(3)]).astype(np.float32))
    links = [dict(index=np.zeros(0, np.int32), sim=np.asarray(s, np.float32), inlier=np.zeros(0, np.uint8), err=np.zeros(0, np.float32),
                  status=0 if status is None else int(status[i])) for i, s in enumerate(sims)]
    return FS.run_host(FL, S, dict(K=np.eye(3, dtype=np.float32), pairs=[empty] * k, links=links))["frames"]


@pytest.fixture(scope="module")
def closures(S, HL):
    """Per k of CLOSURE_K: the input, the host build's result and the twin's, computed once."""
    out = {}
    for k in CLOSURE_K:
        sc, inp = drifting(k)
        out[k] = (sc, inp, RS.run_host(HL, S, inp), RF.close_ring(inp))
    return out


# ---- the rotation's logarithm and exponential ------------------------------------------------------------------------------------
def test_rotation_log_and_exp_round_trip(HL):
    rng = np.random.default_rng(5)
    worst_w, worst_R, worst_twin = 0.0, 0.0, 0.0
    angles = [0.0, 1e-300, 1e-12, 1e-8, 1e-4, 2e-3, 0.1, 0.35, 1.0, 0.5 * np.pi, 2.5]
    for th in angles + list(rng.uniform(0, 0.5 * np.pi, 50)):
        a = rng.standard_normal(3); a /= np.linalg.norm(a)
        w = np.ascontiguousarray(th * a)
        R, back = np.zeros(9), np.zeros(3)
        HL.ring_exp(w.ctypes.data, R.ctypes.data)
        angle = HL.ring_log(R.ctypes.data, back.ctypes.data)
        Rm = R.reshape(3, 3)
        worst_R = max(worst_R, float(np.abs(Rm @ Rm.T - np.eye(3)).max()), abs(np.linalg.det(Rm) - 1.0))
        worst_w = max(worst_w, float(np.linalg.norm(back - w)), abs(angle - th))
        worst_twin = max(worst_twin, float(np.abs(Rm - RF.rot_exp(w)).max()), float(np.linalg.norm(back - RF.rot_log(Rm)[0])))
    print(f"ring log / exp: |log(exp w) - w| {worst_w:.3g}, orthonormality of exp {worst_R:.3g}, against the twin {worst_twin:.3g}")
    # fp64 through sin, cos and atan2: measured 4.44e-16 each; the bars are 4 x that
    assert worst_w <= 4 * 4.44e-16 and worst_R <= 4 * 4.44e-16 and worst_twin <= 4 * 4.44e-16
    # the vanishing case returns v itself, and the identity has no logarithm but 0
    R, back = np.eye(3).ravel().copy(), np.ones(3)
    assert HL.ring_log(R.ctypes.data, back.ctypes.data) == 0.0 and not back.any()


# ---- closure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CLOSURE_K)
def test_corrected_links_compose_to_the_identity(S, FL, closures, k):
    sc, inp, (links, frames, seam, rep), twin = closures[k]
    assert rep["status"] == S.RING_CLOSED and rep["first_invalid"] == -1 and rep["num_links"] == k
    identity = RF.pack(RF.IDENTITY)

    def composed(sims):
        F = RF.IDENTITY
        for L in sims:
            F = RF.compose(F, RF.invert(RF.unpack(L)))
        return RF.pack(F)
    closed, was = sim_diff(composed(links), identity), sim_diff(composed(inp["sims"]), identity)
    re = worst_of(zip(fuse_frames(FL, S, links[:k - 1]), frames))
    d_in, d_out = defect(inp["sims"]), defect(links)
    print(f"ring closure k={k}: corrected {closed}, measured links {was}; recomposed by fusecheck {re}; defect in {d_in:.3g} out {d_out:.3g}")
    within(closed, bars(CLOSURE_MEASURED), "closure")
    within(re, bars(RECOMPOSED_MEASURED), "recomposed")
    assert d_out <= 4.0 * DEFECT_MEASURED
    assert np.array_equal(frames[0], FS.sim13(1.0, np.eye(3), np.zeros(3)))
    assert was["rot"] > 100 * closed["rot"]                                    # the drift was there to close


def test_exact_ring_closes_onto_itself(S, HL):
    worst, drift = dict(s=0.0, rot=0.0, t=0.0), dict(s=0.0, rot=0.0, t=0.0)
    for k in CLOSURE_K:
        sc = RS.build(k, 64, 100 + k)
        inp = RS.ring_input(sc)
        links, frames, seam, rep = RS.run_host(HL, S, inp)
        assert rep["status"] == S.RING_CLOSED
        w = worst_of(zip(links, inp["sims"]))
        worst = {q: max(worst[q], w[q]) for q in worst}
        # the drift numbers in sim_diff's units: |ln s|, the angle, |t| relative to the largest translation of a frame
        d = dict(s=abs(rep["drift_log_scale"]), rot=rep["drift_rotation_rad"], t=rep["drift_t"] / max(1.0, np.abs(frames[:, 10:]).max()))
        drift = {q: max(drift[q], d[q]) for q in drift}
    print(f"exact ring: corrected against input links {worst}, drift numbers {drift}")
    within(worst, bars(ROUNDING_MEASURED), "exact ring")
    within(drift, bars(EXACT_DRIFT_MEASURED), "exact ring's drift numbers")


@pytest.mark.parametrize("k", [6, 36])
def test_one_bad_link_absorbs_the_whole_drift(S, HL, k):
    sc = RS.build(k, 64, 100 + k)
    delta = (1.05, RS.rodrigues([0.02, -0.05, 0.03]), np.array([0.03, -0.02, 0.05]))
    for m in (0, k // 2, k - 1):
        sims = RS.perturbed(sc["sims"], [delta if i == m else None for i in range(k)])
        inp = RS.ring_input(sc, sims=sims)
        links, frames, seam, rep = RS.run_host(HL, S, inp, weights=np.eye(k)[m])
        assert rep["status"] == S.RING_CLOSED
        t = sc["true"][m]
        d = sim_diff(links[m], RF.pack(t))
        d["t"] = float(np.linalg.norm(links[m, 10:].astype(np.float64) - t[2]) / np.linalg.norm(t[2]))
        others = worst_of((links[i], sims[i]) for i in range(k) if i != m)
        print(f"one bad link k={k} m={m}: corrected link against the truth {d}; the others against their inputs {others}")
        assert max(d.values()) <= EXACT_BAR
        within(others, bars(ROUNDING_MEASURED), "the links without weight")
        assert sim_diff(sims[m], RF.pack(t))["rot"] > 0.05                     # ... and it was off before


def centres_error(frames, sc):
    return float(np.linalg.norm(np.asarray(frames, np.float64)[:, 10:13] - RS.true_centres(sc), axis=1).max())


@pytest.mark.parametrize("k", [6, 36])
def test_distributed_drift_brings_the_cameras_closer_to_the_truth(S, HL, FL, k):
    for seed in DRIFT_SEEDS[k]:
        sc = RS.build(k, 64, 100 + k)
        sims = RS.perturbed(sc["sims"], RS.small_similarities(k, seed))
        inp = RS.ring_input(sc, sims=sims)
        twin = RF.close_ring(inp)
        links, frames, seam, rep = RS.run_host(HL, S, inp)
        e_open_twin, e_closed_twin = centres_error(twin["open"], sc), centres_error(twin["frames"], sc)
        e_open, e_closed = centres_error(fuse_frames(FL, S, sims[:k - 1]), sc), centres_error(frames, sc)
        print(f"distributed drift k={k} seed={seed}: largest camera-centre error open {e_open:.4g} closed {e_closed:.4g} (twin {e_open_twin:.4g} / {e_closed_twin:.4g})")
        assert rep["status"] == S.RING_CLOSED
        assert e_closed_twin < e_open_twin, "the seed list holds scenes on which the twin shows it"
        assert e_closed < e_open
        assert e_closed <= 1.25 * e_closed_twin + 1e-7                         # 6f's rule


# ---- against the twin ------------------------------------------------------------------------------------------------------------
def against_twin(S, got, twin, inp, thr=4.0, flags=True):
    """Integers equal, floats measured; returns the differences.  flags: the records' membership in S is compared too, outside the
    band around the threshold, which at most BAND_CAP of them may lie in (the seam scenes are chosen for that)."""
    links, frames, seam, rep = got
    t = twin["report"]
    for f in ("status", "num_links", "first_invalid", "seam_count", "seam_lost_open", "seam_lost_closed"):
        assert rep[f] == t[f], (f, rep[f], t[f])
    d = worst_of(list(zip(links, twin["links"])) + list(zip(frames, twin["frames"])))
    d["drift"] = max(abs(rep[f] - t[f]) / max(1.0, abs(t[f])) for f in ("drift_log_scale", "drift_rotation_rad", "drift_t"))
    d["rms_px"] = max(abs(rep[f] - t[f]) / max(1.0, abs(t[f])) for f in ("seam_rms_link_px", "seam_rms_open_px", "seam_rms_closed_px"))
    assert np.array_equal(np.isfinite(seam), np.isfinite(twin["seam"]))
    fin = np.isfinite(seam)
    d["seam_px"] = float((np.abs(seam[fin] - twin["seam"][fin]) / np.maximum(1.0, twin["seam"][fin])).max()) if fin.any() else 0.0
    if flags:
        band = np.abs(twin["seam"][0] - thr) <= BAND * thr
        assert band.mean() <= BAND_CAP, band.mean()
        assert np.array_equal((seam[0] < thr)[~band], (twin["seam"][0] < thr)[~band])
    return d


def test_host_build_equals_the_twin(S, HL, closures):
    worst = dict.fromkeys(TWIN_MEASURED, 0.0)
    runs = [(f"k={k}", inp, got, twin, False) for k, (sc, inp, got, twin) in closures.items()]
    for k, n, seed in SEAM_SCENES:
        sc = RS.build(k, n, seed)
        sims = RS.perturbed(sc["sims"], RS.small_similarities(k, seed, rot=2e-4, scale=1e-3, trans=1e-3))
        inp = RS.ring_input(sc, sims=sims)
        got = RS.run_host(HL, S, inp)
        assert got[3]["seam_count"] >= n // 2, got[3]
        runs.append((f"seam k={k} n={n}", inp, got, RF.close_ring(inp), True))
    for what, inp, got, twin, flags in runs:
        d = against_twin(S, got, twin, inp, flags=flags)
        print(f"ring against the twin, {what}: {d}; report {got[3]}")
        worst = {q: max(worst[q], d[q]) for q in worst}
    within(worst, bars(TWIN_MEASURED), "against the twin")


def test_supplied_weights_follow_the_twin_and_move_only_where_they_weigh(S, HL):
    sc, inp = drifting(6, scale=0.1)
    w = np.array([0.0, 2.0, 0.0, 1.0, 1.0, 0.0], np.float32)
    got, twin = RS.run_host(HL, S, inp, weights=w), RF.close_ring(inp, weights=w)
    d = against_twin(S, got, twin, inp, flags=False)
    print(f"ring with supplied weights against the twin: {d}")
    within(d, bars(TWIN_MEASURED), "weights")
    for i in np.flatnonzero(w == 0):
        within(sim_diff(got[0][i], inp["sims"][i]), bars(ROUNDING_MEASURED), f"link {i} carries no weight")
    for i in np.flatnonzero(w > 0):
        assert sim_diff(got[0][i], inp["sims"][i])["rot"] > 1e-5, i


# ---- OPEN and REJECTED -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "inner", "closing"])
@pytest.mark.parametrize("what", ["degenerate", "s = 0", "NaN in t"])
def test_an_invalid_link_leaves_the_ring_open(S, HL, FL, what, where):
    k = 7
    sc, inp = drifting(k, scale=0.1)
    m = dict(first=0, inner=3, closing=k - 1)[where]
    sims, status = inp["sims"].copy(), inp["status"].copy()
    if what == "degenerate":
        status[m] = S.REFINE_DEGENERATE
    elif what == "s = 0":
        sims[m, 0] = 0.0
    else:
        sims[m, 11] = np.nan
    bad = dict(inp, sims=sims, status=status)
    links, frames, seam, rep = RS.run_host(HL, S, bad)
    assert rep["status"] == S.RING_OPEN and rep["first_invalid"] == m and rep["num_links"] == k
    assert (rep["drift_log_scale"], rep["drift_rotation_rad"], rep["drift_t"]) == (0.0, 0.0, 0.0)
    assert np.array_equal(u8(links), u8(sims))
    assert np.array_equal(u8(frames), u8(fuse_frames(FL, S, sims[:k - 1], status)))
    if m < k - 1:
        assert np.array_equal(frames[m + 1], FS.sim13(1.0, np.eye(3), np.zeros(3)))
    # the seam is still measured, closed = open
    assert np.array_equal(u8(seam[1]), u8(seam[2])) and rep["seam_lost_open"] == rep["seam_lost_closed"]
    assert u8(np.float32(rep["seam_rms_open_px"])).tolist() == u8(np.float32(rep["seam_rms_closed_px"])).tolist()
    twin = RF.close_ring(bad)
    for f in ("status", "first_invalid", "seam_count", "seam_lost_open", "seam_lost_closed"):
        assert rep[f] == twin["report"][f], f
    two = dict(bad, status=np.where(np.arange(k) == 5, S.REFINE_DEGENERATE, status))
    assert RS.run_host(HL, S, two)[3]["first_invalid"] == min(m, 5)


def test_either_gate_rejects_and_returns_the_links(S, HL, FL):
    k = 6
    sc = RS.build(k, 64, 100 + k)
    turned = RS.perturbed(sc["sims"], [None, None, (1.0, RS.rodrigues([0.0, 0.4, 0.0]), np.zeros(3))] + [None] * 3)
    scaled = RS.perturbed(sc["sims"], [None, (2.2, np.eye(3), np.zeros(3))] + [None] * 4)
    for what, sims, kw in (("rotation", turned, {}), ("scale", scaled, {}), ("rotation, a tighter gate", turned, dict(max_rotation_rad=0.5, max_log_scale=1.0)),
                           ("scale, a tighter gate", scaled, dict(max_rotation_rad=0.5, max_log_scale=1.0))):
        inp = RS.ring_input(sc, sims=sims)
        links, frames, seam, rep = RS.run_host(HL, S, inp, **kw)
        twin = RF.close_ring(inp, **kw)["report"]
        print(f"ring gate ({what}): status {rep['status']}, drift ln s {rep['drift_log_scale']:.4f} rot {rep['drift_rotation_rad']:.4f}")
        rejected = what in ("rotation", "scale")
        assert rep["status"] == twin["status"] == (S.RING_REJECTED if rejected else S.RING_CLOSED), what
        assert abs(rep["drift_rotation_rad"] - twin["drift_rotation_rad"]) <= 1e-6 and abs(rep["drift_log_scale"] - twin["drift_log_scale"]) <= 1e-6
        if rejected:
            assert np.array_equal(u8(links), u8(sims)) and np.array_equal(u8(frames), u8(fuse_frames(FL, S, sims[:k - 1])))
            assert np.array_equal(u8(seam[1]), u8(seam[2]))
        else:
            assert not np.array_equal(u8(links), u8(sims))
    assert abs(RS.run_host(HL, S, RS.ring_input(sc, sims=turned))[3]["drift_rotation_rad"] - 0.4) <= 1e-3
    assert abs(abs(RS.run_host(HL, S, RS.ring_input(sc, sims=scaled))[3]["drift_log_scale"]) - np.log(2.2)) <= 1e-3


def test_seam_sums_do_not_depend_on_the_block_count(S, HL):
    """1025 records are five blocks, 300 000 more than kRingMaxBlocks rounds: the counts equal the twin's either way."""
    assert [HL.ring_blocks(n) for n in (0, 1, 256, 257, 1025, 262144, 262145, 1 << 26)] == [1, 1, 1, 2, 5, 1024, 1024, 1024]
    sc = RS.build(5, 1025, 13)
    sims = RS.perturbed(sc["sims"], RS.small_similarities(5, 13, rot=2e-4, scale=1e-3, trans=1e-3))
    inp = RS.ring_input(sc, sims=sims)
    reps = 300
    L = sc["pairs"][4]
    big = dict(L, n=1025 * reps, ld=1025 * reps, points=np.tile(L["points"], (1, reps)), valid=np.tile(L["valid"], reps),
               X1=np.tile(L["X1"][:, :1025], (1, reps)))
    one, many = RS.run_host(HL, S, inp)[3], RS.run_host(HL, S, dict(inp, last=big))[3]
    assert many["seam_count"] == reps * one["seam_count"] > 0
    for f in ("seam_rms_link_px", "seam_rms_open_px", "seam_rms_closed_px"):
        assert abs(many[f] - one[f]) <= 1e-6 * one[f], f


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_struct_layouts_equal_the_ctypes_mirrors(S, HL):
    for which, cls in enumerate((S.RingParams, S.RingLinkIn, S.RingReport, S.RingOut)):
        o = (C.c_int64 * 16)()
        count = HL.ring_layout(which, o)
        assert o[0] == C.sizeof(cls) and count == len(cls._fields_), cls.__name__
        assert [o[i + 1] for i in range(count)] == [getattr(cls, f).offset for f, _ in cls._fields_], cls.__name__
    assert C.sizeof(S.RingReport) == 48


def test_header_python_and_defaults(S):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_amd.h")).read(), flags=re.S)
    for name in ("sfm_ring_default_params", "sfm_close_ring"):
        assert re.search(rf"\b{name}\s*\(", text) and name in S.EXPORTS and hasattr(S.lib(), name)
    assert "#define SFM_ABI_VERSION 3" in text and S.ABI_VERSION == 3
    assert (S.RING_CLOSED, S.RING_OPEN, S.RING_REJECTED) == (0, 1, 2)
    p = S.ring_params()
    assert (p.threshold_px, p.max_rotation_rad, p.weights, list(p.reserved)) == (4.0, np.float32(0.35), None, [0, 0, 0, 0])
    assert p.max_log_scale == np.float32(np.log(2.0))
    with pytest.raises(TypeError):
        S.ring_params(max_iterations=3)


def test_argument_checks_precede_the_device(S):
    """Everything that needs no pair: refused with SFM_E_INVALID and its text before any pointer is followed."""
    k = 4
    fake = 0x1000                                                              # never dereferenced: the checks come first
    links = (S.RingLinkIn * k)(*[S.RingLinkIn(fake, fake) for _ in range(k)])
    pair = S.FusePairIn(fake, None, None, None)
    out = S.RingOut(fake, fake, None, fake)

    def refused(ctx=fake, lk=links, count=k, last=pair, p=None, o=out):
        p = S.ring_params() if p is None else p
        rc = S.lib().sfm_close_ring(ctx, lk, count, C.byref(last) if last is not None else None, C.byref(p) if p is not False else None,
                                    C.byref(o) if o is not None else None)
        assert rc == S.E_INVALID
        return S.lib().sfm_last_error().decode()
    assert "null params" in refused(p=False)
    assert "num_links 2 outside 3..4096" in refused(count=2)
    assert "num_links 4097" in refused(count=4097)
    assert "null context" in refused(ctx=None) and "null context" in refused(last=None) and "null context" in refused(o=None)
    assert "null context" in refused(lk=None)
    holes = (S.RingLinkIn * k)(*[S.RingLinkIn(fake, fake if i != 2 else None) for i in range(k)])
    assert "links[2]: d_sim and d_report are required" in refused(lk=holes)
    assert "last_pair: null pair" in refused(last=S.FusePairIn(None, None, None, None))
    assert "last_pair: d_valid needs d_points" in refused(last=S.FusePairIn(fake, None, fake, None))
    assert "every buffer of sfm_ring_out but d_seam_err is required" in refused(o=S.RingOut(fake, None, None, fake))
    assert "reserved" in refused(p=S.ring_params(reserved=[0, 0, 1, 0]))
    for bad in (0.0, -0.1, 1.6, float("nan")):
        assert "max_rotation_rad" in refused(p=S.ring_params(max_rotation_rad=bad))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert "max_log_scale" in refused(p=S.ring_params(max_log_scale=bad))
    for bad in (0.0, -4.0, float("nan")):
        assert "threshold_px" in refused(p=S.ring_params(threshold_px=bad))
    assert "links[1]: its weight" in refused(p=S.ring_params(weights=[1, -1, 1, 1]))
    assert "links[3]: its weight" in refused(p=S.ring_params(weights=[1, 1, 1, float("nan")]))
    assert "positive sum" in refused(p=S.ring_params(weights=[0, 0, 0, 0]))


def test_kernels_use_no_scratch():
    """The compiler's resource report of ring.hip (build/ring.usage.txt, written by the Makefile's object rule): no kernel uses
    scratch; the registers and LDS are recorded in DESIGN 6j."""
    assert os.path.exists(USAGE), f"{USAGE} is missing: make builds it"
    text = open(USAGE).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    kernels = ("ring_walk_kernel", "ring_correct_kernel", "ring_seam_kernel")
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == len(kernels)
    for name, kernel, sc, v, l in zip(names, kernels, scratch, vgprs, lds):
        assert kernel in name and sc == 0 and v <= 128 and l <= 32768, (name, sc, v, l)
    print({k: (v, l) for k, v, l in zip(kernels, vgprs, lds)})
