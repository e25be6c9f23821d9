"""CPU: sfm_fuse_ring without a device -- the host build (tests/hostcheck/libfuseringcheck.so: fuse_ring_math.hpp's functions, the
nodes visited serially) against the fp64 twin (tests/fuse_ring_reference.py), against sfm_fuse_chain's host build
(libfusecheck.so) and against ground truth: the track table and the report on six rings, the join rule on hand-made rings, OPEN
and REJECTED byte for byte, exact and noisy points, the gain at the seam, sfm_adjust_chain's host build over the ring's table;
struct layouts, header / exports / Python mirror / INTEGRATION.md, the argument checks that precede the device, and the compiler's
resource report of fuse_ring.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chain_adjust_reference as CR
import chain_adjust_scene as CS
import fuse_reference as FR
import fuse_ring_reference as RR
import fuse_ring_scene as RS
import fuse_scene as FS
import ring_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "build", "fuse_ring.usage.txt")
NAMES = ["sfm_fuse_ring_default_params", "sfm_fuse_ring"]
INTS = ("status", "first_invalid", "seam_proposals", "seam_ineligible", "seam_tracks", "seam_refined", "seam_kept")
EXACT_BAR = 1e-4                                      # fused point against the truth, relative to its depth (6h's bar)
BAND = 0.10                                           # flags are compared outside this share of the threshold ...
BAND_CAP = 0.01                                       # ... which at most this share of the tracks may lie in
# The noisy rings whose flags, points and errors are held to the twin: all six checked rings (fuse_ring_scene.RINGS, seeds 7, 7, 7,
# 61, 5, 3).  On each the TWIN alone keeps at most BAND_CAP of its tracks within BAND of the threshold: 0 / 408, 3 / 473, 1 / 625,
# 4 / 2305, 0 / 140 and 5 / 784 tracks.
NOISY = list(RS.RINGS)
# Host build (fp32) against the twin (fp64) on the tracks outside the band, MEASURED over NOISY: points 1.11e-5 of max(1, depth) (on
# (36, 65, 3), whose frames are composed over 35 links), errors 1.46e-2 relative above 1 px (on (6, 1024, 61), on a kept track whose
# LM result lies hundreds of pixels off).  The bars are 4 x these.
POINTS_MEASURED, ERR_MEASURED = 1.11e-5, 1.46e-2
POINTS_BAR, ERR_BAR = 4.0 * POINTS_MEASURED, 4.0 * ERR_MEASURED


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


@pytest.fixture(scope="module")
def HC():
    return FS.host_lib()


@pytest.fixture(scope="module")
def runs(S, HL):
    """Per checked ring: the scene, its ring chain, the host build's result and the twin's, computed once."""
    out = {}
    for key in RS.RINGS:
        sc, ring = RS.build(*key)
        out[key] = (sc, ring, RS.run_host(HL, S, ring), RR.fuse(ring))
    return out


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def structure_equal(got, want):
    for k in ("track", "track_offset", "obs_cam", "obs_record", "root"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("tracks", "observations", "segments", "longest_track"):
        assert got["counts"][k] == want["counts"][k], (k, got["counts"], want["counts"])
    for f in ("status", "first_invalid", "seam_proposals", "seam_ineligible", "seam_tracks"):
        assert got["report"][f] == want["report"][f], (f, got["report"], want["report"])


def offsets(ring):
    return np.concatenate([[0], np.cumsum([P["n"] for P in ring["pairs"]])]).astype(int)


def seam_tracks(res):
    first = res["obs_cam"][res["track_offset"][:-1]] >> 1
    last = res["obs_cam"][res["track_offset"][1:] - 1] >> 1
    return first > last


# ---- the six rings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", RS.RINGS)
def test_track_structure_and_report_equal_the_twin(runs, key):
    sc, ring, got, want = runs[key]
    k = len(ring["pairs"])
    structure_equal(got, want)
    r = got["report"]
    assert r["status"] == RR.CLOSED and r["first_invalid"] == -1
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == RS.EXPECTED[key]
    assert r["seam_refined"] + r["seam_kept"] == r["seam_tracks"]
    assert abs(r["closure_log_scale"]) <= 1e-6 and r["closure_rotation_rad"] <= 1e-6 and r["closure_t"] <= 1e-5
    # the table is consistent in itself: every live node in exactly one track, the pairs of a track step modulo k, no track has more
    # than k pairs, a track crosses the seam at most once, seam tracks and only they carry the seam flags
    off = offsets(ring)
    seen = np.zeros(off[-1], int)
    seam = seam_tracks(got)
    assert seam.sum() == r["seam_tracks"] and np.array_equal(seam, want["seam"])
    assert np.array_equal(np.isin(got["flags"], (RR.SEAM_REFINED, RR.SEAM_KEPT)), seam)
    heads = []
    for t in range(got["counts"]["tracks"]):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1])
        cam = got["obs_cam"][o]
        L = len(o) - 1
        assert 1 <= L <= k and np.array_equal(cam[:-1] >> 1, ((cam[0] >> 1) + np.arange(L)) % k) and cam[-1] == cam[-2] + 1 and (cam[:-1] & 1 == 0).all()
        assert got["obs_record"][o[-1]] == got["obs_record"][o[-2]]
        assert int((np.diff(cam[:-1] >> 1) < 0).sum()) == int(seam[t])
        nodes = off[cam[:-1] >> 1] + got["obs_record"][o[:-1]]
        assert (got["track"][nodes] == t).all()
        seen[nodes] += 1
        heads.append(nodes[0])
    assert heads == sorted(heads)                              # numbered by head: pair, then record
    live = np.concatenate([FR.live_nodes(P) for P in ring["pairs"]])
    assert np.array_equal(seen, live.astype(int)) and np.array_equal(got["track"] >= 0, live)
    assert got["counts"]["observations"] == live.sum() + got["counts"]["tracks"]
    assert got["counts"]["refined"] + got["counts"]["kept"] == got["counts"]["tracks"]
    assert got["counts"]["refined"] == np.isin(got["flags"], (RR.REFINED, RR.SEAM_REFINED)).sum()
    assert r["seam_refined"] == (got["flags"] == RR.SEAM_REFINED).sum() and r["seam_kept"] == (got["flags"] == RR.SEAM_KEPT).sum()
    print(f"fuse ring {key}: {got['counts']}, {r}")


def test_closed_ring_keeps_the_chains_frames_roots_and_cameras(S, HL, HC, runs):
    for key in RS.RINGS:
        sc, ring, got, _ = runs[key]
        chain = FS.run_host(HC, S, RS.open_chain(ring))
        for name in ("frames", "root", "cams"):
            assert np.array_equal(u8(got[name]), u8(chain[name])), (key, name)
        # every join takes one head away: T falls by the joins, the observations by as many (A's slot-1 observation of view 0)
        assert chain["counts"]["tracks"] - got["counts"]["tracks"] == got["report"]["seam_tracks"]
        assert chain["counts"]["observations"] - got["counts"]["observations"] == got["report"]["seam_tracks"]


# ---- the join rule on hand-made rings ----------------------------------------------------------------------------------------------
def mini(k, n=8, sizes=None):
    """k pairs of n records (or sizes[i]), every point usable, identity links without a single edge."""
    K, Kinv = ring_scene.AS.camera()
    rng = np.random.default_rng(k)
    pairs, links = [], []
    for i in range(k):
        m = n if sizes is None else sizes[i]
        ld = 128
        X = np.full((3, ld), np.nan, np.float32)
        X[:, :m] = np.stack([rng.uniform(-0.1, 0.1, m), rng.uniform(-0.1, 0.1, m), np.ones(m)]).astype(np.float32)
        pts = np.ascontiguousarray(np.stack([X[0, :m] * 5, X[1, :m] * 5, np.full(m, 5.0), np.ones(m)]).astype(np.float32))
        pairs.append(dict(n=m, ld=ld, points=pts, valid=np.ones(m, np.uint8), X0=X, X1=X.copy(),
                          pose=np.concatenate([np.eye(3).ravel(), [0.0, 0.0, 0.0]]).astype(np.float32)))
        links.append(dict(index=np.full(m, -1, np.int32), sim=FS.sim13(1.0, np.eye(3), np.zeros(3)), inlier=np.zeros(m, np.uint8),
                          err=np.full(m, 0.25, np.float32), status=0))
    return dict(K=K, Kinv=Kinv, pairs=pairs, links=links)


def edge(ring, i, j, m, err=0.25):
    L = ring["links"][i]
    L["index"][j] = m; L["inlier"][j] = 1; L["err"][j] = err


def both(S, HL, ring):
    got = RS.run_host(HL, S, ring, max_iterations=0)
    structure_equal(got, RR.fuse(ring, max_iterations=0))
    assert got["report"]["status"] == RR.CLOSED
    return got


def track_of(got, ring, pair, rec):
    return int(got["track"][offsets(ring)[pair] + rec])


def observations(got, t):
    o = slice(got["track_offset"][t], got["track_offset"][t + 1])
    return list(zip(got["obs_cam"][o].tolist(), got["obs_record"][o].tolist()))


def test_the_join_needs_len_b_below_h_a(S, HL):
    # A = (2, 0) -> (3, 1), h_A = 2; it proposes (0, 4)
    ring = mini(4)
    edge(ring, 2, 0, 1); edge(ring, 3, 1, 4)
    edge(ring, 0, 4, 6)                                       # B = (0, 4) -> (1, 6): len(B) = 2 = h_A
    got = both(S, HL, ring)
    r = got["report"]
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == (1, 1, 0)
    assert track_of(got, ring, 3, 1) != track_of(got, ring, 0, 4) and not seam_tracks(got).any()
    assert observations(got, track_of(got, ring, 3, 1)) == [(4, 0), (6, 1), (7, 1)]
    ring = mini(4)
    edge(ring, 2, 0, 1); edge(ring, 3, 1, 4)                  # B = (0, 4) alone: len(B) = 1 = h_A - 1
    got = both(S, HL, ring)
    r = got["report"]
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == (1, 0, 1)
    t = track_of(got, ring, 2, 0)
    assert t == track_of(got, ring, 3, 1) == track_of(got, ring, 0, 4)
    # X0 of every record in path order, then X1 of B's last record: views 2, 3, 0, 1
    assert observations(got, t) == [(4, 0), (6, 1), (0, 4), (1, 4)] and got["flags"][t] in (RR.SEAM_REFINED, RR.SEAM_KEPT)
    assert got["counts"]["tracks"] == 4 * 8 - 2 and got["counts"]["longest_track"] == 4
    # h_A = 3 against len(B) = 2 joins; the joined track has k - 1 pairs
    ring = mini(4)
    edge(ring, 3, 1, 4); edge(ring, 0, 4, 6)
    got = both(S, HL, ring)
    assert got["report"]["seam_tracks"] == 1 and observations(got, track_of(got, ring, 3, 1)) == [(6, 1), (0, 4), (2, 6), (3, 6)]


def test_the_full_cycle_stays_one_chain_track(S, HL):
    ring = mini(3)
    edge(ring, 0, 2, 3); edge(ring, 1, 3, 5); edge(ring, 2, 5, 2)       # round the ring to its own record: A = B, h_A = 0
    got = both(S, HL, ring)
    r = got["report"]
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == (1, 1, 0)
    t = track_of(got, ring, 0, 2)
    assert observations(got, t) == [(0, 2), (2, 3), (4, 5), (5, 5)] and got["flags"][t] in (RR.REFINED, RR.KEPT)
    assert got["counts"]["longest_track"] == 4
    # ... and so does a cycle that comes back to ANOTHER record of pair 0: len(B) = 1 is not below h_A = 0
    ring = mini(3)
    edge(ring, 0, 2, 3); edge(ring, 1, 3, 5); edge(ring, 2, 5, 7)
    got = both(S, HL, ring)
    assert got["report"]["seam_ineligible"] == 1 and track_of(got, ring, 0, 7) != track_of(got, ring, 0, 2)


@pytest.mark.parametrize("recs,errs,winner", [([1, 5], [0.5, 0.25], 5), ([1, 5], [0.25, 0.25], 1), ([1, 3, 5], [0.5, 0.125, 0.25], 3),
                                              ([1, 3, 5], [0.25, 0.25, 0.25], 1), ([1, 3, 5], [0.25, 0.5, 0.25], 1)])
def test_contests_go_to_the_smallest_error_then_the_lowest_record(S, HL, recs, errs, winner):
    ring = mini(4)
    for j, e in zip(recs, errs):
        edge(ring, 3, j, 6, e)                                # every proposer heads its own track in pair 3: h_A = 3
    got = both(S, HL, ring)
    r = got["report"]
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == (len(recs), 0, 1)
    t = track_of(got, ring, 0, 6)
    assert track_of(got, ring, 3, winner) == t and observations(got, t) == [(6, winner), (0, 6), (1, 6)]
    for j in recs:
        if j != winner:                                       # a loser keeps its own track: one pair, two observations
            assert observations(got, track_of(got, ring, 3, j)) == [(6, j), (7, j)]


def test_an_ineligible_proposer_never_blocks_an_eligible_one(S, HL):
    ring = mini(4)
    edge(ring, 1, 0, 0); edge(ring, 2, 0, 1)                  # A1 = (1, 0) -> (2, 0) -> (3, 1): h_A = 1, not above len(B) = 1
    edge(ring, 3, 1, 6, 0.01)                                 # ... with the smallest error
    edge(ring, 3, 2, 6, 0.5)                                  # A2 = (3, 2): h_A = 3
    got = both(S, HL, ring)
    r = got["report"]
    assert (r["seam_proposals"], r["seam_ineligible"], r["seam_tracks"]) == (2, 1, 1)
    assert track_of(got, ring, 3, 2) == track_of(got, ring, 0, 6) != track_of(got, ring, 3, 1)
    assert observations(got, track_of(got, ring, 3, 1)) == [(2, 0), (4, 0), (6, 1), (7, 1)]


def test_what_gives_no_edge_at_the_seam(S, HL):
    def one(change):
        ring = mini(4)
        edge(ring, 3, 1, 6)
        change(ring)
        got = both(S, HL, ring)
        assert got["report"]["seam_proposals"] == 0 and got["report"]["seam_tracks"] == 0 and not seam_tracks(got).any()
        return got
    one(lambda r: r["links"][3]["index"].__setitem__(1, 8))             # one past the end
    one(lambda r: r["links"][3]["index"].__setitem__(1, -1))
    one(lambda r: r["links"][3]["inlier"].__setitem__(1, 0))
    one(lambda r: r["links"][3]["err"].__setitem__(1, np.nan))
    one(lambda r: r["links"][3]["err"].__setitem__(1, np.inf))
    got = one(lambda r: r["pairs"][3]["valid"].__setitem__(1, 0))       # the proposer is dead
    assert got["track"][3 * 8 + 1] == -1
    got = one(lambda r: r["pairs"][0]["points"].__setitem__((2, 6), -1.0))      # the target lies behind its camera
    assert got["track"][6] == -1


def test_a_ring_whose_first_or_last_pair_has_no_records(S, HL):
    for sizes in ([0, 8, 8, 8], [8, 8, 8, 0], [0, 8, 8, 0]):
        ring = mini(4, sizes=sizes)
        if sizes[1] and sizes[2]:
            edge(ring, 1, 2, 3)
        if sizes[3]:
            edge(ring, 2, 3, 1); edge(ring, 3, 1, 0)          # an index into the empty pair 0: out of range
        if sizes[0]:
            edge(ring, 0, 1, 1)
        got = both(S, HL, ring)
        assert got["report"]["seam_proposals"] == 0 and got["counts"]["tracks"] > 0, sizes


# ---- OPEN and REJECTED -------------------------------------------------------------------------------------------------------------
def with_link(ring, i, **change):
    return dict(ring, links=[dict(L, **change) if q == i else L for q, L in enumerate(ring["links"])])


def equals_the_chain(S, HC, ring, got, what):
    """Every array of sfm_fuse_out as sfm_fuse_chain's host build leaves it over the k pairs and the first k - 1 links: the written
    parts byte for byte, and nothing written behind them (both start from zeroed arrays)."""
    chain = FS.run_host(HC, S, RS.open_chain(ring))
    for name in ("frames", "root", "cams", "track", "track_offset", "obs_cam", "obs_record", "points", "flags", "err"):
        assert np.array_equal(u8(got[name]), u8(chain[name])), (what, name)
    assert got["counts"] == chain["counts"], what
    T, M, N = got["counts"]["tracks"], got["counts"]["observations"], int(offsets(ring)[-1])
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = got["raw"]
    assert not off[T + 1:].any() and not ocam[M:].any() and not orec[M:].any() and not pts.reshape(4, N)[:, T:].any()
    assert not flags[T:].any() and not err[T:].any() and not counts[6:].any()
    assert not seam_tracks(got).any()


def test_open_and_rejected_rings_are_the_chains_bytes(S, HL, HC, runs):
    sc, ring, closed, _ = runs[(6, 257, 7)]
    k = 6
    for i in (0, 2, k - 1):
        nan_t = ring["links"][i]["sim"].copy(); nan_t[11] = np.nan
        zero_s = ring["links"][i]["sim"].copy(); zero_s[0] = 0.0
        for name, change in (("degenerate", dict(status=S.REFINE_DEGENERATE)), ("s = 0", dict(sim=zero_s)), ("NaN in t", dict(sim=nan_t))):
            broken = with_link(ring, i, **change)
            got = RS.run_host(HL, S, broken)
            r = got["report"]
            assert r["status"] == RR.OPEN and r["first_invalid"] == i, (i, name, r)
            assert (r["closure_log_scale"], r["closure_rotation_rad"], r["closure_t"]) == (0.0, 0.0, 0.0)
            assert all(r[f] == 0 for f in INTS[2:]), r
            equals_the_chain(S, HC, broken, got, (i, name))
            twin = RR.fuse(broken, max_iterations=0)
            assert twin["report"]["status"] == RR.OPEN and twin["report"]["first_invalid"] == i
            assert got["counts"]["segments"] == (1 if i == k - 1 else 2)
    both_bad = with_link(with_link(ring, 4, status=S.REFINE_DEGENERATE), 1, status=S.REFINE_DEGENERATE)
    assert RS.run_host(HL, S, both_bad)["report"]["first_invalid"] == 1
    # REJECTED by either gate, CLOSED under wider ones
    turn = ring_scene.compose((1.0, ring_scene.rodrigues([0.0, 5e-3, 0.0]), np.zeros(3)), ring_scene.unpack(ring["links"][k - 1]["sim"]))
    grow = ring_scene.compose((np.exp(5e-3), np.eye(3), np.zeros(3)), ring_scene.unpack(ring["links"][k - 1]["sim"]))
    for name, sim, wide in (("rotation", turn, dict(max_closure_rotation_rad=1e-2)), ("scale", grow, dict(max_closure_log_scale=1e-2))):
        off_ring = with_link(ring, k - 1, sim=FS.sim13(*sim))
        got = RS.run_host(HL, S, off_ring)
        r = got["report"]
        assert r["status"] == RR.REJECTED and r["first_invalid"] == -1 and all(r[f] == 0 for f in INTS[2:]), (name, r)
        want = 5e-3
        assert abs((r["closure_rotation_rad"] if name == "rotation" else abs(r["closure_log_scale"])) - want) <= 1e-5, (name, r)
        assert (r["closure_log_scale"] if name == "rotation" else r["closure_rotation_rad"]) <= 1e-5
        equals_the_chain(S, HC, off_ring, got, name)
        assert RR.fuse(off_ring, max_iterations=0)["report"]["status"] == RR.REJECTED
        wider = RS.run_host(HL, S, off_ring, **wide)
        assert wider["report"]["status"] == RR.CLOSED and wider["report"]["seam_tracks"] == closed["report"]["seam_tracks"], name
        structure_equal(wider, RR.fuse(off_ring, max_iterations=0, **wide))
        # the other gate does not help
        other = dict(max_closure_log_scale=1e-2) if name == "rotation" else dict(max_closure_rotation_rad=1e-2)
        assert RS.run_host(HL, S, off_ring, **other)["report"]["status"] == RR.REJECTED


# ---- points --------------------------------------------------------------------------------------------------------------------
def head_feature(sc, res, t):
    o = res["track_offset"][t]
    return RS.feature(sc, res["obs_cam"][o] >> 1, res["obs_record"][o])


def test_exact_ring_recovers_the_seam_tracks_points(S, HL):
    """No noise, no wrong matches, no wrong indices -- but a fifth of every link's matches missed, without which every feature goes
    round the whole ring and nothing is left to join."""
    sc, ring = RS.build(6, 512, 11, noise_px=0.0, wrong_match=0.0, wrong_index=0.0)
    rng = np.random.default_rng(11)
    for L in ring["links"]:
        L["inlier"][rng.random(len(L["inlier"])) < 0.2] = 0
    got = RS.run_host(HL, S, ring)
    seam = np.flatnonzero(seam_tracks(got))
    truth = RS.truth_in_pair0(sc, [head_feature(sc, got, t) for t in range(got["counts"]["tracks"])])
    d = np.linalg.norm(got["points"][:3].T.astype(np.float64) - truth, axis=1) / truth[:, 2]
    print(f"fuse ring, exact: {got['counts']}, {got['report']}; |X - truth| / depth: seam tracks {d[seam].max():.3g}, all {d.max():.3g}")
    assert len(seam) >= 100 and (got["flags"][seam] == RR.SEAM_REFINED).all() and got["report"]["seam_kept"] == 0
    assert d[seam].max() <= EXACT_BAR and d.max() <= EXACT_BAR


@pytest.mark.parametrize("key", NOISY)
def test_noisy_rings_against_the_twin(runs, key):
    sc, ring, got, want = runs[key]
    thr = 4.0
    band = np.abs(want["err"] - thr) <= BAND * thr
    print(f"fuse ring {key}: refined / kept {got['counts']['refined']} / {got['counts']['kept']} (twin {want['counts']['refined']} / "
          f"{want['counts']['kept']}), seam {got['report']['seam_refined']} / {got['report']['seam_kept']}, {band.sum()} of {len(band)} tracks within "
          f"{BAND:.0%} of the threshold")
    assert band.mean() <= BAND_CAP
    same = ~band
    assert np.array_equal(got["flags"][same], want["flags"][same])
    scale = np.maximum(1.0, np.abs(want["points"][2]))
    d = np.abs(got["points"].astype(np.float64) - want["points"])[:3].max(0) / scale
    fin = np.isfinite(want["err"]) & same
    assert np.array_equal(np.isfinite(got["err"][same]), np.isfinite(want["err"][same]))
    de = np.abs(got["err"][fin].astype(np.float64) - want["err"][fin]) / np.maximum(1.0, want["err"][fin])
    print(f"  against the twin: points {d[same].max():.3g} relative to depth, err {de.max():.3g}")
    assert d[same].max() <= POINTS_BAR and de.max() <= ERR_BAR


def twice_and_once(sc, ring, chain, res):
    """The features the chain fusion holds twice and the ring fusion once: per seam track of `res` whose records all observe one
    true feature through good matches, (ring track, chain track of its A side, chain track of its B side)."""
    off = offsets(ring)
    out = []
    for t in np.flatnonzero(seam_tracks(res)):
        o = np.arange(res["track_offset"][t], res["track_offset"][t + 1] - 1)
        pairs, recs = res["obs_cam"][o] >> 1, res["obs_record"][o]
        ids = {RS.feature(sc, p, r) for p, r in zip(pairs, recs)}
        if len(ids) != 1 or not all(sc["pairs"][p]["good"][r] for p, r in zip(pairs, recs)):
            continue
        a, b = chain["track"][off[pairs[0]] + recs[0]], chain["track"][off[0] + recs[np.flatnonzero(pairs == 0)[0]]]
        assert a >= 0 and b >= 0 and a != b
        out.append((t, a, b, ids.pop()))
    return out


def seam_gain(sc, ring, chain, res):
    """Median distance to the truth of the ring's point and of the midpoint of the chain's two copies, over twice_and_once's
    features whose three tracks are all refined."""
    rows = [(t, a, b, f) for t, a, b, f in twice_and_once(sc, ring, chain, res)
            if res["flags"][t] == RR.SEAM_REFINED and chain["flags"][a] == FR.REFINED and chain["flags"][b] == FR.REFINED]
    if not rows:
        return 0, np.nan, np.nan
    t, a, b, f = (np.array(c) for c in zip(*rows))
    truth = RS.truth_in_pair0(sc, f)
    one = np.linalg.norm(np.asarray(res["points"], np.float64)[:3, t].T - truth, axis=1)
    cp = np.asarray(chain["points"], np.float64)
    two = np.linalg.norm(0.5 * (cp[:3, a] + cp[:3, b]).T - truth, axis=1)
    return len(rows), float(np.median(one)), float(np.median(two))


@pytest.mark.parametrize("key", [(6, 257, 7), (6, 1024, 61), (36, 65, 3)])
def test_gain_at_the_seam(S, HC, runs, key):
    """One point from all the views of a feature against the mean of the two points the chain fusion leaves: in the twin first;
    the host build is held to 1.25 x the twin only where the twin shows the gain."""
    sc, ring, got, want = runs[key]
    open_ring = RS.open_chain(ring)
    n_t, one_t, two_t = seam_gain(sc, ring, FR.fuse(open_ring), want)
    n_h, one_h, two_h = seam_gain(sc, ring, FS.run_host(HC, S, open_ring), got)
    print(f"fuse ring {key}: {n_t} features held twice by the chain and once by the ring; median distance to the truth: twin ring {one_t:.4g} "
          f"against midpoint {two_t:.4g}; host build ring {one_h:.4g} against midpoint {two_h:.4g}" +
          ("" if one_t < two_t else "   (the twin shows no gain: nothing asserted)"))
    assert n_t >= 8
    if one_t < two_t:
        assert n_h >= 8 and one_h <= 1.25 * one_t


# ---- sfm_adjust_chain over the ring's table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(6, 257, 7), (5, 257, 7)])
def test_adjust_chain_leaves_the_seam_tracks_alone(S, HL, runs, key):
    """libchainadjustcheck over the host build's ring table: seam tracks unused and their columns returned bit for bit, every block
    index of a used track in range, the rest against chain_adjust_reference within 6i's bars.  (5, 257, 7) is the table the device
    test hands to sfm_adjust_chain."""
    import test_chain_adjust_host as TC
    if key in runs:
        sc, ring, got, _ = runs[key]
    else:
        sc, ring = RS.build(*key)
        got = RS.run_host(HL, S, ring)
    k, N = key[0], key[0] * key[1]
    HA = CS.host_lib()
    res = {name: got[name] for name in ("root", "cams", "track_offset", "obs_cam", "obs_record", "points", "flags", "counts")}
    fused = CS.fused_arrays(res, k, N)
    host = CS.run_host(HA, S, ring, fused)
    twin = CR.adjust_chain(ring["pairs"], ring["K"], res)
    seam = seam_tracks(got)
    assert seam.sum() == got["report"]["seam_tracks"] >= 60 and not host["used"][seam].any() and not twin["used"][seam].any()
    assert np.array_equal(u8(host["points"][:, seam]), u8(got["points"][:, seam]))
    assert np.array_equal(host["used"] != 0, twin["used"]) and host["used"].sum() > 100
    for t in np.flatnonzero(host["used"]):
        cam = got["obs_cam"][got["track_offset"][t]:got["track_offset"][t + 1]]
        blocks = [(c >> 1) if c & 1 else ((c >> 1) - 1 if got["root"][c >> 1] != (c >> 1) else -1) for c in cam]
        assert min(blocks) >= -1 and max(blocks) <= k - 1 and blocks == list(range(blocks[0], blocks[0] + len(blocks))), (t, blocks)
    rt, rh = twin["reports"][0], host["reports"][0]
    for f in ("num_cameras", "num_tracks", "num_observations", "num_over_long"):
        assert rh[f] == rt[f], (f, rh[f], rt[f])
    assert rh["status"] != CR.DEGENERATE and rh["final_rms_px"] < rh["initial_rms_px"]
    cams = host["cams"].astype(np.float64)
    drot = max(CS.rotation_angle(cams[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(k))
    dt = float(np.abs(cams[:, 1, 9:] - twin["cams"][:, 1, 9:]).max())
    drms = abs(float(rh["final_rms_px"]) - rt["final_rms_px"])
    print(f"adjust_chain over the ring table {key}: {int(seam.sum())} seam tracks, {rh['num_tracks']} used tracks, rms {rt['initial_rms_px']:.4f} -> {rt['final_rms_px']:.4f} px; "
          f"host - twin: rot {drot:.3g} rad, t {dt:.3g}, rms {drms:.3g} px")
    assert drot <= TC.BAR_ROT and dt <= TC.BAR_T and drms <= TC.BAR_RMS


# ---- layouts, documents, argument checks, resources --------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(S, HL):
    for which, T in enumerate((S.FuseRingParams, S.FuseRingReport)):
        out = (C.c_int64 * 16)()
        nf = HL.fuse_ring_layout(which, out)
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
    assert re.search(r"#define\s+SFM_FUSE_SEAM_REFINED\s+3\b", hdr) and re.search(r"#define\s+SFM_FUSE_SEAM_KEPT\s+4\b", hdr)
    for f in ("fuse_ring_params", "fuse_ring", "fuse_ring_enqueue"):
        assert callable(getattr(S, f)), f
    assert (S.FUSE_SEAM_REFINED, S.FUSE_SEAM_KEPT) == (3, 4) == (RR.SEAM_REFINED, RR.SEAM_KEPT)
    p = S.fuse_ring_params()
    assert (p.fuse.threshold_px, p.fuse.max_iterations, p.fuse.huber_px) == (4.0, 5, 1.0)
    assert p.max_closure_rotation_rad == np.float32(1e-3) and p.max_closure_log_scale == np.float32(1e-3) and not any(p.reserved)
    assert S.fuse_ring_params(max_iterations=7, max_closure_log_scale=0.5).fuse.max_iterations == 7
    with pytest.raises(TypeError):
        S.fuse_ring_params(num_hypotheses=4)


def test_argument_checks_come_before_any_device_call(S):
    call, ref = S.lib().sfm_fuse_ring, C.byref
    p = S.fuse_ring_params()
    pin = (S.FusePairIn * 3)(*[S.FusePairIn(None, None, None, None)] * 3)           # null pairs: refused before any pair is read
    full = lambda: (S.FuseLinkIn * 3)(*[S.FuseLinkIn(0x100, 0x200, 0x300, 0x400, 0x500)] * 3)
    lin = full()
    out = S.FuseOut(*[0x1000 * (i + 2) for i in range(11)])
    ctx, rep = C.c_void_p(0x7000), C.c_void_p(0x9000)                              # never dereferenced
    err = lambda: S.lib().sfm_last_error()
    assert call(ctx, pin, 3, lin, None, ref(out), rep) == S.E_INVALID
    for k in (-1, 0, 1, 2, 4097):
        assert call(ctx, pin, k, lin, ref(p), ref(out), rep) == S.E_INVALID and b"3..4096" in err(), k
    for args in ((None, pin, 3, lin, ref(p), ref(out), rep), (ctx, None, 3, lin, ref(p), ref(out), rep), (ctx, pin, 3, None, ref(p), ref(out), rep),
                 (ctx, pin, 3, lin, ref(p), None, rep), (ctx, pin, 3, lin, ref(p), ref(out), None)):
        assert call(*args) == S.E_INVALID and b"null" in err()
    for i, (f, _) in enumerate(S.FuseOut._fields_):
        if f == "d_err":
            continue
        o = S.FuseOut(*[None if q == i else 0x1000 * (q + 2) for q in range(11)])
        assert call(ctx, pin, 3, lin, ref(p), ref(o), rep) == S.E_INVALID and b"required" in err(), f
    for i in range(3):                                                            # every one of the k links, the closing one too
        for f, _ in S.FuseLinkIn._fields_:
            lk = full()
            setattr(lk[i], f, None)
            assert call(ctx, pin, 3, lk, ref(p), ref(out), rep) == S.E_INVALID and f"links[{i}]".encode() in err(), (i, f)
    for kw in (dict(reserved=[0, 1, 0, 0]), dict(fuse_reserved=[0, 0, 1, 0]), dict(max_closure_rotation_rad=0.0), dict(max_closure_rotation_rad=1.6),
               dict(max_closure_rotation_rad=float("nan")), dict(max_closure_log_scale=0.0), dict(max_closure_log_scale=float("inf")),
               dict(max_closure_log_scale=float("nan")), dict(threshold_px=0.0), dict(threshold_px=float("nan")), dict(max_iterations=-1),
               dict(max_iterations=51), dict(huber_px=-1.0), dict(min_rel_decrease=float("inf")), dict(initial_lambda=-1.0)):
        assert call(ctx, pin, 3, lin, ref(S.fuse_ring_params(**kw)), ref(out), rep) == S.E_INVALID, kw
    assert call(ctx, pin, 3, lin, ref(p), ref(out), rep) == S.E_INVALID and b"pairs[0]" in err()        # what is left: the null pair


def test_kernels_use_no_scratch():
    """The compiler's resource report of fuse_ring.hip (build/fuse_ring.usage.txt, written by the Makefile's object rule): its six
    kernels, no scratch in any, the node kernels' LDS is their scan's wave sums; fuse.hip keeps its own seven."""
    assert os.path.exists(USAGE), "run `make`: the product build leaves the compiler's resource report next to the objects"
    text = open(USAGE).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    kernels = ("closure", "edges", "links", "count", "fill", "points")
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == len(kernels), names
    for name, kernel, sc, v, l in zip(names, kernels, scratch, vgprs, lds):
        print(f"fuse_ring_{kernel}: {v} VGPRs, LDS {l}, scratch {sc}")
        assert f"fuse_ring_{kernel}_kernel" in name and sc == 0 and v <= 128 and l <= 128, (name, sc, v, l)
    chain = re.findall(r"Function Name: (\S+)", open(os.path.join(ROOT, "build", "fuse.usage.txt")).read())
    assert len(chain) == 7 and not any("ring" in n for n in chain)
