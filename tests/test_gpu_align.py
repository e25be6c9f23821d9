"""GPU: sfm_align_pair (csrc/align.hip) through the C ABI -- every output against the host build of the same arithmetic
(tests/hostcheck/libaligncheck.so), which differs from the kernels only in the order of the fp64 sums of the refinement;
determinism, nothing in either pair changed, every refusal with nothing written; the full chain on the device against the truth
and the fp64 twin; the dino frames 0, 1, 2."""
import ctypes as C

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV, to_dev
import align_reference as AR
import align_scene as AS
import refine_reference as RR
import view_points_scene as VS
from test_align_host import ROT_BAR, T_BAR, S_BAR

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
CANDIDATES = [3, 4, 63, 64, 65, 257, 1024, 1025]         # 1025: the smallest count with a second scoring tile
HYPOTHESES = [1, 256, 4096]
# Kernel against host build at 10 iterations: the two differ only in the order of the fp64 sums of the system and of the costs (a
# thread's stride, wave butterflies and wave order against candidate order).  MEASURED: the largest difference over the 24 cases
# below on the MI355X -- relative in s, rotation angle (rad), |dt| / |t|, largest |err - err'| / max(1, err'), rms (px), cost
# (relative).  Every one is 0 on all 24 cases, so the bars, 4 x the measured maximum, are equality.
MEASURED = dict(s=0.0, rot=0.0, t=0.0, err=0.0, rms=0.0, cost=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def HL():
    return AS.host_lib()


@pytest.fixture(scope="module")
def scene():
    """1536 records, 0.5 px noise, 15 % wrong matches on each side, 5 % wrong indices: over 1025 candidates."""
    return AS.build(1536, 17)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def device_pair(gpu, sc, P):
    """A pair that only has points (fillXU) and the scene pair over the device's OWN normalised observations."""
    torch, dev, ctx = gpu
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, P["n"])
    pair.fillXU(to_dev(torch, dev, P["sift"]))
    return pair, dict(P, X0=pair.get_XU(S.BUF_X0), ld=P["n"])


def first_candidates(A, B, index, m):
    """index with only the first m candidates left."""
    cand = np.flatnonzero(AS.candidates(A, B, index))
    assert len(cand) >= m
    out = np.full(len(index), -1, np.int32)
    out[cand[:m]] = index[cand[:m]]
    return out


def run_device(gpu, pa, pb, A, B, index, **kw):
    torch, dev, _ = gpu
    d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
    return pa.align_to(pb, d(np.asarray(index, np.int32)), points_a=d(A["points"]), valid_a=d(A["valid"]), points_b=d(B["points"]),
                       valid_b=d(B["valid"]), **kw)


def differences(got, want):
    """The figures of MEASURED for one pair of results (sim, inlier, err, counts, report, ...)."""
    f = lambda a: np.asarray(a, np.float64)
    gs, ws = f(got[0]), f(want[0])
    fin = np.isfinite(want[2]) & np.isfinite(got[2])
    return dict(s=abs(gs[0] - ws[0]) / ws[0], rot=RR.rotation_angle(gs[1:10].reshape(3, 3), ws[1:10].reshape(3, 3)),
                t=float(np.linalg.norm(gs[10:13] - ws[10:13]) / max(np.linalg.norm(ws[10:13]), 1e-30)),
                err=float((np.abs(f(got[2])[fin] - f(want[2])[fin]) / np.maximum(1.0, f(want[2])[fin])).max()) if fin.any() else 0.0,
                rms=abs(got[4]["final_rms_px"] - want[4]["final_rms_px"]),
                cost=abs(got[4]["final_cost"] - want[4]["final_cost"]) / max(want[4]["final_cost"], 1e-30))


@pytest.fixture(scope="module")
def pairs(gpu, scene):
    (pa, A), (pb, B) = device_pair(gpu, scene, scene["pairs"][0]), device_pair(gpu, scene, scene["pairs"][1])
    yield pa, pb, A, B
    pa.close(); pb.close()


@pytest.mark.parametrize("H", HYPOTHESES)
@pytest.mark.parametrize("m", CANDIDATES)
def test_override_path_against_the_host_build(gpu, HL, scene, pairs, m, H):
    """d_points_* given, so both pairs have points only.  The work buffer does not leave the library: the candidate order is held
    through every hypothesis' count (a sample is three places in that order), the error and flag of every record, and the report."""
    pa, pb, A, B = pairs
    index = first_candidates(A, B, scene["links"][0]["index"], m)
    worst = dict.fromkeys(MEASURED, 0.0)
    for iters in (0, 10):
        got = run_device(gpu, pa, pb, A, B, index, num_hypotheses=H, max_iterations=iters)
        want = AS.run_host(HL, S, A, B, index, K=scene["K"], num_hypotheses=H, max_iterations=iters)
        assert got[4]["num_candidates"] == m
        assert np.array_equal(got[3], want[3])                                 # every hypothesis' count
        assert got[4]["best_hypothesis"] == want[4]["best_hypothesis"] and np.array_equal(u8(got[0][13:]), u8(want[0][13:]))
        for k in ("status", "num_candidates", "ransac_inliers", "iterations", "accepted"):
            assert got[4][k] == want[4][k], (k, got[4], want[4])               # the same accept sequence
        assert np.array_equal(np.isinf(got[2]), np.isinf(want[2]))
        if iters == 0:                                                         # nothing summed reaches these
            for name, a, b in zip(("sim", "inlier", "err", "counts"), got, want):
                assert np.array_equal(u8(a), u8(b)), name
            assert np.array_equal(u8(got[0][:13]), u8(got[0][13:]))
            for k in ("num_inliers", "initial_rms_px") if got[4]["status"] == S.REFINE_DEGENERATE else ("num_inliers",):
                assert got[4][k] == want[4][k], (k, got[4], want[4])
        else:
            d = differences(got, want)
            worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"align m={m} H={H}: report {got[4]}, differences {worst}")
    if H >= 256 and m >= 63:
        assert got[4]["status"] != S.REFINE_DEGENERATE
    for k, bar in BARS.items():
        assert worst[k] <= bar, (k, worst[k], bar)
    if max(worst.values()) == 0.0:                                             # the same bytes, then
        for name, a, b in zip(("sim", "inlier", "err"), got, want):
            assert np.array_equal(u8(a), u8(b)), name


def test_degenerate_links_return_the_winner(gpu, HL, scene, pairs):
    pa, pb, A, B = pairs
    L = scene["links"][0]
    for name, index in (("2 candidates", first_candidates(A, B, L["index"], 2)), ("none", np.full(A["n"], -1, np.int32)),
                        ("out of range", np.where(np.arange(A["n"]) % 2 == 0, B["n"], -7).astype(np.int32))):
        got = run_device(gpu, pa, pb, A, B, index)
        want = AS.run_host(HL, S, A, B, index, K=scene["K"])
        assert got[4] == want[4] and got[4]["status"] == S.REFINE_DEGENERATE, (name, got[4], want[4])
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(u8(a), u8(b)), name
        assert not got[1].any() and got[0][0] == 1.0 and np.array_equal(got[0][:13], got[0][13:])


def assert_equals_host(got, want, what):
    """A device result against the host build's on the same inputs: counts, winner and every integer of the report equal, the
    rest within BARS."""
    assert np.array_equal(got[3], want[3]) and np.array_equal(u8(got[0][13:]), u8(want[0][13:])), what
    for k in ("status", "num_candidates", "ransac_inliers", "best_hypothesis", "iterations", "accepted"):
        assert got[4][k] == want[4][k], (what, k, got[4], want[4])
    d = differences(got, want)
    for k, bar in BARS.items():
        assert d[k] <= bar, (what, k, d[k], bar)


def filled(torch, dev, n, H):
    return (torch.full((26,), -3.0, dtype=torch.float32, device=dev), torch.full((n,), PATTERN, dtype=torch.uint8, device=dev),
            torch.full((n,), -7.0, dtype=torch.float32, device=dev), torch.full((H,), -9, dtype=torch.int32, device=dev),
            torch.full((C.sizeof(S.AlignReport),), PATTERN, dtype=torch.uint8, device=dev))


def untouched(outs):
    sim, inl, err, counts, rep = outs
    return bool((sim == -3.0).all() and (inl == PATTERN).all() and (err == -7.0).all() and (counts == -9).all() and (rep == PATTERN).all())


def read_buffers(pair, ctx):
    """Every SFM_BUF_* of the pair as bytes (None where the id answers (NULL, 0))."""
    L = S.lib()
    L.sfm_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    out = []
    for which in range(19):
        ptr, nbytes = pair.device_ptr(which)
        if not ptr:
            out.append(None)
            continue
        buf = np.empty(nbytes, np.uint8)
        assert L.sfm_copy_to_host(ctx._h, buf.ctypes.data_as(C.c_void_p), ptr, nbytes) == S.OK
        out.append(buf)
    return out


def getters(pair):
    """Every getter of a refined pair."""
    scored = pair.device_ptr(S.BUF_COUNTS)[1] // 4
    return (pair.get_E(), pair.get_inlier_mask(), *pair.get_refined_pose(), pair.get_refined_points(),
            *pair.get_reprojection_errors(), pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1),
            np.array(list(pair.get_refine_report().values()), np.float64), np.array([pair.get_key()], np.uint64),
            np.array(pair.get_best(), np.int64), pair.get_inlier_counts(1024)[:scored], pair.get_E_candidates(1024)[:scored])


def chain(gpu, sc, hyps=1024, good_masks=False):
    """Every pair of the scene on the device: fillXU -> estimateE -> one refine_pairs.  good_masks: the refinement runs over the
    records whose view-2 match is right instead of estimateE's inlier mask (which keeps about half of them at its 1e-6
    threshold and 1024 hypotheses), for the tests that need a given number of candidates."""
    torch, dev, ctx = gpu
    made = []
    for v, P in enumerate(sc["pairs"]):
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, P["n"])
        pair.fillXU(to_dev(torch, dev, P["sift"]))
        pair.estimateE(S.default_params(P["n"], num_hypotheses=hyps, seed=5 + v))
        made.append(pair)
    masks = [to_dev(torch, dev, P["good"].astype(np.uint8)) for P in sc["pairs"]] if good_masks else None
    reports = S.refine_pairs(made, max_iterations=20, masks=masks)
    return made, reports


def read_back(pair):
    """The pair's state as the dict the host build and the twin take."""
    _, used = pair.get_reprojection_errors()
    return dict(n=pair.num_points, ld=pair.num_points, points=pair.get_refined_points(), valid=used, X0=pair.get_XU(S.BUF_X0))


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, scene):
    torch, dev, ctx = gpu
    sc = AS.build(257, 7)
    made, _ = chain(gpu, sc, good_masks=True)
    pa, pb, pc = made
    d_index = to_dev(torch, dev, sc["links"][0]["index"])
    before = [(read_buffers(p, ctx), getters(p)) for p in (pa, pb)]
    first, second = pa.align_to(pb, d_index), pa.align_to(pb, d_index)
    assert first[4]["status"] != S.REFINE_DEGENERATE and first[4] == second[4]
    for a, b in zip(first[:4], second[:4]):
        assert np.array_equal(u8(a), u8(b))
    for p, (bufs, answers) in zip((pa, pb), before):
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
        for a, b in zip(answers, getters(p)):
            assert np.array_equal(u8(a), u8(b))
    n, params = pa.num_points, S.align_params()
    outs = filled(torch, dev, n, params.num_hypotheses)
    d_pts, d_val = to_dev(torch, dev, sc["pairs"][0]["points"]), to_dev(torch, dev, sc["pairs"][0]["valid"])
    big = torch.full((n + 64,), -7.0, dtype=torch.float32, device=dev)
    bigi = torch.full((4 * n,), -1, dtype=torch.int32, device=dev)              # the index in the middle of a buffer of its own
    bigi[n:2 * n] = d_index
    mid_index = bigi.data_ptr() + 4 * n
    bigr = torch.full((4 * params.num_hypotheses + 64,), PATTERN, dtype=torch.uint8, device=dev)

    def refused(code, a=pa, b=pb, index=d_index, p=params, o=outs):
        with pytest.raises(S.SfmError) as e:
            a.align_to_enqueue(b, index, p, *o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    # aliasing: an output on an input, on another output (equal addresses and ranges)
    assert "out.d_inlier overlaps d_index" in refused(S.E_INVALID, o=(outs[0], d_index) + outs[2:])
    assert "out.d_err overlaps d_index" in refused(S.E_INVALID, index=mid_index, o=outs[:2] + (mid_index + 4 * (n - 1),) + outs[3:])
    assert "out.d_sim overlaps params.d_points_a" in refused(S.E_INVALID, p=S.align_params(points_a=d_pts), o=(d_pts.data_ptr() + 16,) + outs[1:])
    assert "overlaps params.d_valid_b" in refused(S.E_INVALID, p=S.align_params(points_b=d_pts, valid_b=d_val), o=outs[:1] + (d_val,) + outs[2:])
    assert "out.d_sim overlaps out.d_err" in refused(S.E_INVALID, o=(big.data_ptr() + 4 * n - 4, outs[1], big) + outs[3:])
    assert "out.d_counts overlaps out.d_report" in refused(S.E_INVALID, o=outs[:3] + (bigr, bigr.data_ptr() + 4 * params.num_hypotheses - 4))
    # the same pair twice, another context, a missing stage on either side
    assert "same pair" in refused(S.E_INVALID, b=pa)
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, sc["K"], sc["Kinv"], 2, n)
    foreign.fillXU(to_dev(torch, dev, sc["pairs"][1]["sift"]))
    assert "different contexts" in refused(S.E_INVALID, b=foreign)
    bare = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    refused(S.E_STATE, b=bare)                                                 # no points
    bare.fillXU(to_dev(torch, dev, sc["pairs"][1]["sift"]))
    refused(S.E_STATE, b=bare)                                                 # points, no refinement
    refused(S.E_STATE, a=bare, b=pb)
    refused(S.E_STATE, b=bare, p=S.align_params(points_a=d_pts))               # the override of a does not serve b
    assert untouched(outs) and bool((big == -7.0).all()) and bool((bigr == PATTERN).all())
    assert np.array_equal(bigi.cpu().numpy(), np.concatenate([np.full(n, -1), sc["links"][0]["index"], np.full(2 * n, -1)]))
    assert np.array_equal(d_index.cpu().numpy(), sc["links"][0]["index"]) and np.array_equal(u8(d_pts.cpu().numpy()), u8(sc["pairs"][0]["points"]))
    # ... and with the override on its own side the bare pair serves as a: points are all it needs
    bare.align_to_enqueue(pb, d_index, S.align_params(points_a=d_pts, valid_a=d_val), *outs)
    ctx.synchronize()
    assert not untouched(outs)
    for p in (pa, pb, pc, bare, foreign):
        p.close()
    other.close()


def test_full_chain_on_the_device(gpu, HL):
    """4 views, n = 1024: fillXU -> estimateE -> refine_pairs -> align_pairs over 2 links, against the truth at the level the
    twin reaches on the read-back state (device error <= 1.25 x the twin's, 6f's rule) and against the twin at the host-build
    bars."""
    torch, dev, ctx = gpu
    sc = AS.build(1024, 61)
    made, reports = chain(gpu, sc)
    assert all(r["status"] != S.REFINE_DEGENERATE for r in reports)
    print("full chain: refined pairs use " + ", ".join(f"{r['num_used']} records at {r['final_rms_px']:.3f} px" for r in reports))
    idx = [to_dev(torch, dev, L["index"]) for L in sc["links"]]
    res = S.align_pairs(made[:2], made[1:], idx)
    state = [read_back(p) for p in made]
    for v, (L, got) in enumerate(zip(sc["links"], res)):
        sim, inl, err, counts, rep = got
        A, B = state[v], state[v + 1]
        host = AS.run_host(HL, S, A, B, L["index"], K=sc["K"])
        assert_equals_host(got, host, f"link {v}")
        cand = AS.candidates(A, B, L["index"])
        h0 = AS.run_host(HL, S, A, B, L["index"], K=sc["K"], max_iterations=0)
        win = (float(sim[13]), sim[14:23].reshape(3, 3).astype(np.float64), sim[23:26].astype(np.float64))
        tw = AR.run(A, B, L["index"], sc["K"], sc["K"], start=win, inliers=h0[1][cand].astype(bool))
        ts, tR, tt = tw["sim"]
        ds, dr = abs(sim[0] - ts) / ts, RR.rotation_angle(sim[1:10].reshape(3, 3).astype(np.float64), tR)
        dt = np.linalg.norm(sim[10:13] - tt) / np.linalg.norm(tt)
        dev_err, twin_err = AS.sim_errors(sim[:13], L), AS.sim_errors(AR.pack(tw["sim"]), L)
        print(f"full chain link {v}: {rep}\n  s {sim[0]:.6f} (truth {L['s']:.6f}); errors s / rot / t: device {dev_err}, twin {twin_err}; "
              f"device against twin s {ds:.3g} rot {dr:.3g} t {dt:.3g}")
        assert rep["status"] != S.REFINE_DEGENERATE
        assert dr <= ROT_BAR and dt <= T_BAR and ds <= S_BAR
        assert abs(rep["final_rms_px"] - tw["lm"]["final_rms"]) <= 1e-4
        for name, a, b in zip(("s", "rot", "t"), dev_err, twin_err):
            assert a <= 1.25 * b + 1e-7, (v, name, a, b)
    for p in made:
        p.close()


def test_dino_frames_0_1_2(gpu, HL):
    """Real frames: pair A = (0, 1), pair B = (1, 2).  No bar on s or |t| (6c's gauge findings): a status that is not DEGENERATE
    and agreement with the twin on the read-back state."""
    torch, dev, ctx = gpu
    (d0, n0), (d1, n1), (d2, n2) = (VS.dino_extract(gpu, k) for k in (0, 1, 2))
    ctx.match(d0, n0, d1, n1)
    ctx.match(d1, n1, d2, n2)
    pa, pb = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0), S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n1)
    pa.fillXU(d0); pb.fillXU(d1)
    pa.estimateE(S.default_params(n0)); pb.estimateE(S.default_params(n1))
    S.refine_pairs([pa, pb], max_iterations=20)
    d_index = torch.empty(n0, dtype=torch.int32, device=dev)
    S.align_index_from_matches(ctx, d0, n0, d_index)
    sim, inl, err, counts, rep = pa.align_to(pb, d_index)
    index = d_index.cpu().numpy()
    rec = np.frombuffer(d0[:n0].cpu().numpy().tobytes(), S.SIFT_DTYPE)
    gate = (rec["match"] >= 0) & (rec["score"] > 0.85) & (rec["ambiguity"] < 0.95)
    assert np.array_equal(index, np.where(gate, rec["match"], -1))
    A, B = read_back(pa), read_back(pb)
    host = AS.run_host(HL, S, A, B, index, K=DINO_K)
    assert_equals_host((sim, inl, err, counts, rep), host, "dino")
    RA = pa.get_refined_pose()[0][:3, :3].astype(np.float64)
    angle = RR.rotation_angle(sim[1:10].reshape(3, 3).astype(np.float64), RA)
    print(f"dino 0-1-2: {rep}\n  s {sim[0]:.5f}, |t| {np.linalg.norm(sim[10:13]):.5f}, angle between the link's R and pair A's refined R {angle:.3e} rad")
    assert rep["status"] != S.REFINE_DEGENERATE and rep["num_inliers"] == int(inl.sum()) and np.isfinite(sim).all()
    cand = AS.candidates(A, B, index)
    h0 = AS.run_host(HL, S, A, B, index, K=DINO_K, max_iterations=0)
    win = (float(sim[13]), sim[14:23].reshape(3, 3).astype(np.float64), sim[23:26].astype(np.float64))
    tw = AR.run(A, B, index, DINO_K, DINO_K, start=win, inliers=h0[1][cand].astype(bool))
    ts, tR, tt = tw["sim"]
    ds, dr = abs(sim[0] - ts) / ts, RR.rotation_angle(sim[1:10].reshape(3, 3).astype(np.float64), tR)
    # t = mean X_B - s R mean X_A is the difference of two vectors of the size of the inliers' centroid in B's frame, which fp32
    # holds to 6e-8 of THAT size; in the dino's gauges |t| is a hundredth of it (no bar on |t|, 6c), so the agreement in t is
    # taken relative to the larger of the two.  (On the synthetic scenes |t| is the larger or close to it: their bar stays |t|'s.)
    Pb = B["points"].astype(np.float64)
    kb = index[inl.astype(bool)]
    centroid = np.linalg.norm((Pb[:3, kb] / Pb[3, kb]).mean(1))
    dt = np.linalg.norm(sim[10:13] - tt) / max(np.linalg.norm(tt), centroid)
    print(f"  device against twin: s {ds:.3g} rot {dr:.3g} t {dt:.3g} (|t| {np.linalg.norm(tt):.4f}, |centroid of B's inliers| {centroid:.4f}); "
          f"rms {rep['final_rms_px']:.6f} / {tw['lm']['final_rms']:.6f}")
    assert dr <= ROT_BAR and dt <= T_BAR and ds <= S_BAR and abs(rep["final_rms_px"] - tw["lm"]["final_rms"]) <= 1e-4
    pa.close(); pb.close()
