"""GPU: sfm_adjust_view / sfm_adjust_views (csrc/adjust.hip) through the C ABI -- every output against the host build of the same
arithmetic (tests/hostcheck/libadjustcheck.so), which differs from the kernel only in the order of the fp64 sums; degenerate
inputs; determinism and the aliasing checks; the full chain on the device with nothing in the pair changed; the batched call
against the single call; the dino frames 0, 1, 2."""
import ctypes as C
import os

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import DINO_K, DINO_KINV, make_pair, to_dev
import adjust_reference as AR
import adjust_scene as AS
import refine_reference as RR
import register_scene as RS
import view_points_reference as VR
import view_points_scene as VS
from test_adjust_host import ROT_BAR, T_BAR, RMS_BAR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0xA5
SIZES = [63, 64, 65, 257, 1024]
# Kernel against host build: the two differ only in the order of the fp64 sums of the system and of the costs (wave butterflies
# and wave order against record order).  MEASURED: the largest difference over the ten cases below on the MI355X -- rotation angle
# of cameras 2 / 3 (rad), largest |t| difference, largest |X - X'| / |X'| over the used points, largest |err - err'| / max(1, err'),
# rms (px), cost (relative).  Every one is 0: an fp64 sum of about a thousand fp32 terms has 29 spare bits, so it comes out the
# same in either order, and the accept sequences are identical on every case (20 iterations: 18 / 20 / 6 / 20 / 20 iterations,
# 7 / 9 / 6 / 8 / 9 accepted at n = 63 / 64 / 65 / 257 / 1024).  The bars are 4 x the measured maximum: equality.
MEASURED = dict(rot=0.0, t=0.0, points=0.0, err=0.0, rms=0.0, cost=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def HL():
    return VS.host_lib()


@pytest.fixture(scope="module")
def AL():
    return AS.host_lib()


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def device_start(gpu, HL, n, seed):
    """A pair that only has points (fillXU) and the perturbed start over the pair's OWN normalised observations."""
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    pair, _ = make_pair(S, gpu, sc)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
    s = AS.perturb(VS.finish(sc, rec, truth, pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1)), seed)
    s["vp_points"], s["vp_flags"], _, _ = VS.run_host(HL, S, s, threshold_px=16.0)
    s["used2"] = s["valid"].copy()
    return pair, s


def run_device(gpu, pair, s, points=None, flags=None, used2=None, **kw):
    torch, dev, _ = gpu
    d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
    return pair.adjust_view(d(s["rec"]), d(s["vp_points"] if points is None else points), d(s["vp_flags"] if flags is None else flags),
                            used2=d(s["used2"] if used2 is None else used2), poses=d(s["poses"]), **kw)


def differences(got, want):
    """The figures of MEASURED for one pair of results (poses, points, views, err, report)."""
    (gp, gx, gv, ge, gr), (wp, wx, wv, we, wr) = got, want
    u = wv != 0
    f = lambda a: np.asarray(a, np.float64)
    d = dict(rot=max(RR.rotation_angle(gp[:9].reshape(3, 3), wp[:9].reshape(3, 3)), RR.rotation_angle(gp[12:21].reshape(3, 3), wp[12:21].reshape(3, 3))),
             t=float(max(np.abs(f(gp[9:12]) - f(wp[9:12])).max(), np.abs(f(gp[21:]) - f(wp[21:])).max())),
             points=0.0, err=0.0, rms=abs(gr["final_rms_px"] - wr["final_rms_px"]),
             cost=abs(gr["final_cost"] - wr["final_cost"]) / max(wr["final_cost"], 1e-30))
    if u.any():
        d["points"] = float((np.linalg.norm(f(gx[:3, u]) - f(wx[:3, u]), axis=0) / np.linalg.norm(f(wx[:3, u]), axis=0)).max())
        d["err"] = float((np.abs(f(ge[u]) - f(we[u])) / np.maximum(1.0, f(we[u]))).max())
    return d


@pytest.mark.parametrize("max_iterations", [0, 20])
@pytest.mark.parametrize("n", SIZES)
def test_override_path_against_the_host_build(gpu, HL, AL, n, max_iterations):
    """d_used2 and d_poses given, so the pair has points only: one wavefront short, full and over, a second block with one live
    lane, more than one round of the solve block.  The classes are sfm_triangulate_view's at the perturbed start with a 16 px
    threshold (device_start): at 4 px view 3 would see fewer than six records of the small scenes."""
    pair, s = device_start(gpu, HL, n, 61 if n == 1024 else 7 + n)
    got = run_device(gpu, pair, s, max_iterations=max_iterations)
    want = AS.run_host(AL, S, s, max_iterations=max_iterations)
    d = differences(got, want)
    print(f"adjust n={n} iterations={max_iterations}: report {got[4]}, host {want[4]}, differences {d}")
    assert np.array_equal(got[2], want[2])                                     # d_views: equal on every record
    for k in ("status", "iterations", "accepted", "num_points", "num_view2", "num_view3"):
        assert got[4][k] == want[4][k], (k, got[4], want[4])                  # the same accept sequence
    assert got[4]["num_view2"] >= 16 and got[4]["num_view3"] >= 6
    unused = want[2] == 0
    assert np.array_equal(u8(got[1][:, unused]), u8(s["vp_points"][:, unused])) and np.isposinf(got[3][unused]).all()
    if max_iterations == 0:                                                    # nothing summed reaches these
        for name, a, b in zip(("poses", "points", "views", "err"), got, want):
            assert np.array_equal(u8(a), u8(b)), name
        assert np.array_equal(u8(got[0]), u8(s["poses"]))
    for k, bar in BARS.items():
        assert d[k] <= bar, (k, d[k], bar)
    pair.close()


def test_degenerate_inputs_return_the_start(gpu, HL, AL):
    pair, s = device_start(gpu, HL, 257, 7)
    _, _, views, _, full = AS.run_host(AL, S, s)
    cases = []
    for keep in (15, 16):                                                      # records in view 2: the boundary
        used2 = np.zeros(s["n"], np.uint8)
        used2[np.flatnonzero((views & 2) != 0)[:keep]] = 1
        cases.append((f"view2={keep}", dict(used2=used2), keep == 15))
    for keep in (5, 6):                                                        # records in view 3
        flags = s["vp_flags"].copy()
        flags[np.flatnonzero((views & 4) != 0)[keep:]] = S.VP_KEPT
        cases.append((f"view3={keep}", dict(flags=flags), keep == 5))
    cases.append(("none", dict(used2=np.zeros(s["n"], np.uint8), flags=np.zeros(s["n"], np.uint8)), True))
    pts = s["vp_points"].copy()
    a, b = np.flatnonzero(views != 0)[:2]
    pts[3, a] = 0.0; pts[1, b] = np.nan
    cases.append(("w0 and nan", dict(points=pts), False))
    for name, kw, degenerate in cases:
        got = run_device(gpu, pair, s, **kw)
        want = AS.run_host(AL, S, s, **kw)
        assert np.array_equal(got[2], want[2]), name
        assert (got[4]["status"] == S.REFINE_DEGENERATE) == degenerate, (name, got[4])
        for k in ("status", "iterations", "accepted", "num_points", "num_view2", "num_view3"):
            assert got[4][k] == want[4][k], (name, k, got[4], want[4])
        if degenerate:                                                         # the start poses, the input columns, d_views filled
            assert np.array_equal(u8(got[0]), u8(s["poses"])), name
            assert np.array_equal(u8(got[1]), u8(kw.get("points", s["vp_points"]))), name
            assert np.array_equal(u8(got[3]), u8(want[3])), name
            assert got[4]["iterations"] == 0 and got[4]["final_rms_px"] == got[4]["initial_rms_px"]
        else:
            d = differences(got, want)
            for k, bar in BARS.items():
                assert d[k] <= bar, (name, k, d[k], bar)
    assert got[2][a] == 0 and got[2][b] == 0 and np.array_equal(u8(got[1][:, [a, b]]), u8(pts[:, [a, b]])) and np.isfinite(got[0]).all()
    pair.close()


def filled(torch, dev, n):
    return (torch.full((24,), -3.0, dtype=torch.float32, device=dev), torch.full((4, n), float("nan"), dtype=torch.float32, device=dev),
            torch.full((n,), PATTERN, dtype=torch.uint8, device=dev), torch.full((n,), -7.0, dtype=torch.float32, device=dev),
            torch.full((C.sizeof(S.AdjustReport),), PATTERN, dtype=torch.uint8, device=dev))


def untouched(torch, outs):
    poses, pts, views, err, rep = outs
    return bool((poses == -3.0).all() and torch.isnan(pts).all() and (views == PATTERN).all() and (err == -7.0).all() and (rep == PATTERN).all())


def test_second_call_repeats_and_aliasing_is_refused_with_nothing_written(gpu, HL):
    torch, dev, ctx = gpu
    pair, s = device_start(gpu, HL, 257, 7)
    first, second = run_device(gpu, pair, s), run_device(gpu, pair, s)
    for a, b in zip(first[:4], second[:4]):
        assert np.array_equal(u8(a), u8(b))
    assert first[4] == second[4]
    d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
    d_rec, d_pts, d_flags, d_used2, d_poses = d(s["rec"]), d(s["vp_points"]), d(s["vp_flags"]), d(s["used2"]), d(s["poses"])
    params = S.adjust_params(used2=d_used2, poses=d_poses)
    outs = filled(torch, dev, s["n"])
    big = torch.full((4 * s["n"] + 64,), float("nan"), dtype=torch.float32, device=dev)

    def refused(args, p=params, rec=d_rec):
        with pytest.raises(S.SfmError) as e:
            pair.adjust_view_enqueue(rec, d_pts, d_flags, p, *args)
        ctx.synchronize()
        assert e.value.code == S.E_INVALID, str(e.value)
        return str(e.value)
    assert "16-byte aligned" in refused(outs, rec=d_rec.data_ptr() + 8)
    assert "out.d_points overlaps in.d_points" in refused((outs[0], d_pts) + outs[2:])
    assert "overlaps in.d_flags" in refused(outs[:2] + (d_flags,) + outs[3:])
    assert "overlaps params.d_used2" in refused(outs[:2] + (d_used2,) + outs[3:])
    assert "out.d_poses overlaps params.d_poses" in refused((d_poses,) + outs[1:])
    assert "overlaps in.d_sift" in refused(outs[:3] + (d_rec.data_ptr() + 64, outs[4]))
    # ranges, not only equal addresses: the error array inside the output points, the poses inside them
    assert "out.d_points overlaps out.d_err" in refused((outs[0], big, outs[2], big.data_ptr() + 4 * s["n"], outs[4]))
    assert "out.d_poses overlaps out.d_points" in refused((big.data_ptr() + 16 * s["n"] - 4, big) + outs[2:])
    assert untouched(torch, outs) and bool(torch.isnan(big).all())
    assert np.array_equal(u8(d_pts.cpu().numpy()), u8(s["vp_points"])) and np.array_equal(d_flags.cpu().numpy(), s["vp_flags"])
    pair.close()


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
    scored = pair.device_ptr(S.BUF_COUNTS)[1] // 4
    return (pair.get_E(), pair.get_inlier_mask(), pair.get_points(), pair.get_result(), *pair.get_refined_pose(), pair.get_refined_points(),
            *pair.get_reprojection_errors(), *pair.get_view_pose(), *pair.get_view_errors(), pair.get_view_counts(), pair.get_pose_candidates(),
            pair.get_pose_inverses(), np.array([pair.get_pose_index()]), pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1),
            np.array(list(pair.get_refine_report().values()), np.float64), np.array(list(pair.get_register_report().values()), np.float64),
            np.array([pair.get_key()], np.uint64), np.array(pair.get_best(), np.int64), pair.get_inlier_counts(1024)[:scored], pair.get_E_candidates(1024)[:scored])


def chain(gpu, n, seed):
    """fillXU -> estimateE -> pose_chain(CORRECT) -> refine -> register on the device; the pair and the records of view 3."""
    torch, dev, _ = gpu
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=seed))
    pair.pose_chain(S.POSE_CORRECT)
    pair.refine(max_iterations=20)
    rec, truth = RS.third_view(sc, seed=seed, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
    d_rec = to_dev(torch, dev, rec)
    pair.register_view(d_rec)
    return sc, pair, d_sift, rec, d_rec


def start_poses(pair):
    """float32[24]: the refined pose and the registered view's refined pose in the d_poses layout."""
    P2, P3 = pair.get_refined_pose()[0], pair.get_view_pose()[0]
    return np.concatenate([P2[:3, :3].ravel(), P2[:3, 3], P3[:3, :3].ravel(), P3[:3, 3]]).astype(np.float32)


def test_full_chain_reads_the_pair_and_changes_nothing(gpu):
    torch, dev, ctx = gpu
    sc, pair, d_sift, rec, d_rec = chain(gpu, 1024, 61)
    vp = pair.triangulate_view(d_rec)
    d_pts, d_flags = to_dev(torch, dev, vp[0]), to_dev(torch, dev, vp[1])
    buffers, answers = read_buffers(pair, ctx), getters(pair)
    poses, points, views, err, rep = pair.adjust_view(d_rec, d_pts, d_flags)
    for which, (a, b) in enumerate(zip(buffers, read_buffers(pair, ctx))):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    for a, b in zip(answers, getters(pair)):
        assert np.array_equal(u8(a), u8(b))
    # the twin over the read-back state: fp32 chain against fp64, the host build's bars (tests/test_adjust_host.py)
    _, used = pair.get_reprojection_errors()
    p0 = start_poses(pair)
    tp, tx, tv, terr, tr = AR.run(sc["K"], sc["Kinv"], rec, pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1), vp[0], vp[1], used, p0)
    print(f"full chain: report {rep}; twin rms {tr['initial_rms_px']:.6f} -> {tr['final_rms_px']:.6f}, {tr['iterations']} iterations")
    assert np.array_equal(views, tv)
    assert (rep["num_points"], rep["num_view2"], rep["num_view3"]) == (tr["num_points"], tr["num_view2"], tr["num_view3"])
    assert RR.rotation_angle(poses[:9].reshape(3, 3), tp[:9].reshape(3, 3)) <= ROT_BAR and RR.rotation_angle(poses[12:21].reshape(3, 3), tp[12:21].reshape(3, 3)) <= ROT_BAR
    assert np.abs(poses[9:12] - tp[9:12]).max() <= T_BAR and np.abs(poses[21:] - tp[21:]).max() <= T_BAR
    assert abs(rep["final_rms_px"] - tr["final_rms_px"]) <= RMS_BAR and abs(rep["initial_rms_px"] - tr["initial_rms_px"]) <= RMS_BAR
    assert rep["final_rms_px"] <= rep["initial_rms_px"]                        # the rms over all three views does not rise
    assert abs(np.linalg.norm(poses[9:12]) - 1.0) < 1e-6
    # one more triangulation with the adjusted poses: at least as many accepted records as the first, minus what the twin itself
    # loses between the two states plus its records within 10 % of the threshold or of the smallest parallax at the adjusted state
    second = pair.triangulate_view(d_rec, poses=to_dev(torch, dev, poses))
    accepted = lambda f: int(((f == S.VP_NEW) | (f == S.VP_REFINED)).sum())
    cam = lambda p, o: (p[o:o + 9].reshape(3, 3).astype(np.float64), p[o + 9:o + 12].astype(np.float64))
    pts_r = pair.get_refined_points()
    X0, X1 = pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1)
    ref1 = VR.view_points(sc["K"], sc["Kinv"], rec, X0, X1, pts_r, used, cam(p0, 0), cam(p0, 12))
    ref2 = VR.view_points(sc["K"], sc["Kinv"], rec, X0, X1, pts_r, used, cam(tp, 0), cam(tp, 12))
    with np.errstate(invalid="ignore"):
        band = ref2["seen"] & ((np.abs(ref2["err"] - 4.0) <= 0.4) | (np.abs(ref2["parallax"] - 1.0) <= 0.1))
    slack = max(0, accepted(ref1["flags"]) - accepted(ref2["flags"])) + int(band.sum())
    print(f"full chain: accepted {accepted(vp[1])} -> {accepted(second[1])}, twin {accepted(ref1['flags'])} -> {accepted(ref2['flags'])}, slack {slack}")
    assert accepted(second[1]) >= accepted(vp[1]) - slack
    pair.close()


@pytest.mark.parametrize("order", ["listed", "permuted"])
def test_batched_call_equals_the_single_call(gpu, order):
    torch, dev, ctx = gpu
    sizes = [64, 257, 1024, 300, 8]                                            # the 8-point pair is degenerate
    if order == "permuted":
        sizes = [300, 8, 1024, 64, 257]
    made = [chain(gpu, n, 20 + n) for n in sizes]
    pairs, recs = [m[1] for m in made], [m[4] for m in made]
    vps = [p.triangulate_view(r) for p, r in zip(pairs, recs)]
    ins = [(r, to_dev(torch, dev, v[0]), to_dev(torch, dev, v[1])) for r, v in zip(recs, vps)]
    single = [p.adjust_view(*i) for p, i in zip(pairs, ins)]
    assert single[sizes.index(8)][4]["status"] == S.REFINE_DEGENERATE and single[sizes.index(1024)][4]["status"] != S.REFINE_DEGENERATE
    outs = [filled(torch, dev, p.num_points) for p in pairs]
    S.adjust_views_enqueue(pairs, ins, S.adjust_params(), outs)
    ctx.synchronize()
    for k, (want, got) in enumerate(zip(single, outs)):
        for name, a, b in zip(("poses", "points", "views", "err"), want, got):
            assert np.array_equal(u8(a), u8(b.cpu().numpy())), (order, sizes[k], name)
        r = S.AdjustReport.from_buffer_copy(got[4].cpu().numpy().tobytes())
        assert {f: getattr(r, f) for f, _ in S.AdjustReport._fields_} == want[4], (order, sizes[k])
    again = S.adjust_views(pairs, ins)
    assert [tuple(u8(a).tobytes() for a in r[:4]) + (r[4],) for r in again] == [tuple(u8(a).tobytes() for a in r[:4]) + (r[4],) for r in single]
    # a pair without its registration and a pair listed twice: the error names the pair, nothing is written
    sc = synth.two_view_scene(64, seed=5, noise_px=0.5, outlier_frac=0.3)
    bare, _ = make_pair(S, gpu, sc)
    bare.estimateE(S.default_params(64, num_hypotheses=256, seed=5))
    bare.refine(max_iterations=5)
    # ... and an output of one pair on an output, or on an input, of another pair
    # (the smaller pair 0 is given the buffer of the 1024-point pair 2, so that the buffer is large enough for its user)
    share_out = lambda o: [o[0][:3] + (o[2][3],) + o[0][4:]] + o[1:]
    share_in = lambda o: [(o[0][0], ins[2][1]) + o[0][2:]] + o[1:]
    for plist, ilist, code, text, tweak in ((pairs[:2] + [bare] + pairs[2:], ins[:2] + [ins[0]] + ins[2:], S.E_STATE, "no registration", None),
                                            (pairs[:2] + [pairs[0]] + pairs[2:], ins[:2] + [ins[0]] + ins[2:], S.E_INVALID, "listed twice", None),
                                            (pairs, ins, S.E_INVALID, "overlaps a buffer of pairs[0]", share_out),
                                            (pairs, ins, S.E_INVALID, "overlaps a buffer of pairs[0]", share_in)):
        outs = [filled(torch, dev, p.num_points) for p in plist]
        if tweak:
            outs = tweak(outs)
        with pytest.raises(S.SfmError) as e:
            S.adjust_views_enqueue(plist, ilist, S.adjust_params(), outs)
        assert e.value.code == code and "pairs[2]" in str(e.value) and text in str(e.value), str(e.value)
        ctx.synchronize()
        assert all(untouched(torch, o) for k, o in enumerate(outs) if not (tweak is share_in and k == 0))      # (that one holds an input)
    for p in pairs + [bare]:
        p.close()


def test_dino_frames_0_1_2(gpu):
    torch, dev, ctx = gpu
    (d0, n0), (d1, n1), (d2, n2) = (VS.dino_extract(gpu, k) for k in (0, 1, 2))
    ctx.match(d0, n0, d1, n1)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    pair.refine(max_iterations=20)
    ctx.match(d0, n0, d2, n2)
    pair.register_view(d0)
    points, flags, err, counts = pair.triangulate_view(d0)
    p0 = start_poses(pair)
    poses, apts, views, aerr, rep = pair.adjust_view(d0, to_dev(torch, dev, points), to_dev(torch, dev, flags))
    _, used = pair.get_reprojection_errors()
    centre = lambda p: float(np.linalg.norm(p[12:21].reshape(3, 3).astype(np.float64).T @ p[21:24].astype(np.float64)))
    print(f"dino 0-1-2: classes {counts[:5].tolist()}, report {rep}, |C3| {centre(p0):.4f} -> {centre(poses):.4f}, "
          f"camera 3 rotated by {RR.rotation_angle(poses[12:21].reshape(3, 3), p0[12:21].reshape(3, 3)):.3e} rad, "
          f"camera 2 by {RR.rotation_angle(poses[:9].reshape(3, 3), p0[:9].reshape(3, 3)):.3e} rad")
    # the report against the classes: view 3 sees the new and refined records that are used, view 2 no more than the refinement used
    assert rep["num_view3"] == int(((views & 4) != 0).sum()) <= counts[S.VP_NEW] + counts[S.VP_REFINED]
    assert rep["num_view2"] == int(((views & 2) != 0).sum()) <= int(used.sum())
    assert rep["num_points"] == int((views != 0).sum()) and np.array_equal((views & 4) != 0, (views != 0) & np.isin(flags, (S.VP_NEW, S.VP_REFINED)))
    assert rep["final_rms_px"] <= rep["initial_rms_px"] and np.isfinite(poses).all()
    pair.close()
