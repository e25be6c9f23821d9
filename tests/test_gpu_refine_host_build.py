"""GPU: sfm_refine_two_view / sfm_refine_pairs (csrc/refine.hip) against the host build of the whole call (rc_run of
tests/hostcheck/librefinecheck.so) at the block edges of the three kernels -- the cases of tests/refine_scene.py, designed over
the pair's own buffers (get_XU, get_E, the inlier mask), so that the host build reads exactly what the kernels read.  Equality is
the bar: the two run the same header functions, the host build takes the fp64 sums in the block's order, both are compiled without
contraction.  Every report integer, the used flags, the pose, E, all 4 x n points, the errors and the report's floats are compared
bit for bit (a NaN equals a NaN whatever its payload: the points of a record without pixels can be NaN; its error is +inf).
tests/test_refine_run_host.py holds the host build to the fp64 twin and checks on the CPU that the cases are what they are meant
to be."""
import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import make_pair, same_bits, to_dev
import refine_scene as RS

pytestmark = pytest.mark.gpu
INTS = ("status", "iterations", "accepted", "num_used", "pose_index")
FLOATS = ("initial_rms_px", "final_rms_px", "final_cost", "lambda")


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


def device_case(gpu, HL, case):
    """The case on the device up to estimateE, its mask designed over the pair's own buffers: dict(pair, sc, X0, X1, E, mask, d_mask)."""
    torch, dev, ctx = gpu
    sc = RS.scene_of(case)
    if case.special == "z":
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, case.n)
        X0, X1 = RS.points_cpu(sc)
        pair.set_points(to_dev(torch, dev, X0), to_dev(torch, dev, X1))
    else:
        pair, _ = make_pair(S, gpu, sc)
    pair.estimateE(S.default_params(case.n, num_hypotheses=RS.HYPS, seed=case.seed))
    X0, X1, E, inl = pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1), pair.get_E(), pair.get_inlier_mask()
    mask, caller = RS.design(HL, S, case, sc, X0, X1, E, inl)
    return dict(case=case, pair=pair, sc=sc, X0=X0, X1=X1, E=E, mask=mask, d_mask=to_dev(torch, dev, mask) if caller else None)


def reading(pair):
    P, E = pair.get_refined_pose()
    err, used = pair.get_reprojection_errors()
    return dict(report=pair.get_refine_report(), pose=P, E=E, points=pair.get_refined_points(), err=err, used=used)


def differing(got, want):
    """The names of the fields in which a device reading differs from a host run."""
    out = [k for k in INTS if got["report"][k] != want["report"][k]]
    out += [k for k in FLOATS if not same_bits([got["report"][k]], [want["report"][k]])]
    out += [k for k in ("pose", "E", "points", "err") if not same_bits(got[k], want[k])]
    if not np.array_equal(got["used"], want["used"]):
        out.append("used")
    return out


def line(case, got, diff):
    r = got["report"]
    return (f"refine {case.name}: n={case.n} m={r['num_used']} pose_index={r['pose_index']} status={r['status']} "
            f"iterations={r['iterations']} accepted={r['accepted']} rms {r['initial_rms_px']:.4f} -> {r['final_rms_px']:.4f}: "
            + ("equal" if not diff else "DIFFERS in " + ", ".join(diff)))


def check_design(case, got):
    """On the device's own buffers the case is still what the table says."""
    r = got["report"]
    assert got["used"].sum() == r["num_used"]
    if case.name in RS.EXACT:
        assert r["num_used"] == RS.EXACT[case.name]
    if case.name in RS.DEGENERATE:
        assert r["status"] == S.REFINE_DEGENERATE and r["iterations"] == 0 and np.isfinite(got["pose"]).all() and np.isfinite(got["E"]).all()
    else:
        assert r["status"] in (S.REFINE_CONVERGED, S.REFINE_MAX_ITER) and r["num_used"] >= 16
    if case.name in ("last511", "last512"):
        assert np.flatnonzero(got["used"])[-1] == int(case.name[4:])
    if case.special == "unused":
        assert not got["used"][[*RS.UNUSED_NAN, RS.UNUSED_BEHIND]].any()


@pytest.mark.parametrize("case", RS.CASES, ids=[c.name for c in RS.CASES])
def test_single_call_equals_the_host_build(gpu, HL, case):
    d = device_case(gpu, HL, case)
    pair = d["pair"]
    rep = pair.refine(mask=d["d_mask"], **case.kw)
    got = reading(pair)
    assert rep == got["report"]
    want = RS.run_host(HL, S, d["X0"], d["X1"], d["E"], d["sc"]["K"], d["mask"], **case.kw)
    diff = differing(got, want)
    print(line(case, got, diff))
    if diff:
        print("  device", got["report"], "\n  host  ", want["report"], "trace", want["trace"].tolist())
    assert not diff, (case.name, diff, got["report"], want["report"])
    check_design(case, got)
    pair.close()


def test_batched_call_equals_the_host_build(gpu, HL):
    """Every case's pair in one sfm_refine_pairs call per parameter set (the call takes one set for all its pairs): all cases with
    the default parameters in one call with their masks, the few with other parameters in a call each group."""
    defaults = dict(max_iterations=20, huber_px=1.0)                       # a case that restates them joins the large call
    groups = {}
    for case in RS.CASES:
        groups.setdefault(tuple(sorted((k, v) for k, v in case.kw.items() if defaults[k] != v)), []).append(case)
    assert len(groups[()]) >= 25
    for kw, cases in groups.items():
        ds = [device_case(gpu, HL, c) for c in cases]
        reports = S.refine_pairs([d["pair"] for d in ds], masks=[d["d_mask"] for d in ds], **dict(kw))
        for d, rep in zip(ds, reports):
            got = reading(d["pair"])
            assert rep == got["report"]
            want = RS.run_host(HL, S, d["X0"], d["X1"], d["E"], d["sc"]["K"], d["mask"], **dict(kw))
            diff = differing(got, want)
            print("batched " + line(d["case"], got, diff))
            assert not diff, (d["case"].name, diff, got["report"], want["report"])
            check_design(d["case"], got)
        for d in ds:
            d["pair"].close()


def test_generic_z_pair_equals_the_host_build_of_the_same_rays_at_unit_z(gpu, HL):
    """The committed case (tests/golden/refine_generic_z_case.npz: points with z != 1 through sfm_set_points) on the device against
    the host build over the SAME RAYS rescaled to z = 1, with the fixture's E and mask: bit for bit.  The call reads the points as
    x / z, y / z only -- the start once triangulated on x, y as given -- so the bar is equality (tests/test_refine_run_host.py)."""
    torch, dev, ctx = gpu
    g = np.load(RS.GENERIC_Z_FIXTURE)
    n = g["X0"].shape[1]
    pair = S.ImagePair(ctx, g["K"], g["Kinv"], 2, n)
    pair.set_points(to_dev(torch, dev, g["X0"]), to_dev(torch, dev, g["X1"]))
    pair.estimateE(S.default_params(n, num_hypotheses=int(g["hyps"]), seed=int(g["seed"])))
    assert same_bits(pair.get_E(), g["E"]) and same_bits(pair.get_XU(S.BUF_X0), g["X0"])
    for kw in (dict(), dict(max_iterations=0)):
        pair.refine(mask=to_dev(torch, dev, g["mask"]), **kw)
        got = reading(pair)
        want = RS.run_host(HL, S, RS.unit_z(g["X0"]), RS.unit_z(g["X1"]), g["E"], g["K"], g["mask"], **kw)
        diff = differing(got, want)
        print(f"generic z against unit z {kw}: {got['report']}: " + ("equal" if not diff else "DIFFERS in " + ", ".join(diff)))
        assert not diff, (diff, got["report"], want["report"])
        assert got["report"]["num_used"] == g["mask"].sum()
    pair.close()


@pytest.mark.parametrize("name", ["round513", "round1025", "unused", "skew-120"])
def test_second_call_repeats_the_bytes_and_nothing_else_changes(gpu, HL, name):
    """An odd and an even number of committed steps, a mask with unused records, estimateE's own mask."""
    case = next(c for c in RS.CASES if c.name == name)
    d = device_case(gpu, HL, case)
    pair = d["pair"]
    pair.pose_chain(S.POSE_CORRECT)
    others = lambda: (pair.get_E(), pair.get_inlier_mask(), pair.get_best(), pair.get_points(), pair.get_pose_index(), pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1))
    before = others()
    pair.refine(mask=d["d_mask"], **case.kw)
    first = reading(pair)
    pair.refine(mask=d["d_mask"], **case.kw)
    second = reading(pair)
    assert not differing(second, first)
    for a, b in zip(before, others()):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        else:
            assert a == b
    if d["d_mask"] is not None:
        assert np.array_equal(d["d_mask"].cpu().numpy(), d["mask"])
    pair.close()
