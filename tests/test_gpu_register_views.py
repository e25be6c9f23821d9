"""GPU: sfm_register_views (csrc/register.hip: the four registration kernels over an array of jobs, grid = pairs) against
sfm_register_view on the same handles.  The single call is pinned by the host build of its arithmetic and the numpy twin in
tests/test_gpu_register.py; here every comparison is byte for byte: the report, the refined and the RANSAC pose, the errors and
the inlier flags, the per-hypothesis counts.  The batched scoring launch uses ONE share count for all jobs, usually another than
the single call's: equal counts show that they do not depend on it."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import DINO_K, DINO_KINV, make_pair, same_bits, to_dev
import register_scene as RS
from test_gpu_register import HL, dino_extract, host_candidates, host_ransac, obs_on_device  # noqa: F401  (HL: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTERS = ("get_register_report", "get_view_pose", "get_view_errors", "get_view_counts")
VIEW_BUFS = (S.BUF_VIEW_POSE, S.BUF_VIEW_COUNTS, S.BUF_VIEW_REPROJ)
STATUSES = (S.REFINE_CONVERGED, S.REFINE_MAX_ITER, S.REFINE_DEGENERATE)
SEED_A, SEED_B = 0x5EED5F3D, 0x0BADC0DE


def view_case(gpu, n, m, seed, noise_px=0.5, outlier_frac=0.3):
    """A pair over a noise-free two-view scene of n points (fillXU only), view 1's records re-matched against a synthetic third
    view with exactly m candidates (the score of every record beyond m fails the gate), the scene's exact points on the device."""
    torch, dev, _ = gpu
    sc = synth.two_view_scene(n, seed=seed, noise_px=0.0, outlier_frac=0.0)
    pair, _ = make_pair(S, gpu, sc)
    rec, _ = RS.third_view(sc, seed=seed, noise_px=noise_px, outlier_frac=outlier_frac)
    rec["score"][m:] = 0.5
    pts = RS.homogeneous(sc["points3d"])
    return {"sc": sc, "pair": pair, "rec": rec, "pts": pts, "d_rec": to_dev(torch, dev, rec), "d_pts": torch.from_numpy(pts).to(dev)}


def reading(pair):
    """Everything the registration left in the pair."""
    return (pair.get_register_report(), *pair.get_view_pose(), *pair.get_view_errors(), pair.get_view_counts())


def same_report(a, b):
    assert a.keys() == b.keys()
    return all(same_bits([a[k]], [b[k]]) if isinstance(a[k], float) else a[k] == b[k] for k in a)


def same_reading(a, b):
    (ra, Pa, Qa, ea, ia, ca), (rb, Pb, Qb, eb, ib, cb) = a, b
    return (same_report(ra, rb) and same_bits(Pa, Pb) and same_bits(Qa, Qb) and same_bits(ea, eb) and np.array_equal(ia, ib)
            and ca.shape == cb.shape and np.array_equal(ca, cb))


def assert_no_view(pair):
    for name in GETTERS:
        with pytest.raises(S.SfmError) as e:
            getattr(pair, name)()
        assert e.value.code == S.E_STATE, name
    for which in VIEW_BUFS:
        assert pair.device_ptr(which) == (None, 0)


def batched(cases, **kw):
    return S.register_views([c["pair"] for c in cases], [c["d_rec"] for c in cases], points=[c["d_pts"] for c in cases], **kw)


def single(case, **kw):
    return case["pair"].register_view(case["d_rec"], points=case["d_pts"], **kw)


def test_parity_with_the_single_call_on_the_same_handles_and_overwrite(gpu, HL):
    H = 4096
    # (n, m): a handful of candidates, fewer than one wavefront, a ragged LDS stage, exact points, a degenerate view (3
    # candidates), several LDS stages per share
    shapes = [(64, 5), (64, 37), (1024, 1000), (2048, 2048), (1024, 3), (4096, 4096)]
    cases = [view_case(gpu, n, m, 100 + k, **(dict(noise_px=0.0, outlier_frac=0.0) if (n, m) == (2048, 2048) else {}))
             for k, (n, m) in enumerate(shapes)]
    for c in cases:
        assert_no_view(c["pair"])
    A = []
    for c in cases:
        rep = single(c, num_hypotheses=H, seed=SEED_A)
        A.append(reading(c["pair"]))
        assert same_report(rep, A[-1][0])
    assert A[4][0]["status"] == S.REFINE_DEGENERATE and all(a[0]["status"] != S.REFINE_DEGENERATE for k, a in enumerate(A) if k not in (0, 4))
    # another seed: the batched call writes every pair's results
    reports = batched(cases, num_hypotheses=H, seed=SEED_B)
    B = [reading(c["pair"]) for c in cases]
    assert all(same_report(r, b[0]) for r, b in zip(reports, B))
    for k, (a, b) in enumerate(zip(A, B)):
        assert k == 4 or not same_reading(a, b), shapes[k]
    # the same seed: byte for byte what the single calls left
    reports = batched(cases, num_hypotheses=H, seed=SEED_A)
    for k, c in enumerate(cases):
        got = reading(c["pair"])
        assert same_report(reports[k], got[0]) and same_reading(got, A[k]), (shapes[k], got[0], A[k][0])
        assert got[0]["num_candidates"] == shapes[k][1]
    # independent anchor: the host build of the same arithmetic
    for k in (1, 2):
        c = cases[k]
        idx, Xc = host_candidates(c["rec"], c["pts"], None, c["sc"]["Kinv"])
        Oc = obs_on_device(gpu, c["sc"], c["rec"])[idx]
        key, counts, _ = host_ransac(HL, c["sc"]["K"], Oc, Xc, H, seed=SEED_A)
        got = reading(c["pair"])
        assert np.array_equal(got[5], counts) and got[0]["best_hypothesis"] == S.unpack_key(key)[1], shapes[k]


@pytest.mark.parametrize("H", [1, 65536])
def test_hypothesis_counts(gpu, H):
    cases = [view_case(gpu, 1024, 1000, 200 + k) for k in range(3)]
    batched(cases, num_hypotheses=H)
    got = [reading(c["pair"]) for c in cases]
    for c, g in zip(cases, got):
        assert g[5].shape == (H,)
        single(c, num_hypotheses=H)
        assert same_reading(g, reading(c["pair"]))


def test_per_hypothesis_buffers_grow_across_batched_calls(gpu):
    cases = [view_case(gpu, 1024, 1000, 210 + k) for k in range(3)]
    for H in (256, 4096):
        reports = batched(cases, num_hypotheses=H)
        for c, r in zip(cases, reports):
            counts = c["pair"].get_view_counts()
            assert counts.shape == (H,) and c["pair"].device_ptr(S.BUF_VIEW_COUNTS)[1] == 4 * H
            assert counts.max() == r["ransac_inliers"] and r["best_hypothesis"] == int(np.argmax(counts))
    got = [reading(c["pair"]) for c in cases]
    for c, g in zip(cases, got):
        single(c, num_hypotheses=4096)
        assert same_reading(g, reading(c["pair"]))


def test_more_jobs_than_compute_units(gpu):
    """300 gate / LM blocks on 256 compute units; 300 pairs over six scenes, each with a third view of its own."""
    torch, dev, _ = gpu
    count, H = 300, 256
    sizes = (64, 97, 128, 200, 255, 256)
    scenes = [synth.two_view_scene(n, seed=300 + s, noise_px=0.0, outlier_frac=0.0) for s, n in enumerate(sizes)]
    d_pts = [torch.from_numpy(RS.homogeneous(sc["points3d"])).to(dev) for sc in scenes]
    cases = []
    for k in range(count):
        sc = scenes[k % len(scenes)]
        rec, _ = RS.third_view(sc, seed=1000 + k, noise_px=0.5, outlier_frac=0.3)
        cases.append({"pair": make_pair(S, gpu, sc)[0], "d_rec": to_dev(torch, dev, rec), "d_pts": d_pts[k % len(scenes)]})
    reports = batched(cases, num_hypotheses=H)
    assert len(reports) == count
    for k, r in enumerate(reports):
        assert r["status"] in STATUSES and r["num_candidates"] == sizes[k % len(sizes)] and r["best_hypothesis"] < H, (k, r)
    assert sum(r["status"] != S.REFINE_DEGENERATE for r in reports) > count // 2
    for k in range(0, count, 37):
        got = reading(cases[k]["pair"])
        assert same_report(got[0], reports[k])
        single(cases[k], num_hypotheses=H)
        assert same_reading(got, reading(cases[k]["pair"])), k


def test_order_independence_reproducibility_and_no_side_effects(gpu):
    torch, dev, _ = gpu
    sizes = (300, 1100, 300, 64, 700, 1100)                    # equal sizes too: the job order is a stable sort by size
    pairs, recs = [], []
    for k, n in enumerate(sizes):
        sc = synth.two_view_scene(n, seed=500 + k, noise_px=0.5, outlier_frac=0.3)
        pair, _ = make_pair(S, gpu, sc)
        pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=500 + k))
        pair.pose_chain(S.POSE_CORRECT)
        pair.refine(max_iterations=10)
        rec, _ = RS.third_view(sc, seed=500 + k, noise_px=0.5, outlier_frac=0.3)
        pairs.append(pair)
        recs.append(to_dev(torch, dev, rec))

    def others(p):
        return (p.get_E(), p.get_inlier_mask(), p.get_points(), p.get_result(), np.array([p.get_pose_index()]), p.get_refined_pose()[0],
                p.get_refined_points(), *p.get_reprojection_errors())

    before = [others(p) for p in pairs]
    S.register_views(pairs, recs)
    first = [reading(p) for p in pairs]
    assert sum(r[0]["status"] != S.REFINE_DEGENERATE for r in first) >= 4
    S.register_views(pairs[::-1], recs[::-1])
    assert all(same_reading(a, reading(p)) for a, p in zip(first, pairs))
    S.register_views(pairs, recs)
    assert all(same_reading(a, reading(p)) for a, p in zip(first, pairs))
    for b, p in zip(before, pairs):
        for x, y in zip(b, others(p)):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    for p, d, got in zip(pairs, recs, first):
        p.register_view(d)
        assert same_reading(got, reading(p))


def test_mixed_point_sources_and_a_pending_pipelined_estimate(gpu):
    torch, dev, _ = gpu
    n = 1024
    # on its refined points
    sc_a = synth.two_view_scene(n, seed=600, noise_px=0.5, outlier_frac=0.3)
    pa, _ = make_pair(S, gpu, sc_a)
    pa.estimateE(S.default_params(n, num_hypotheses=1024, seed=600))
    pa.refine(max_iterations=10)
    rec_a, _ = RS.third_view(sc_a, seed=600, noise_px=0.5, outlier_frac=0.3)
    d_a = to_dev(torch, dev, rec_a)
    # on caller points, with a pipelined estimateE burst still pending
    b = view_case(gpu, n, n, 601)
    for s in (1, 2):
        b["pair"].estimateE_pipelined(S.default_params(n, num_hypotheses=1024, seed=s))
    # on caller points with every second point cleared
    c = view_case(gpu, n, n, 602)
    valid = np.ones(n, np.uint8); valid[1::2] = 0
    d_valid = torch.from_numpy(valid).to(dev)
    reports = S.register_views([pa, b["pair"], c["pair"]], [d_a, b["d_rec"], c["d_rec"]], points=[None, b["d_pts"], c["d_pts"]],
                               valid=[None, None, d_valid])
    got = [reading(p) for p in (pa, b["pair"], c["pair"])]
    _, used = pa.get_reprojection_errors()
    assert 10 < reports[0]["num_candidates"] <= int(used.sum()) and reports[1]["num_candidates"] == n and reports[2]["num_candidates"] == n // 2
    assert not got[2][4][1::2].any() and np.isinf(got[2][3][1::2]).all()
    twin, _ = make_pair(S, gpu, b["sc"])
    twin.estimateE(S.default_params(n, num_hypotheses=1024, seed=2))
    assert np.array_equal(b["pair"].get_E().view(np.uint32), twin.get_E().view(np.uint32))
    pa.register_view(d_a)
    assert same_reading(got[0], reading(pa))
    single(b)
    assert same_reading(got[1], reading(b["pair"]))
    c["pair"].register_view(c["d_rec"], points=c["d_pts"], valid=d_valid)
    assert same_reading(got[2], reading(c["pair"]))


def test_contracts_on_the_device(gpu):
    torch, dev, ctx = gpu
    a, b, c = (view_case(gpu, n, n, 700 + k) for k, n in enumerate((400, 600, 500)))
    pairs, recs, pts = [x["pair"] for x in (a, b, c)], [x["d_rec"] for x in (a, b, c)], [x["d_pts"] for x in (a, b, c)]

    def refused(pairs, recs, params, code, points=None, valid=None):
        with pytest.raises(S.SfmError) as e:
            S.register_views_enqueue(pairs, recs, params, points, valid)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    refused([pairs[0], pairs[1], pairs[0]], recs, S.register_params(), S.E_INVALID, pts)
    ctx2 = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(ctx2, b["sc"]["K"], b["sc"]["Kinv"], 2, 600)
    foreign.fillXU(to_dev(torch, dev, b["sc"]["sift"]))
    refused([pairs[0], foreign, pairs[2]], recs, S.register_params(), S.E_INVALID, pts)
    refused(pairs, recs, S.register_params(points=pts[0]), S.E_INVALID, pts)
    refused(pairs, recs, S.register_params(num_hypotheses=0), S.E_INVALID, pts)
    refused(pairs, recs, S.register_params(), S.E_INVALID, [pts[0], None, pts[2]], [None, pts[1], None])     # valid without points
    for p in pairs + [foreign]:
        assert_no_view(p)
    foreign.close()
    ctx2.close()

    # the third pair has no refined points and no points entry; the first has a registration already
    single(a)
    kept = reading(pairs[0])
    text = refused(pairs, recs, S.register_params(), S.E_STATE, [pts[0], pts[1], None])
    assert "pairs[2]" in text
    assert same_reading(kept, reading(pairs[0]))
    for which in VIEW_BUFS:
        assert pairs[0].device_ptr(which)[0]
    assert_no_view(pairs[1])
    assert_no_view(pairs[2])

    # after a call that went through, fillXU on one pair makes only that pair's view stale
    batched([a, b, c], num_hypotheses=512)
    kept = [reading(p) for p in (pairs[0], pairs[2])]
    pairs[1].fillXU(to_dev(torch, dev, b["sc"]["sift"]))
    assert_no_view(pairs[1])
    for p, k in zip((pairs[0], pairs[2]), kept):
        assert same_reading(k, reading(p))
        for which in VIEW_BUFS:
            assert p.device_ptr(which)[0]


def test_dino_triples(gpu):
    torch, dev, ctx = gpu
    feats = [dino_extract(gpu, k) for k in range(4)]
    pairs = []
    for i in (0, 1):
        (d1, n1), (d2, n2) = feats[i], feats[i + 1]
        ctx.match(d1, n1, d2, n2)
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n1)
        pair.fillXU(d1)
        pair.estimateE(S.default_params(n1))
        pairs.append(pair)
    S.refine_pairs(pairs, max_iterations=20)
    for i in (0, 1):
        ctx.match(feats[i][0], feats[i][1], feats[i + 2][0], feats[i + 2][1])
    recs = [feats[0][0], feats[1][0]]
    reports = S.register_views(pairs, recs)
    got = [reading(p) for p in pairs]
    print(f"dino triples (0, 1, 2), (1, 2, 3): {reports}")
    for p, d, g, r in zip(pairs, recs, got, reports):
        assert r["num_inliers"] > 50 and same_report(r, g[0])
        p.register_view(d)
        assert same_reading(g, reading(p))


def test_facade_demo_prints_what_sfm_main_prints_per_triple(tmp_path):
    """host/register_views_demo (SfM::refine_pairs, then SfM::register_views of host/sfm.h) on the feature files of two dino
    triples against host/sfm_main on the images they came from, one triple per run: the same view3 line."""
    host = os.path.join(ROOT, "cuda-sfm_amd", "host")
    demo, app, sift_demo = (os.path.join(host, x) for x in ("register_views_demo", "sfm_main", "sift_demo"))
    for exe in (demo, app, sift_demo):
        assert os.path.exists(exe), f"{os.path.basename(exe)} not built (make)"
    frames = [os.path.join(ROOT, "tests", "golden", "dino", f"dino_grey_00{k}.pgm") for k in range(4)]
    feats = []
    for k in (0, 2):                                            # sift_demo extracts two frames per run
        out = [str(tmp_path / f"f{k + d}.sift") for d in (0, 1)]
        r = subprocess.run([sift_demo, frames[k], frames[k + 1], *out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        for path in out:                                        # sift_demo's files carry a count in front of the records
            raw = open(path, "rb").read()
            n = int(np.frombuffer(raw[:4], np.int32)[0])
            rec = path.replace(".sift", ".bin")
            open(rec, "wb").write(raw[4:4 + 576 * n])
            feats.append(rec)
    triples = [(0, 1, 2), (1, 2, 3)]
    line = re.compile(r"^view3: \d+/\d+ inliers, rms [0-9.]+ -> [0-9.]+ px, \|C3\| [0-9.]+$", flags=re.M)
    want = []
    for i, j, k in triples:
        r = subprocess.run([app, frames[i], frames[j], str(tmp_path / "cloud.ply"), "", "0", "0", "1.0", "1.5", "2360", "20", frames[k]],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        want += line.findall(r.stdout)
    r = subprocess.run([demo, "20", *[feats[f] for t in triples for f in t]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = line.findall(r.stdout)
    assert len(want) == 2 and got == want, (got, want)
