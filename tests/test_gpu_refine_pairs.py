"""GPU: sfm_refine_pairs (csrc/refine.hip: the three refinement kernels over an array of jobs, grid = pairs) against
sfm_refine_two_view on the same handles.  The single call is pinned by the numpy twin in tests/test_gpu_refine.py; here every
comparison is bit for bit: the report, the refined pose and E, the refined points, the reprojection errors and the used flags."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import make_pair, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTERS = ("get_refine_report", "get_refined_pose", "get_refined_points", "get_reprojection_errors")


def estimated(gpu, n, seed, hyps=1024, scene=None, estimate=True):
    sc = scene if scene is not None else synth.two_view_scene(n, seed=seed, noise_px=0.5, outlier_frac=0.3)
    pair, d_sift = make_pair(S, gpu, sc)
    if estimate:
        pair.estimateE(S.default_params(n, num_hypotheses=hyps, seed=seed))
    return sc, pair, d_sift


def reading(pair):
    """Everything the refinement left in the pair."""
    return (pair.get_refine_report(), pair.get_refined_pose(), pair.get_refined_points(), pair.get_reprojection_errors())


def same_report(a, b):
    assert a.keys() == b.keys()
    return all(same_bits([a[k]], [b[k]]) if isinstance(a[k], float) else a[k] == b[k] for k in a)


def same_reading(a, b):
    (ra, (Pa, Ea), Xa, (ea, ua)), (rb, (Pb, Eb), Xb, (eb, ub)) = a, b
    return (same_report(ra, rb) and same_bits(Pa, Pb) and same_bits(Ea, Eb) and same_bits(Xa, Xb) and same_bits(ea, eb)
            and np.array_equal(ua, ub))


def assert_not_refined(pair):
    for name in GETTERS:
        with pytest.raises(S.SfmError) as e:
            getattr(pair, name)()
        assert e.value.code == S.E_STATE, name


def first_inliers_mask(gpu, pair, count):
    """Ones at the first `count` inliers of the pair's mask (tests/test_gpu_refine.py::test_contracts)."""
    torch, dev, _ = gpu
    mask = np.zeros(pair.num_points, np.uint8)
    mask[np.flatnonzero(pair.get_inlier_mask())[:count]] = 1
    return torch.from_numpy(mask).to(dev)


def test_parity_with_the_single_call_on_the_same_handles(gpu):
    # a start block of exactly 64 points, ragged start / finish blocks, one and several rounds of the 512-wide compaction scan,
    # very unequal block counts inside one launch
    sizes = (64, 100, 257, 512, 513, 1100, 2155, 4096)
    pairs = [estimated(gpu, n, 100 + k)[1] for k, n in enumerate(sizes)]
    for p in pairs:
        assert_not_refined(p)
    reports = S.refine_pairs(pairs, max_iterations=20)
    batched = [reading(p) for p in pairs]
    assert len(reports) == len(pairs) and all(same_report(r, b[0]) for r, b in zip(reports, batched))
    for n, p, got in zip(sizes, pairs, batched):
        rep = p.refine(max_iterations=20)
        single = reading(p)
        assert same_report(rep, single[0])
        assert same_reading(got, single), (n, got[0], single[0])
        assert got[3][1].sum() == got[0]["num_used"]


def test_the_batched_call_overwrites(gpu):
    pairs = [estimated(gpu, n, 200 + k)[1] for k, n in enumerate((700, 1024, 300))]
    start = []
    for p in pairs:
        p.refine(max_iterations=0)
        start.append(reading(p))
    S.refine_pairs(pairs, max_iterations=20)
    batched = [reading(p) for p in pairs]
    for p, got in zip(pairs, batched):
        p.refine(max_iterations=20)
        assert same_reading(got, reading(p))
    assert any(not same_reading(a, b) for a, b in zip(start, batched))
    assert any(b[0]["iterations"] > 0 for b in batched)


def test_masks_and_the_degenerate_case(gpu):
    pairs = [estimated(gpu, n, 300 + k)[1] for k, n in enumerate((600, 1024, 900))]
    m10 = first_inliers_mask(gpu, pairs[1], 10)
    masks = [None, m10, None]
    reports = S.refine_pairs(pairs, max_iterations=20, masks=masks)
    batched = [reading(p) for p in pairs]
    assert reports[1]["status"] == S.REFINE_DEGENERATE and reports[1]["iterations"] == 0 and reports[1]["num_used"] <= 10
    assert reports[0]["num_used"] > 10 and reports[2]["num_used"] > 10
    for p, m, got in zip(pairs, masks, batched):
        p.refine(max_iterations=20, mask=m)
        assert same_reading(got, reading(p))
    # a pointer array with every entry null is the call without masks
    S.refine_pairs(pairs, max_iterations=20, masks=[None, None, None])
    with_nulls = [reading(p) for p in pairs]
    S.refine_pairs(pairs, max_iterations=20)
    assert all(same_reading(a, reading(p)) for a, p in zip(with_nulls, pairs))
    assert not same_reading(with_nulls[1], batched[1])


def test_more_pairs_than_compute_units(gpu):
    """260 solve blocks on 256 compute units: 260 pairs of 128 points over 4 scenes (the estimates differ by their seeds)."""
    count, n = 260, 128
    t0 = time.perf_counter()
    scenes = [synth.two_view_scene(n, seed=400 + s, noise_px=0.5, outlier_frac=0.3) for s in range(4)]
    pairs = [estimated(gpu, n, 1000 + k, hyps=256, scene=scenes[k % 4])[1] for k in range(count)]
    t1 = time.perf_counter()
    reports = S.refine_pairs(pairs, max_iterations=20)
    full = {k: reading(pairs[k]) for k in range(0, count, 13)}
    t2 = time.perf_counter()
    for k, p in enumerate(pairs):
        assert same_report(reports[k], p.refine(max_iterations=20)), k
        if k in full:
            assert same_reading(full[k], reading(p)), k
    t3 = time.perf_counter()
    print(f"{count} pairs: create + estimateE {t1 - t0:.2f} s, batched + read {t2 - t1:.2f} s, per-pair loop {t3 - t2:.2f} s")


def test_order_independence_reproducibility_and_no_side_effects(gpu):
    sizes = (300, 1100, 300, 64, 700, 1100)                    # equal sizes too: the job order is a stable sort by size
    pairs = [estimated(gpu, n, 500 + k)[1] for k, n in enumerate(sizes)]
    pairs[1].pose_chain(S.POSE_CORRECT)
    keep = pairs[1]

    def others():
        return (keep.get_E(), keep.get_inlier_mask(), keep.get_best(), keep.get_points(), keep.get_pose_index(), keep.get_result())

    before = others()
    S.refine_pairs(pairs, max_iterations=20)
    first = [reading(p) for p in pairs]
    S.refine_pairs(pairs[::-1], max_iterations=20)
    assert all(same_reading(a, reading(p)) for a, p in zip(first, pairs))
    S.refine_pairs(pairs, max_iterations=20)
    assert all(same_reading(a, reading(p)) for a, p in zip(first, pairs))
    for a, b in zip(before, others()):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        else:
            assert a == b
    for p, got in zip(pairs, first):
        p.refine(max_iterations=20)
        assert same_reading(got, reading(p))


def test_pipelined_estimates_pending(gpu):
    n = 1024
    sc = synth.two_view_scene(n, seed=41)
    pa, _ = make_pair(S, gpu, sc)
    for s in (1, 2):
        pa.estimateE_pipelined(S.default_params(n, num_hypotheses=1024, seed=s))
    left, right = estimated(gpu, 500, 600)[1], estimated(gpu, 1500, 601)[1]
    S.refine_pairs([left, pa, right], max_iterations=20)
    pb, _ = make_pair(S, gpu, sc)
    pb.estimateE(S.default_params(n, num_hypotheses=1024, seed=2))
    pb.refine(max_iterations=20)
    assert same_reading(reading(pa), reading(pb))
    assert np.array_equal(pa.get_E().view(np.uint32), pb.get_E().view(np.uint32))


def test_contracts_on_the_device(gpu):
    torch, dev, ctx = gpu
    a, b, c = (estimated(gpu, n, 700 + k)[1] for k, n in enumerate((400, 600, 500)))

    def refused(pairs, params, code, masks=None):
        with pytest.raises(S.SfmError) as e:
            S.refine_pairs_enqueue(pairs, params, masks)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    refused([a, b, a], S.refine_params(), S.E_INVALID)
    ctx2 = S.Context(0, torch.cuda.current_stream().cuda_stream)
    sc = synth.two_view_scene(300, seed=710)
    foreign = S.ImagePair(ctx2, sc["K"], sc["Kinv"], 2, 300)
    foreign.fillXU(torch.from_numpy(sc["sift"].view(np.uint8).reshape(300, 576)).to(dev))
    foreign.estimateE(S.default_params(300, num_hypotheses=256))
    refused([a, foreign, b], S.refine_params(), S.E_INVALID)
    refused([a, b, c], S.refine_params(reserved=[0, 0, 1, 0]), S.E_INVALID)
    refused([a, b, c], S.refine_params(max_iterations=201), S.E_INVALID)
    refused([a, b, c], S.refine_params(mask=first_inliers_mask(gpu, a, 10)), S.E_INVALID)
    for p in (a, b, c, foreign):
        assert_not_refined(p)
    foreign.close()
    ctx2.close()

    _, middle, d_middle = estimated(gpu, 450, 720, estimate=False)             # fillXU, no estimateE
    text = refused([a, middle, b], S.refine_params(), S.E_STATE)
    assert "pairs[1]" in text and "estimateE" in text
    for p in (a, middle, b):
        assert_not_refined(p)

    S.refine_pairs([a, b, c], max_iterations=5)
    kept = [reading(p) for p in (a, c)]
    sc_b = synth.two_view_scene(600, seed=701, noise_px=0.5, outlier_frac=0.3)
    b.fillXU(torch.from_numpy(sc_b["sift"].view(np.uint8).reshape(600, 576)).to(dev))
    assert_not_refined(b)
    for which in (S.BUF_REFINED_POSE, S.BUF_REFINED_POINTS, S.BUF_REPROJ):
        assert b.device_ptr(which) == (None, 0)
        assert a.device_ptr(which)[0] and c.device_ptr(which)[0]
    assert all(same_reading(k, reading(p)) for k, p in zip(kept, (a, c)))


def test_facade_demo_prints_what_sfm_main_prints_per_pair(tmp_path):
    """host/refine_pairs_demo (SfM::refine_pairs of host/sfm.h) on three pairs of feature files against host/sfm_main on the
    images they came from, one pair per run: the same used count, rms values and iteration count."""
    host = os.path.join(ROOT, "cuda-sfm_amd", "host")
    demo, app, sift_demo = (os.path.join(host, x) for x in ("refine_pairs_demo", "sfm_main", "sift_demo"))
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
    order = [(0, 1), (1, 2), (2, 3)]
    line = re.compile(r"^refine: \d+ points, rms [0-9.]+ -> [0-9.]+ px, \d+ iterations$", flags=re.M)
    want = []
    for i, j in order:
        r = subprocess.run([app, frames[i], frames[j], str(tmp_path / "cloud.ply"), "", "0", "0", "1.0", "1.5", "2360", "20"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        want += line.findall(r.stdout)
    args = [f for i, j in order for f in (feats[i], feats[j])]
    r = subprocess.run([demo, "20", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = line.findall(r.stdout)
    assert len(want) == 3 and got == want, (got, want)
