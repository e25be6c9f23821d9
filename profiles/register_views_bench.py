"""Cost of sfm_register_views against a loop of sfm_register_view over the same pairs: HIP events around the enqueued calls, one
process.  For every list of P pairs: a warm-up of both forms, then three repetitions of [P single calls back to back | one
batched call], alternating; the loop of the same run is the baseline.  Lists: P synthetic pairs of n points registered on the
scene's exact points (eight scenes x eight third views with 0.5 px noise and 30 % outliers, shared by the pairs in turn), with
the default parameters and with max_iterations = 0; with --dino the ring of 36 triples (i, i + 1, i + 2) of the committed dino
frames (features by sfm_extract_views, per triple sfm_match + fillXU + estimateE, ONE sfm_refine_pairs, then view i re-matched
against view i + 2) on the refined points.  `splits` is the share count of the batched scoring launch, recomputed here by the
launcher's rule (csrc/register.hip: register_splits) from the device's CU count.
    python profiles/register_views_bench.py [--dino]
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/register_views_bench.py --pairs 630 --reps 1 --batched-only"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
from cuda_sfm_amd import synth  # noqa: E402
import register_scene as RS  # noqa: E402


def splits_of(num_cus, hyps, jobs, nmax):
    hblocks = (hyps + 255) // 256
    blocks = hblocks * jobs
    return max(1, min((4 * num_cus + blocks - 1) // blocks, max(1, nmax // 128)))


def synthetic_jobs(ctx, dev, count, n):
    """(pair, records, points) per job: eight scenes, eight third views each."""
    scenes = []
    for s in range(8):
        sc = synth.two_view_scene(n, seed=7 + s, noise_px=0.0, outlier_frac=0.0)
        d_sift = torch.from_numpy(sc["sift"].view(np.uint8).reshape(n, 576)).to(dev)
        d_pts = torch.from_numpy(RS.homogeneous(sc["points3d"])).to(dev)
        views = []
        for v in range(8):
            rec, _ = RS.third_view(sc, seed=100 * s + v, noise_px=0.5, outlier_frac=0.3)
            views.append(torch.from_numpy(rec.view(np.uint8).reshape(n, 576)).to(dev))
        scenes.append((sc, d_sift, d_pts, views))
    jobs = []
    for k in range(count):
        sc, d_sift, d_pts, views = scenes[k % 8]
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
        pair.fillXU(d_sift)
        jobs.append((pair, views[(k // 8) % 8], d_pts))
    return jobs


def dino_jobs(ctx, dev):
    from helpers import read_pnm_grey, dino_frame, DINO_K, DINO_KINV, DINO_SIFT
    views = [read_pnm_grey(dino_frame(k)) for k in range(36)]
    max_pts = 8192
    _, counts = S.process_views(ctx, views, DINO_K, DINO_KINV, pairs=[(0, 1)], max_pts=max_pts, sift=DINO_SIFT, device=dev)
    block = ctx._views_block[:36 * (max_pts * 576 + 64)].view(36, max_pts * 576 + 64)
    pairs = []
    for i in range(36):
        j = (i + 1) % 36
        ctx.match(block[i], counts[i], block[j], counts[j])           # writes view i's match fields; fillXU reads them next on the stream
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, counts[i])
        pair.fillXU(block[i])
        pair.estimateE()
        pairs.append(pair)
    S.refine_pairs(pairs, max_iterations=20)
    for i in range(36):
        k = (i + 2) % 36
        ctx.match(block[i], counts[i], block[k], counts[k])           # view i re-matched against the triple's third view
    return [(pairs[i], block[i], None) for i in range(36)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, jobs, kw, reps, num_cus, batched_only=False):
    pairs, recs, pts = [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs]
    params = S.register_params(**kw)
    singles = [S.register_params(points=p, **kw) for p in pts]

    def loop():
        for pair, d, sp in zip(pairs, recs, singles):
            pair.register_enqueue(d, sp)

    def batched():
        S.register_views_enqueue(pairs, recs, params, pts)

    if not batched_only:
        loop()
    torch.cuda.synchronize()
    single = [p.get_register_report() for p in pairs] if not batched_only else None
    batched()
    torch.cuda.synchronize()
    reports = [p.get_register_report() for p in pairs]
    same = "n/a" if batched_only else str(reports == single)
    t_loop, t_batch = [], []
    for _ in range(reps):
        if not batched_only:
            t_loop.append(timed(loop))
        t_batch.append(timed(batched))
    cand = [r["num_candidates"] for r in reports]
    iters = [r["iterations"] for r in reports]
    nmax = max(p.num_points for p in pairs)
    line = (f"{name}: P={len(pairs)} n={min(p.num_points for p in pairs)}..{nmax} candidates={min(cand)}..{max(cand)} "
            f"iterations={min(iters)}..{max(iters)} splits batched={splits_of(num_cus, params.num_hypotheses, len(pairs), nmax)} "
            f"single={splits_of(num_cus, params.num_hypotheses, 1, min(p.num_points for p in pairs))}.."
            f"{splits_of(num_cus, params.num_hypotheses, 1, nmax)} reports equal: {same} | ")
    if not batched_only:
        line += "loop ms " + " ".join(f"{t:.3f}" for t in t_loop) + " | "
    line += "batched ms " + " ".join(f"{t:.3f}" for t in t_batch)
    if not batched_only:
        lo, ba = float(np.median(t_loop)), float(np.median(t_batch))
        line += f" | medians {lo:.3f} / {ba:.3f} ms = {lo / ba:.1f}x, {1e3 * lo / len(pairs):.1f} -> {1e3 * ba / len(pairs):.1f} us per pair"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--batched-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {num_cus} compute units", flush=True)
    modes = (("defaults", {}), ("max_iterations=0", dict(max_iterations=0)))
    counts = [int(x) for x in a.pairs.split(",") if x]
    if counts:
        pool = synthetic_jobs(ctx, dev, max(counts), a.n)
        for mode, kw in modes:
            for count in counts:
                measure(f"synthetic {mode}", pool[:count], kw, a.reps, num_cus, a.batched_only)
        for j in pool:
            j[0].close()
    if a.dino:
        jobs = dino_jobs(ctx, dev)
        for mode, kw in modes:
            measure(f"dino ring of triples {mode}", jobs, kw, a.reps, num_cus, a.batched_only)
        for j in jobs:
            j[0].close()


if __name__ == "__main__":
    main()
