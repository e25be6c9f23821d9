"""Cost of sfm_refine_pairs against a loop of sfm_refine_two_view over the same pairs: HIP events around the enqueued calls, one
process, 20 LM iterations each (min_rel_decrease = 0 so that every chain runs all 20: the conditions of r07_refine_bench.txt).
For every list of P pairs: a warm-up of both forms, then three repetitions of [P single calls back to back | one batched call],
alternating; the loop of the same run is the baseline.  Lists: P synthetic pairs of n correspondences (eight scenes, every pair
its own estimateE seed), and with --dino the 36-pair ring and all 630 pairs of the committed dino frames (features by
sfm_extract_views, per pair sfm_match + fillXU + estimateE with N / 8 hypotheses).
    python profiles/refine_pairs_bench.py [--dino]
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/refine_pairs_bench.py --pairs 630 --reps 1 --batched-only"""
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


def synthetic_pairs(ctx, dev, count, n, scenes):
    pairs = []
    for k in range(count):
        sc, d_sift = scenes[k % len(scenes)]
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
        pair.fillXU(d_sift)
        pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=1000 + k))
        pairs.append(pair)
    return pairs


def dino_pairs(ctx, dev, which):
    from helpers import read_pnm_grey, dino_frame, DINO_K, DINO_KINV, DINO_SIFT
    views = [read_pnm_grey(dino_frame(k)) for k in range(36)]
    max_pts = 8192
    _, counts = S.process_views(ctx, views, DINO_K, DINO_KINV, pairs=[(0, 1)], max_pts=max_pts, sift=DINO_SIFT, device=dev)
    block = ctx._views_block[:36 * (max_pts * 576 + 64)].view(36, max_pts * 576 + 64)
    pairs = []
    for i, j in which:
        ctx.match(block[i], counts[i], block[j], counts[j])           # writes view i's match fields; fillXU reads them next on the stream
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, counts[i])
        pair.fillXU(block[i])
        try:
            pair.estimateE()
        except S.SfmError as e:                                       # a pair of views too far apart for an estimate is left out
            print(f"dino pair {(i, j)} left out: {e}", flush=True)
            pair.close()
            continue
        pairs.append(pair)
    return pairs


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, pairs, params, reps, batched_only=False):
    def loop():
        for p in pairs:
            p.refine_enqueue(params)

    def batched():
        S.refine_pairs_enqueue(pairs, params)

    if not batched_only:
        loop()
    torch.cuda.synchronize()
    single = [p.get_refine_report() for p in pairs] if not batched_only else None
    batched()
    torch.cuda.synchronize()
    reports = [p.get_refine_report() for p in pairs]
    same = "n/a" if batched_only else str(reports == single)
    t_loop, t_batch = [], []
    for _ in range(reps):
        if not batched_only:
            t_loop.append(timed(loop))
        t_batch.append(timed(batched))
    iters = [r["iterations"] for r in reports]
    used = [r["num_used"] for r in reports]
    line = (f"{name}: P={len(pairs)} n={min(p.num_points for p in pairs)}..{max(p.num_points for p in pairs)} "
            f"used={min(used)}..{max(used)} iterations={min(iters)}..{max(iters)} reports equal: {same} | ")
    if not batched_only:
        line += "loop ms " + " ".join(f"{t:.3f}" for t in t_loop) + " | "
    line += "batched ms " + " ".join(f"{t:.3f}" for t in t_batch)
    if not batched_only:
        lo, ba = float(np.median(t_loop)), float(np.median(t_batch))
        line += f" | medians {lo:.3f} / {ba:.3f} ms = {lo / ba:.1f}x, {1e3 * ba / len(pairs):.1f} us per pair batched"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,36,256,257,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--batched-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    params = S.refine_params(max_iterations=a.iterations, min_rel_decrease=0.0)
    counts = [int(x) for x in a.pairs.split(",") if x]
    if counts:
        scenes = []
        for s in range(8):
            sc = synth.two_view_scene(a.n, seed=7 + s)
            scenes.append((sc, torch.from_numpy(sc["sift"].view(np.uint8).reshape(a.n, 576)).to(dev)))
        pool = synthetic_pairs(ctx, dev, max(counts), a.n, scenes)
        for count in counts:
            measure("synthetic", pool[:count], params, a.reps, a.batched_only)
        for p in pool:
            p.close()
    if a.dino:
        ring = [(k, (k + 1) % 36) for k in range(36)]
        full = [(i, j) for i in range(36) for j in range(i + 1, 36)]
        for name, which in (("dino ring", ring), ("dino all pairs", full)):
            pairs = dino_pairs(ctx, dev, which)
            measure(name, pairs, params, a.reps, a.batched_only)
            for p in pairs:
                p.close()


if __name__ == "__main__":
    main()
