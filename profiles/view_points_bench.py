"""Cost of sfm_triangulate_view / sfm_triangulate_views: a loop of single calls against one batched call over the same pairs, HIP
events around the enqueued calls, one process, medians of three; next to each, sfm_register_views on the same inputs in the same
run, for scale.  Lists: P synthetic pairs of n points (eight scenes with 0.5 px noise and 30 % outliers x eight third views with
the same, 10 % gated; per pair fillXU + estimateE, ONE sfm_refine_pairs, ONE sfm_register_views), the ring of 36 triples
(i, i + 1, i + 2) of the committed dino frames (--dino), and one pair at each size of --single.
--label names the build in the header line (profiles/view_points_bench.txt holds two runs: the product and a build with the DLT
in place on every lane with a new point, a form that was measured once and not kept).
--dump FILE writes the first list's outputs (points, flags, err, counts of every pair) so that two builds can be compared."""
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


def synthetic_jobs(ctx, dev, count, n):
    """(pair, records of view 3) per job, every pair refined and registered."""
    scenes = []
    for s in range(8):
        sc = synth.two_view_scene(n, seed=7 + s, noise_px=0.5, outlier_frac=0.3)
        d_sift = torch.from_numpy(sc["sift"].view(np.uint8).reshape(n, 576)).to(dev)
        views = []
        for v in range(8):
            rec, _ = RS.third_view(sc, seed=100 * s + v, noise_px=0.5, outlier_frac=0.3, gated_frac=0.1)
            views.append(torch.from_numpy(rec.view(np.uint8).reshape(n, 576)).to(dev))
        scenes.append((sc, d_sift, views))
    pairs, recs = [], []
    for k in range(count):
        sc, d_sift, views = scenes[k % 8]
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
        pair.fillXU(d_sift)
        pair.estimateE(S.default_params(n, num_hypotheses=1024, seed=5 + k))
        pairs.append(pair); recs.append(views[(k // 8) % 8])
    S.refine_pairs(pairs, max_iterations=20)
    S.register_views(pairs, recs)
    return list(zip(pairs, recs))


def dino_jobs(ctx, dev):
    from helpers import read_pnm_grey, dino_frame, DINO_K, DINO_KINV, DINO_SIFT
    views = [read_pnm_grey(dino_frame(k)) for k in range(36)]
    max_pts = 8192
    _, counts = S.process_views(ctx, views, DINO_K, DINO_KINV, pairs=[(0, 1)], max_pts=max_pts, sift=DINO_SIFT, device=dev)
    block = ctx._views_block[:36 * (max_pts * 576 + 64)].view(36, max_pts * 576 + 64)
    pairs = []
    for i in range(36):
        j = (i + 1) % 36
        ctx.match(block[i], counts[i], block[j], counts[j])
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, counts[i])
        pair.fillXU(block[i])
        pair.estimateE()
        pairs.append(pair)
    S.refine_pairs(pairs, max_iterations=20)
    for i in range(36):
        k = (i + 2) % 36
        ctx.match(block[i], counts[i], block[k], counts[k])
    S.register_views(pairs, [block[i] for i in range(36)])
    return [(pairs[i], block[i]) for i in range(36)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(name, jobs, reps, dev, dump=None):
    pairs, recs = [j[0] for j in jobs], [j[1] for j in jobs]
    params, rparams = S.view_points_params(), S.register_params()
    counts = torch.empty((len(pairs), 8), dtype=torch.int32, device=dev)
    mk = lambda: [(torch.empty((4, p.num_points), dtype=torch.float32, device=dev), torch.empty(p.num_points, dtype=torch.uint8, device=dev),
                   torch.empty(p.num_points, dtype=torch.float32, device=dev), counts[i]) for i, p in enumerate(pairs)]
    outs_loop, outs_batch = mk(), mk()

    def loop():
        for pair, d, o in zip(pairs, recs, outs_loop):
            pair.triangulate_view_enqueue(d, params, *o)

    def batched():
        S.triangulate_views_enqueue(pairs, recs, params, outs_batch)

    def register():
        S.register_views_enqueue(pairs, recs, rparams)

    loop()
    torch.cuda.synchronize()
    single = [[t.cpu().numpy().copy() for t in o] for o in outs_loop]
    batched()
    torch.cuda.synchronize()
    both = [[t.cpu().numpy().copy() for t in o] for o in outs_batch]
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for x, y in zip(single, both) for a, b in zip(x, y))
    register()
    torch.cuda.synchronize()
    t_loop, t_batch, t_reg = [], [], []
    for _ in range(reps):
        t_loop.append(timed(loop)); t_batch.append(timed(batched)); t_reg.append(timed(register))
    hist = np.sum([b[3][:5] for b in both], 0)
    lo, ba, rg = (float(np.median(t)) for t in (t_loop, t_batch, t_reg))
    n = [p.num_points for p in pairs]
    print(f"{name}: P={len(pairs)} n={min(n)}..{max(n)} classes (unseen new refined new-rejected kept) {hist.tolist()} outputs equal: {same} | "
          f"loop ms {' '.join(f'{t:.3f}' for t in t_loop)} | batched ms {' '.join(f'{t:.3f}' for t in t_batch)} | "
          f"medians {lo:.3f} / {ba:.3f} ms = {lo / ba:.1f}x, {1e3 * lo / len(pairs):.1f} -> {1e3 * ba / len(pairs):.2f} us per pair | "
          f"sfm_register_views on the same pairs {rg:.3f} ms", flush=True)
    if dump:
        np.savez(dump, **{f"{k}_{name_}": a for k, b in enumerate(both) for name_, a in zip(("points", "flags", "err", "counts"), b)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--single", default="4096,16384")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# {a.label or 'library'}: {os.path.basename(S.LIB_PATH)}, {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    counts = [int(x) for x in a.pairs.split(",") if x]
    if counts:
        pool = synthetic_jobs(ctx, dev, max(counts), a.n)
        for k, count in enumerate(counts):
            measure("synthetic", pool[:count], a.reps, dev, a.dump if k == 0 else None)
        for j in pool:
            j[0].close()
    if a.dino:
        jobs = dino_jobs(ctx, dev)
        measure("dino ring of triples", jobs, a.reps, dev)
        for j in jobs:
            j[0].close()
    for n in [int(x) for x in a.single.split(",") if x]:
        jobs = synthetic_jobs(ctx, dev, 1, n)
        measure("one pair", jobs, a.reps, dev)
        jobs[0][0].close()


if __name__ == "__main__":
    main()
