"""Cost of sfm_adjust_view / sfm_adjust_views: a loop of single calls against one batched call over the same pairs, HIP events
around the enqueued calls, one process, medians of three; next to each, sfm_refine_pairs on the same pairs in the same run, for
scale, and the batched call at 0 iterations (gather, compaction, one cost pass, scatter: what a call costs before any iteration),
from which the cost per iteration follows.  Lists as profiles/view_points_bench.py builds them (every pair refined, registered
and triangulated over its view): P synthetic pairs of n points, the ring of 36 dino triples (--dino), one pair at each size of
--single.  Results: profiles/adjust_bench.txt."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
import view_points_bench as VB  # noqa: E402


def measure(name, jobs, reps, dev):
    pairs, recs = [j[0] for j in jobs], [j[1] for j in jobs]
    vps = S.triangulate_views(pairs, recs)
    ins = [(r, torch.from_numpy(v[0]).to(dev), torch.from_numpy(v[1]).to(dev)) for r, v in zip(recs, vps)]
    params, zero, rparams = S.adjust_params(), S.adjust_params(max_iterations=0), S.refine_params()
    mk = lambda: [S._adjust_buffers(torch, dev, p.num_points) for p in pairs]
    outs_loop, outs_batch = mk(), mk()

    def loop():
        for pair, i, o in zip(pairs, ins, outs_loop):
            pair.adjust_view_enqueue(*i, params, *o)

    def batched():
        S.adjust_views_enqueue(pairs, ins, params, outs_batch)

    def batched_zero():
        S.adjust_views_enqueue(pairs, ins, zero, outs_batch)

    def refine():
        S.refine_pairs_enqueue(pairs, rparams)

    loop()
    torch.cuda.synchronize()
    single = [[t.cpu().numpy().copy() for t in o] for o in outs_loop]
    batched_zero()
    torch.cuda.synchronize()
    batched()
    torch.cuda.synchronize()
    both = [[t.cpu().numpy().copy() for t in o] for o in outs_batch]
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for x, y in zip(single, both) for a, b in zip(x, y))
    reports = [S.AdjustReport.from_buffer_copy(b[4].tobytes()) for b in both]
    t_loop, t_batch, t_zero, t_ref = [], [], [], []
    for _ in range(reps):
        t_loop.append(VB.timed(loop)); t_batch.append(VB.timed(batched)); t_zero.append(VB.timed(batched_zero)); t_ref.append(VB.timed(refine))
    lo, ba, ze, rf = (float(np.median(t)) for t in (t_loop, t_batch, t_zero, t_ref))
    n = [p.num_points for p in pairs]
    used = [r.num_points for r in reports]
    iters = [r.iterations for r in reports]
    per_iter = 1e3 * (ba - ze) / max(iters) if max(iters) else float("nan")      # the longest chain bounds the batched call
    print(f"{name}: P={len(pairs)} n={min(n)}..{max(n)} used {min(used)}..{max(used)} iterations {min(iters)}..{max(iters)} "
          f"degenerate {sum(r.status == S.REFINE_DEGENERATE for r in reports)} outputs equal: {same} | "
          f"loop ms {' '.join(f'{t:.3f}' for t in t_loop)} | batched ms {' '.join(f'{t:.3f}' for t in t_batch)} | "
          f"medians {lo:.3f} / {ba:.3f} ms = {lo / ba:.1f}x, {1e3 * lo / len(pairs):.1f} -> {1e3 * ba / len(pairs):.2f} us per pair | "
          f"batched at 0 iterations {ze:.3f} ms, so {per_iter:.1f} us per iteration of the longest chain | "
          f"sfm_refine_pairs on the same pairs {rf:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--single", default="2155,4096,16384")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# library: {os.path.basename(S.LIB_PATH)}, {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    for n in [int(x) for x in a.single.split(",") if x]:
        jobs = VB.synthetic_jobs(ctx, dev, 1, n)
        measure("one pair", jobs, a.reps, dev)
        jobs[0][0].close()
    counts = [int(x) for x in a.pairs.split(",") if x]
    if counts:
        pool = VB.synthetic_jobs(ctx, dev, max(counts), a.n)
        for count in counts:
            measure("synthetic", pool[:count], a.reps, dev)
        for j in pool:
            j[0].close()
    if a.dino:
        jobs = VB.dino_jobs(ctx, dev)
        measure("dino ring of triples", jobs, a.reps, dev)
        for j in jobs:
            j[0].close()


if __name__ == "__main__":
    main()
