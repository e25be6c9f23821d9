"""Cost of sfm_align_pairs against a loop of sfm_align_pair over the same links, and against sfm_register_views on the same
pairs (the neighbouring one-lane-per-hypothesis RANSAC): HIP events around the enqueued calls, one process.  For every list of
L links: a warm-up of every form, then three repetitions of [L single calls back to back | one batched call | one batched
registration], alternating; medians; the loop of the same run is the baseline.  Lists: L synthetic links of n records (eight
four-view scenes of tests/align_scene.py, 0.5 px noise, 15 % wrong matches on each side, 5 % wrong indices; every pair through
fillXU, estimateE and ONE sfm_refine_pairs; the registration takes pair a's records re-matched against pair b's second view), with
the default parameters; with --dino the ring of 36 links (i, i + 1) -> (i + 1, i + 2) of the committed dino frames; with --single
one link at n = 4096 and 16384 records at 4096 and 65536 hypotheses.  `splits` is the share count of the batched scoring launch,
recomputed here by the launcher's rule (csrc/align.hip: align_splits) from the device's CU count.
    python profiles/align_bench.py [--dino] [--single]
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/align_bench.py --links 630 --reps 1 --batched-only"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
import align_scene as AS  # noqa: E402


def splits_of(num_cus, hyps, jobs, nmax):
    hblocks = (hyps + 255) // 256
    blocks = hblocks * jobs
    return max(1, min((4 * num_cus + blocks - 1) // blocks, max(1, nmax // 128)))


def dev_records(dev, rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), 576)).to(dev)


def third_view_records(sc, v):
    """Pair v's records re-matched against view v + 2 (pair v + 1's second view)."""
    rec = sc["pairs"][v]["sift"].copy()
    uv = sc["uv"][v + 2][sc["perm"][v]]
    rec["match_xpos"], rec["match_ypos"] = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    rec["match"] = sc["inv"][v + 2][sc["perm"][v]].astype(np.int32)
    return rec


def synthetic_links(ctx, dev, count, n, views=4):
    """(a, b, index, records of a against b's second view) per link; every scene instance is a chain of views - 1 pairs."""
    scenes = [AS.build(n, 7 + s, views=views) for s in range(8)]
    up = [([dev_records(dev, P["sift"]) for P in sc["pairs"]], [torch.from_numpy(L["index"]).to(dev) for L in sc["links"]],
           [dev_records(dev, third_view_records(sc, v)) for v in range(views - 2)]) for sc in scenes]
    links, pairs, k = [], [], 0
    while len(links) < count:
        sc, (recs, idx, rec3) = scenes[k % 8], up[k % 8]
        made = []
        for v, P in enumerate(sc["pairs"]):
            pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
            pair.fillXU(recs[v])
            pair.estimateE(S.default_params(n, seed=11 + k + v))
            made.append(pair)
        pairs += made
        for v in range(views - 2):
            links.append((made[v], made[v + 1], idx[v], rec3[v]))
        k += 1
    S.refine_pairs(pairs, max_iterations=20)
    return links[:count], pairs


def dino_links(ctx, dev):
    from helpers import read_pnm_grey, dino_frame, DINO_K, DINO_KINV, DINO_SIFT
    views = [read_pnm_grey(dino_frame(k)) for k in range(36)]
    max_pts = 8192
    _, counts = S.process_views(ctx, views, DINO_K, DINO_KINV, pairs=[(0, 1)], max_pts=max_pts, sift=DINO_SIFT, device=dev)
    block = ctx._views_block[:36 * (max_pts * 576 + 64)].view(36, max_pts * 576 + 64)
    pairs, idx = [], []
    for i in range(36):
        j = (i + 1) % 36
        ctx.match(block[i], counts[i], block[j], counts[j])           # writes view i's match fields; fillXU reads them next on the stream
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, counts[i])
        pair.fillXU(block[i])
        pair.estimateE()
        pairs.append(pair)
        idx.append(torch.empty(counts[i], dtype=torch.int32, device=dev))
        S.align_index_from_matches(ctx, block[i], counts[i], idx[-1])
    S.refine_pairs(pairs, max_iterations=20)
    for i in range(36):
        k = (i + 2) % 36
        ctx.match(block[i], counts[i], block[k], counts[k])           # view i re-matched against pair i + 1's second view
    return [(pairs[i], pairs[(i + 1) % 36], idx[i], block[i]) for i in range(36)], pairs


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report_of(t):
    r = S.AlignReport.from_buffer_copy(t.cpu().numpy().tobytes())
    return {f: getattr(r, f) for f, _ in S.AlignReport._fields_}


def measure(name, links, kw, reps, num_cus, batched_only=False, register=True):
    dev = links[0][2].device
    A, B, I, R3 = ([l[k] for l in links] for k in range(4))
    params = S.align_params(**kw)
    H = params.num_hypotheses
    outs = [S._align_buffers(torch, dev, a.num_points, H) for a in A]
    outs2 = [S._align_buffers(torch, dev, a.num_points, H) for a in A]
    rparams = S.register_params(num_hypotheses=H)

    def loop():
        for a, b, i, o in zip(A, B, I, outs2):
            a.align_to_enqueue(b, i, params, *o)

    def batched():
        S.align_pairs_enqueue(A, B, I, params, outs)

    def registration():
        S.register_views_enqueue(A, R3, rparams)

    if not batched_only:
        loop()
    batched()
    if register:
        registration()
    torch.cuda.synchronize()
    reports = [report_of(o[4]) for o in outs]
    same = "n/a" if batched_only else str(all(bool((x == y).all()) for o, o2 in zip(outs, outs2) for x, y in zip(o, o2)))
    t_loop, t_batch, t_reg = [], [], []
    for _ in range(reps):
        if not batched_only:
            t_loop.append(timed(loop))
        t_batch.append(timed(batched))
        if register:
            t_reg.append(timed(registration))
    cand = [r["num_candidates"] for r in reports]
    inl = [r["num_inliers"] for r in reports]
    iters = [r["iterations"] for r in reports]
    degenerate = sum(r["status"] == S.REFINE_DEGENERATE for r in reports)
    nmax = max(a.num_points for a in A)
    line = (f"{name}: L={len(links)} H={H} n={min(a.num_points for a in A)}..{nmax} candidates={min(cand)}..{max(cand)} inliers={min(inl)}..{max(inl)} "
            f"iterations={min(iters)}..{max(iters)} degenerate={degenerate} splits batched={splits_of(num_cus, H, len(links), nmax)} "
            f"single={splits_of(num_cus, H, 1, min(a.num_points for a in A))}..{splits_of(num_cus, H, 1, nmax)} outputs equal: {same} | ")
    if not batched_only:
        line += "loop ms " + " ".join(f"{t:.3f}" for t in t_loop) + " | "
    line += "batched ms " + " ".join(f"{t:.3f}" for t in t_batch)
    if register:
        line += " | register_views ms " + " ".join(f"{t:.3f}" for t in t_reg)
    ba = float(np.median(t_batch))
    line += f" | medians"
    if not batched_only:
        lo = float(np.median(t_loop))
        line += f" loop {lo:.3f} / batched {ba:.3f} ms = {lo / ba:.1f}x, {1e3 * lo / len(links):.1f} -> {1e3 * ba / len(links):.1f} us per link"
    else:
        line += f" batched {ba:.3f} ms"
    if register:
        line += f"; register_views {float(np.median(t_reg)):.3f} ms = {ba / float(np.median(t_reg)):.2f}x of it"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--batched-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {num_cus} compute units", flush=True)
    counts = [int(x) for x in a.links.split(",") if x]
    if counts:
        links, pairs = synthetic_links(ctx, dev, max(counts), a.n)
        for count in counts:
            measure("synthetic", links[:count], {}, a.reps, num_cus, a.batched_only, register=not a.batched_only)
        for p in pairs:
            p.close()
    if a.single:
        for n in (4096, 16384):
            links, pairs = synthetic_links(ctx, dev, 1, n, views=3)
            for H in (4096, 65536):
                measure("one link", links, dict(num_hypotheses=H), a.reps, num_cus, register=True)
            for p in pairs:
                p.close()
    if a.dino:
        links, pairs = dino_links(ctx, dev)
        measure("dino ring", links, {}, a.reps, num_cus, a.batched_only, register=not a.batched_only)
        for p in pairs:
            p.close()


if __name__ == "__main__":
    main()
