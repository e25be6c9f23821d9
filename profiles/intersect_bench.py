"""Cost of one sfm_intersect_tracks call: HIP events around the enqueued call, one process, medians of three.
Rings: fuse_ring_scene.build(k, 2155, seed) on the override path (profiles/fuse_ring_bench.py's device_ring), fused by
sfm_fuse_ring and adjusted by sfm_adjust_ring on the device; the call runs under the adjusted cameras with and without d_skip =
d_used, beside the whole sfm_fuse_ring call on the same ring in the same run (its points kernel walks the same lists with the same
LM: the kernels themselves stand side by side in the rocprofv3 split below).  Every ring also runs at wave_min_views = INT32_MAX,
16, 32, 64 and 128, with the outputs of every setting compared.
Synthetic table: 1 + 1000 tracks over a ring of 4096 pairs -- one track of 4097 views (round the whole ring) and 1000 of two -- at
the same settings: what one over-long track costs by lane and by wavefront.
    python profiles/intersect_bench.py > profiles/intersect_bench.txt
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/intersect_bench.py --pairs 630 --reps 1 --no-synthetic"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
import fuse_ring_scene as RS  # noqa: E402
import intersect_scene as IS  # noqa: E402
from align_bench import dev_records, timed  # noqa: E402
from fuse_ring_bench import device_ring  # noqa: E402

INT32_MAX = 2 ** 31 - 1
SETTINGS = (INT32_MAX, 16, 32, 64, 128)


def caller(ctx, pairs, table, outs, **kw):
    """One sfm_intersect_tracks call with its ctypes arguments built once, outside the events."""
    k = len(pairs)
    handles = (C.c_void_p * k)(*[p._h.value for p in pairs])
    i = S.IntersectIn(C.cast(handles, C.POINTER(C.c_void_p)), *[t.data_ptr() if t is not None else None for t in table])
    o = S.IntersectOut(*[t.data_ptr() for t in outs])
    p = S.intersect_params(**kw)
    L = S.lib()

    def call():
        assert L.sfm_intersect_tracks(ctx._h, C.byref(i), k, C.byref(p), C.byref(o)) == S.OK, L.sfm_last_error()
    call.keep = (handles, i, o, p)
    return call


def sweep(ctx, pairs, table, N, dev, reps):
    """The call at every setting of wave_min_views: medians in ms, and whether every setting wrote the same bytes."""
    outs = S.intersect_tracks_buffers(dev, N)
    for t in outs:
        t.zero_()
    ms, first, same = {}, None, True
    for w in SETTINGS:
        call = caller(ctx, pairs, table, outs, wave_min_views=w)
        call()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        same = same and (first is None or all(bool((a.view(torch.uint8) == b.view(torch.uint8)).all()) for a, b in zip(first, got)))
        first = first or got
        ms[w] = float(np.median([timed(call) for _ in range(reps)]))
    return ms, same, outs


def fmt(ms):
    return ", ".join(f"{'INT32_MAX' if w == INT32_MAX else w}: {t:.3f}" for w, t in ms.items())


def ring(ctx, dev, k, n, seed, reps):
    t0 = time.perf_counter()
    sc, rg = RS.build(k, n, seed)
    pairs, pin, lin, keep, host_ring = device_ring(ctx, dev, rg)
    built = time.perf_counter() - t0
    N = k * n
    fouts = S._fuse_buffers(torch, dev, k, N)
    rep = torch.zeros(C.sizeof(S.FuseRingReport), dtype=torch.uint8, device=dev)
    fo, rparams, L = S.FuseOut(*[t.data_ptr() for t in fouts]), S.fuse_ring_params(), S.lib()

    def fuse():
        assert L.sfm_fuse_ring(ctx._h, pin, k, lin, C.byref(rparams), C.byref(fo), rep.data_ptr()) == S.OK, L.sfm_last_error()
    fuse()
    torch.cuda.synchronize()
    t_fuse = float(np.median([timed(fuse) for _ in range(reps)]))
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = fouts
    adj = S.adjust_ring_buffers(dev, k, N)
    t_adj = timed(lambda: S.adjust_ring_enqueue(ctx, pairs, (root, cams, off, ocam, orec, pts, flags, counts, rep), S.adjust_ring_params(), adj))
    arep = adj[4].cpu().numpy().view(S.ADJUST_RING_REPORT_DTYPE)[0]
    T = int(counts[0].item())
    lens = np.diff(off.cpu().numpy()[:T + 1])
    table = [adj[0], off, ocam, orec, adj[1], flags, counts]
    print(f"ring: k={k} n={n} N={N} (scene built in {built:.1f} s): {T} tracks, {float(lens.mean()):.2f} views in the mean, longest {int(lens.max())}, "
          f"{int((lens > 8).sum())} over-long; adjust_ring used {int(arep['num_tracks'])} tracks ({t_adj:.1f} ms); sfm_fuse_ring {t_fuse:.3f} ms", flush=True)
    for what, skip in (("no d_skip", None), ("d_skip = d_used", adj[2])):
        ms, same, outs = sweep(ctx, pairs, table + [skip], N, dev, reps)
        c = outs[3].cpu().numpy()
        print(f"  {what}: counts {c.tolist()}; ms at wave_min_views {fmt(ms)}; every setting the same bytes: {same}; "
              f"default (32) / sfm_fuse_ring = {ms[32] / t_fuse:.2f}", flush=True)
    for p in pairs:
        p.close()


def synthetic(ctx, dev, reps, k=4096, short=1000, n=16):
    t0 = time.perf_counter()
    centre = np.array([0.0, 0.0, 10.0])
    views = []
    for v in range(k):
        a = 2.0 * np.pi * v / k
        views.append(IS._look_at(centre + 10.0 * np.array([np.sin(a), 0.15 * np.sin(3.0 * a), -np.cos(a)]), centre) if v else (np.eye(3), np.zeros(3)))
    tracks = [(0, k + 1, 3)] + [(1 + (4 * i) % (k - 2), 2, 1) for i in range(short)]
    rng = np.random.default_rng(5)
    P = rng.uniform(-1.0, 1.0, (len(tracks), 3)) + centre
    chain, tb = IS._table(k, n, views, tracks, P, 5)
    pairs = []
    for Q in chain["pairs"]:
        pair = S.ImagePair(ctx, chain["K"], chain["Kinv"], 2, Q["n"])
        pair.fillXU(dev_records(dev, Q["sift"]))
        pairs.append(pair)
    N = k * n
    pts = tb["points"].copy()
    pts[:3] += 0.5 * rng.standard_normal((3, len(tracks))).astype(np.float32)      # columns 5 % of the depth off
    arrays = IS.table_arrays(dict(tb, points=pts), k, N)
    table = [torch.from_numpy(a).to(dev) if a is not None else None for a in arrays]
    built = time.perf_counter() - t0
    ms, same, outs = sweep(ctx, pairs, table, N, dev, reps)
    c = outs[3].cpu().numpy()
    X = outs[0].cpu().numpy().reshape(4, N)[:3, 0]
    print(f"synthetic: {k} pairs x {n} records (built in {built:.1f} s), 1 track of {k + 1} views + {short} of 2: counts {c.tolist()}, the long track "
          f"{np.linalg.norm(X - P[0]) / 10.0:.2g} of its depth from the truth; ms at wave_min_views {fmt(ms)}; every setting the same bytes: {same}; "
          f"by lane / by wavefront (32) = {ms[INT32_MAX] / ms[32]:.1f}", flush=True)
    for p in pairs:
        p.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-synthetic", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print("## profiles/intersect_bench.py: sfm_intersect_tracks behind sfm_fuse_ring and sfm_adjust_ring, HIP events, medians of "
          f"{a.reps}", flush=True)
    print(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    for k in [int(x) for x in a.pairs.split(",") if x]:
        ring(ctx, dev, k, a.n, a.seed, a.reps)
    if not a.no_synthetic:
        synthetic(ctx, dev, a.reps)


if __name__ == "__main__":
    main()
