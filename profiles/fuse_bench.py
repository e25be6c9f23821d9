"""Cost of one sfm_fuse_chain call against sfm_align_pairs on the same chain and against the host build of the same arithmetic
(tests/hostcheck/libfusecheck.so) on this machine's CPU: HIP events around the enqueued calls, one process.  For every chain of
k pairs: a warm-up of both calls, then three repetitions of [one sfm_align_pairs | one sfm_fuse_chain], alternating; medians.  The
ctypes arrays of a call are built once, outside the events.  Chains: k synthetic pairs of n records -- six-view scenes of
tests/align_scene.py (0.5 px noise, 15 % wrong matches on each side, 5 % wrong indices), five pairs each, one behind the other;
the link between two scenes has no index and comes out degenerate, so a chain of k pairs has k / 5 segments -- every pair through
fillXU, estimateE and ONE sfm_refine_pairs, the links by ONE sfm_align_pairs; with --dino the 36 pairs (i, i + 1) of the committed
dino frames as a chain of 35 links.
    python profiles/fuse_bench.py [--dino]
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/fuse_bench.py --pairs 630 --reps 1 --fuse-only
(with --iterations 0 the points kernel's share that is not the Levenberg-Marquardt: start, acceptance test, stores)"""
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
import align_scene as AS  # noqa: E402
import fuse_scene as FS  # noqa: E402
from align_bench import dev_records, timed  # noqa: E402


def synthetic_chain(ctx, dev, count, n, views=6):
    """(pairs, index tensors of the count - 1 links): scene instances of views - 1 pairs, one behind the other."""
    scenes = [AS.build(n, 7 + s, views=views) for s in range(8)]
    up = [([dev_records(dev, P["sift"]) for P in sc["pairs"]], [torch.from_numpy(L["index"]).to(dev) for L in sc["links"]]) for sc in scenes]
    none = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pairs, idx, k = [], [], 0
    while len(pairs) < count:
        sc, (recs, links) = scenes[k % 8], up[k % 8]
        for v, P in enumerate(sc["pairs"]):
            pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
            pair.fillXU(recs[v])
            pair.estimateE(S.default_params(n, seed=11 + k + v))
            pairs.append(pair)
            idx.append(links[v] if v < views - 2 else none)
        k += 1
    pairs, idx = pairs[:count], idx[:count - 1]
    S.refine_pairs(pairs, max_iterations=20)
    return pairs, idx


def dino_chain(ctx, dev):
    from align_bench import dino_links
    links, pairs = dino_links(ctx, dev)
    return pairs, [l[2] for l in links[:35]]


def read_back(pairs, idx, aouts, K, Kinv):
    """The state the call reads, as the chain dict of the host build."""
    ps, ls = [], []
    for p in pairs:
        _, used = p.get_reprojection_errors()
        P4 = p.get_refined_pose()[0]
        ps.append(dict(n=p.num_points, ld=p.num_points, points=p.get_refined_points(), valid=used, X0=p.get_XU(S.BUF_X0), X1=p.get_XU(S.BUF_X1),
                       pose=np.concatenate([P4[:3, :3].ravel(), P4[:3, 3]]).astype(np.float32)))
    for d_index, a in zip(idx, aouts):
        rep = S.AlignReport.from_buffer_copy(a[4].cpu().numpy().tobytes())
        ls.append(dict(index=d_index.cpu().numpy(), sim=a[0].cpu().numpy()[:13].copy(), inlier=a[1].cpu().numpy(), err=a[2].cpu().numpy(),
                       status=rep.status))
    return dict(K=K, Kinv=Kinv, pairs=ps, links=ls)


def measure(name, ctx, pairs, idx, K, Kinv, reps, fuse_only=False, host=True, iterations=5):
    dev = idx[0].device
    k = len(pairs)
    N = sum(p.num_points for p in pairs)
    aparams, fparams = S.align_params(), S.fuse_params(max_iterations=iterations)
    aouts = [S._align_buffers(torch, dev, p.num_points, aparams.num_hypotheses) for p in pairs[:-1]]
    outs = S._fuse_buffers(torch, dev, k, N)
    # the ctypes arrays of both calls, built once
    ha = (C.c_void_p * (k - 1))(*[p._h.value for p in pairs[:-1]])
    hb = (C.c_void_p * (k - 1))(*[p._h.value for p in pairs[1:]])
    hi = (C.c_void_p * (k - 1))(*[t.data_ptr() for t in idx])
    ao = (S.AlignOut * (k - 1))(*[S.AlignOut(*[t.data_ptr() for t in a]) for a in aouts])
    pin = (S.FusePairIn * k)(*[S.FusePairIn(p._h.value, None, None, None) for p in pairs])
    lin = (S.FuseLinkIn * (k - 1))(*[S.FuseLinkIn(i.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[4].data_ptr()) for i, a in zip(idx, aouts)])
    fo = S.FuseOut(*[t.data_ptr() for t in outs])
    L = S.lib()

    def align():
        assert L.sfm_align_pairs(ha, hb, k - 1, hi, C.byref(aparams), ao) == S.OK, L.sfm_last_error()

    def fuse():
        assert L.sfm_fuse_chain(ctx._h, pin, k, lin, C.byref(fparams), C.byref(fo)) == S.OK, L.sfm_last_error()

    align(); fuse()
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    t_align, t_fuse = [], []
    for _ in range(reps):
        if not fuse_only:
            t_align.append(timed(align))
        t_fuse.append(timed(fuse))
    res = S._fuse_results(outs, k, N)
    same = all(bool((x == y).all()) for x, y in zip((first[q] for q in (1, 3, 10)), (outs[q] for q in (1, 3, 10))))
    line = (f"{name}: k={k} N={N} n={min(p.num_points for p in pairs)}..{max(p.num_points for p in pairs)} {res['counts']} "
            f"second call equal: {same} | fuse ms " + " ".join(f"{t:.3f}" for t in t_fuse))
    fu = float(np.median(t_fuse))
    if not fuse_only:
        al = float(np.median(t_align))
        line += " | align_pairs ms " + " ".join(f"{t:.3f}" for t in t_align)
    if host and not fuse_only:
        HL = FS.host_lib()
        state = read_back(pairs, idx, aouts, K, Kinv)
        t_host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            want = FS.run_host(HL, S, state, max_iterations=iterations)
            t_host.append(1e3 * (time.perf_counter() - t0))
        equal = want["counts"] == res["counts"] and all(np.array_equal(want[q], res[q]) for q in ("track", "track_offset", "obs_cam", "obs_record", "flags")) \
            and np.array_equal(want["points"].view(np.uint8), res["points"].view(np.uint8))
        line += " | host build ms " + " ".join(f"{t:.1f}" for t in t_host) + f" (outputs equal: {equal})"
    line += f" | medians fuse {fu:.3f} ms = {1e3 * fu / k:.2f} us per pair, {1e6 * fu / max(N, 1):.2f} ns per node"
    if not fuse_only:
        line += f"; align_pairs {al:.3f} ms, fuse = {fu / al:.2f}x of it"
    if host and not fuse_only:
        line += f"; host build {float(np.median(t_host)):.1f} ms = {float(np.median(t_host)) / fu:.0f}x"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--fuse-only", action="store_true")
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    counts = [int(x) for x in a.pairs.split(",") if x]
    if counts:
        K, Kinv = AS.camera()
        pairs, idx = synthetic_chain(ctx, dev, max(counts), a.n)
        for count in counts:
            measure("synthetic", ctx, pairs[:count], idx[:count - 1], K, Kinv, a.reps, a.fuse_only, iterations=a.iterations)
        for p in pairs:
            p.close()
    if a.dino:
        from helpers import DINO_K, DINO_KINV
        pairs, idx = dino_chain(ctx, dev)
        measure("dino chain", ctx, pairs, idx, DINO_K, DINO_KINV, a.reps, a.fuse_only, iterations=a.iterations)
        for p in pairs:
            p.close()


if __name__ == "__main__":
    main()
