"""Cost of one sfm_adjust_chain call at 0 and at 10 iterations against sfm_fuse_chain on the same chain and against the host build
of the same arithmetic (tests/hostcheck/libchainadjustcheck.so) on this machine's CPU: HIP events around the enqueued calls, one
process, medians of three (the host build: one run).  The chains are fuse_bench.py's: k synthetic pairs of 2155 records (six-view
scenes, five pairs each, one behind the other: k / 5 segments) and, with --dino, the 36 pairs of the committed dino frames.  The
fused model stays on the device between the two calls.  At the end the per-iteration cost (the 10-iteration call less the
0-iteration call, over the iterations that ran) fitted by least squares to fixed + per observation + per camera block.
    python profiles/chain_adjust_bench.py [--dino]
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/chain_adjust_bench.py --pairs 630 --reps 1 --adjust-only
A long uncut chain (none of the chains above has a segment of more than 10 cameras): --strip K,N is ONE segment of K cameras with N
records per pair (tests/chain_adjust_scene.py: strip), built without sfm_fuse_chain; the call at 10 and 0 iterations, and under
rocprofv3 the solve kernel's time for that segment:
    rocprofv3 --kernel-trace --stats -- python profiles/chain_adjust_bench.py --pairs "" --strip 630,65 --reps 1"""
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
import chain_adjust_scene as CS  # noqa: E402
from align_bench import timed  # noqa: E402
from fuse_bench import dino_chain, read_back, synthetic_chain  # noqa: E402


def measure(name, ctx, pairs, idx, K, Kinv, reps, adjust_only=False, host=True, views=8):
    dev = idx[0].device
    k = len(pairs)
    N = sum(p.num_points for p in pairs)
    aparams, fparams = S.align_params(), S.fuse_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, aparams.num_hypotheses) for p in pairs[:-1]]
    S.align_pairs_enqueue(pairs[:-1], pairs[1:], idx, aparams, aouts)
    fouts = S._fuse_buffers(torch, dev, k, N)
    outs = S.adjust_chain_buffers(dev, k, N)
    pin = (S.FusePairIn * k)(*[S.FusePairIn(p._h.value, None, None, None) for p in pairs])
    lin = (S.FuseLinkIn * (k - 1))(*[S.FuseLinkIn(i.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[4].data_ptr()) for i, a in zip(idx, aouts)])
    fo = S.FuseOut(*[t.data_ptr() for t in fouts])
    handles = (C.c_void_p * k)(*[p._h.value for p in pairs])
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = fouts
    ci = S.AdjustChainIn(C.cast(handles, C.POINTER(C.c_void_p)), *[t.data_ptr() for t in (root, cams, off, ocam, orec, pts, flags, counts)])
    co = S.AdjustChainOut(*[t.data_ptr() for t in outs])
    p0, p10 = S.adjust_chain_params(max_iterations=0, max_track_views=views), S.adjust_chain_params(max_iterations=10, max_track_views=views)
    L = S.lib()

    def fuse():
        assert L.sfm_fuse_chain(ctx._h, pin, k, lin, C.byref(fparams), C.byref(fo)) == S.OK, L.sfm_last_error()

    def adjust(p):
        return lambda: L.sfm_adjust_chain(ctx._h, C.byref(ci), k, C.byref(p), C.byref(co)) == S.OK or sys.exit(L.sfm_last_error())

    fuse(); adjust(p0)(); adjust(p10)()
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    t_fuse, t_0, t_10 = [], [], []
    for _ in range(reps):
        if not adjust_only:
            t_fuse.append(timed(fuse))
            t_0.append(timed(adjust(p0)))
        t_10.append(timed(adjust(p10)))
    same = all(bool((x == y).all()) for x, y in zip(first, outs))
    fres = S._fuse_results(fouts, k, N)
    T = fres["counts"]["tracks"]
    res = S.adjust_chain_results(outs, k, N, T)
    rep = res["reports"][res["reports"]["root"] == np.arange(k)]
    live = rep[rep["status"] != S.REFINE_DEGENERATE]
    iters = float(live["iterations"].max()) if len(live) else 0.0
    line = (f"{name}: k={k} N={N} tracks {T} observations {fres['counts']['observations']} longest {fres['counts']['longest_track']} | segments {len(rep)} "
            f"({len(rep) - len(live)} degenerate), cameras in the largest {int(rep['num_cameras'].max())}, used tracks {int(rep['num_tracks'].sum())}, used observations "
            f"{int(rep['num_observations'].sum())}, over W = {views}: {int(rep['num_over_long'].sum())}, iterations {int(live['iterations'].min()) if len(live) else 0}.."
            f"{int(iters)}, rms (largest segment) {float(rep[np.argmax(rep['num_cameras'])]['initial_rms_px']):.4f} -> {float(rep[np.argmax(rep['num_cameras'])]['final_rms_px']):.4f} px, "
            f"second call equal: {same} | adjust 10 it ms " + " ".join(f"{t:.3f}" for t in t_10))
    a10 = float(np.median(t_10))
    out = dict(k=k, obs=int(rep["num_observations"].sum()), a10=a10, iters=iters)
    if not adjust_only:
        a0, fu = float(np.median(t_0)), float(np.median(t_fuse))
        out.update(a0=a0)
        line += " | adjust 0 it ms " + " ".join(f"{t:.3f}" for t in t_0) + " | fuse ms " + " ".join(f"{t:.3f}" for t in t_fuse)
        line += f" | medians: adjust 10 it {a10:.3f} ms, 0 it {a0:.3f} ms, per iteration {(a10 - a0) / max(iters, 1):.3f} ms; fuse {fu:.3f} ms"
    if host and not adjust_only:
        HL = CS.host_lib()
        state = read_back(pairs, idx, aouts, K, Kinv)
        fused = CS.fused_arrays(fres, k, N)
        t0 = time.perf_counter()
        want = CS.run_host(HL, S, state, fused, max_iterations=10, max_track_views=views)
        th = 1e3 * (time.perf_counter() - t0)
        equal = all(np.ascontiguousarray(want[q]).tobytes() == np.ascontiguousarray(res[q]).tobytes() for q in ("cams", "points", "used", "err", "reports"))
        line += f"; host build {th:.0f} ms = {th / a10:.0f}x (outputs equal: {equal})"
    print(line, flush=True)
    return out


def measure_strip(ctx, dev, k, n, reps):
    chain, fused, _ = CS.strip(k, n)
    pairs = []
    for P in chain["pairs"]:
        pair = S.ImagePair(ctx, chain["K"], chain["Kinv"], 2, n)
        pair.fillXU(torch.from_numpy(np.ascontiguousarray(P["sift"]).view(np.uint8).reshape(n, 576)).to(dev))
        pairs.append(pair)
    N = k * n
    arrays = [torch.from_numpy(a).to(dev) for a in CS.fused_arrays(fused, k, N)]
    outs = S.adjust_chain_buffers(dev, k, N)
    handles = (C.c_void_p * k)(*[p._h.value for p in pairs])
    ci = S.AdjustChainIn(C.cast(handles, C.POINTER(C.c_void_p)), *[t.data_ptr() for t in arrays])
    co = S.AdjustChainOut(*[t.data_ptr() for t in outs])
    p0, p10 = S.adjust_chain_params(max_iterations=0), S.adjust_chain_params(max_iterations=10)
    L = S.lib()
    adjust = lambda p: (lambda: L.sfm_adjust_chain(ctx._h, C.byref(ci), k, C.byref(p), C.byref(co)) == S.OK or sys.exit(L.sfm_last_error()))
    adjust(p10)()
    torch.cuda.synchronize()
    t_0 = [timed(adjust(p0)) for _ in range(reps)]
    t_10 = [timed(adjust(p10)) for _ in range(reps)]
    rep = S.adjust_chain_results(outs, k, N, fused["counts"]["tracks"])["reports"][0]
    a0, a10 = float(np.median(t_0)), float(np.median(t_10))
    print(f"strip: ONE segment of {int(rep['num_cameras'])} cameras, N={N} tracks {int(rep['num_tracks'])} observations {int(rep['num_observations'])} longest "
          f"{fused['counts']['longest_track']} | iterations {int(rep['iterations'])}, accepted {int(rep['accepted'])}, rms {float(rep['initial_rms_px']):.4f} -> "
          f"{float(rep['final_rms_px']):.4f} px | adjust 10 it ms " + " ".join(f"{t:.3f}" for t in t_10) + " | adjust 0 it ms " + " ".join(f"{t:.3f}" for t in t_0) +
          f" | medians: 10 it {a10:.3f} ms, 0 it {a0:.3f} ms, per iteration {(a10 - a0) / max(int(rep['iterations']), 1):.3f} ms", flush=True)
    for p in pairs:
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--adjust-only", action="store_true")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--strip", default="", help="K,N: one segment of K cameras, N records per pair")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    counts = [int(x) for x in a.pairs.split(",") if x]
    rows = []
    if counts:
        K, Kinv = AS.camera()
        pairs, idx = synthetic_chain(ctx, dev, max(counts), a.n)
        for count in counts:
            rows.append(measure("synthetic", ctx, pairs[:count], idx[:count - 1], K, Kinv, a.reps, a.adjust_only, views=a.views))
        for p in pairs:
            p.close()
    if a.strip:
        measure_strip(ctx, dev, *[int(x) for x in a.strip.split(",")], a.reps)
    if a.dino:
        from helpers import DINO_K, DINO_KINV
        pairs, idx = dino_chain(ctx, dev)
        rows.append(measure("dino chain", ctx, pairs, idx, DINO_K, DINO_KINV, a.reps, a.adjust_only, views=a.views))
        for p in pairs:
            p.close()
    if len(rows) >= 3 and not a.adjust_only:
        A = np.array([[1.0, r["obs"], r["k"]] for r in rows])
        y = np.array([(r["a10"] - r["a0"]) / max(r["iters"], 1) for r in rows])
        x, res, rank, _ = np.linalg.lstsq(A, y, rcond=None)
        print(f"# per iteration, least squares over {len(rows)} chains (rank {rank}): fixed {1e3 * x[0]:.1f} us + {1e6 * x[1]:.3f} ns per used observation + "
              f"{1e3 * x[2]:.3f} us per camera block; fitted - measured (us): " + " ".join(f"{1e3 * v:.1f}" for v in A @ x - y), flush=True)


if __name__ == "__main__":
    main()
