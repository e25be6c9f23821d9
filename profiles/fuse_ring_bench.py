"""Cost of one sfm_fuse_ring call next to sfm_fuse_chain on the same ring, and against the host build of the same arithmetic
(tests/hostcheck/libfuseringcheck.so) on this machine's CPU: HIP events around the enqueued calls, one process.  For every ring of
k pairs: a warm-up of both calls, then three repetitions of [one sfm_fuse_chain over the first k - 1 links | one sfm_fuse_ring
over all k], alternating; medians.  The ctypes arrays of a call are built once, outside the events.  Rings: ring_scene.build(k,
2155, seed, pairs="all") (0.5 px noise, 15 % wrong matches, 5 % wrong indices) with the true links, on the override path: every
pair has fillXU, its points, flags and pose are uploaded (the calls read the same arrays either way).
Behind the rings the script runs profiles/fuse_bench.py -- sfm_fuse_chain on that script's own chains -- in a child process of its
own: on this tree, and with --parent DIR on the parent commit too, from a directory that holds the parent's sources and build,
    git archive <parent commit> | tar -x -C DIR && make -C DIR cuda-sfm_amd/lib/libsfm_amd.so tests/hostcheck/libfusecheck.so
so that both stand in one output, from one session on one box: sfm_fuse_chain must not move by more than the spread of the
parent's repetitions.  Every section of the output starts with a `##` line that says what ran.
    python profiles/fuse_ring_bench.py [--parent DIR] > profiles/fuse_ring_bench.txt
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/fuse_ring_bench.py --pairs 630 --reps 1 --no-host --ring-only"""
import argparse
import ctypes as C
import os
import subprocess
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
from align_bench import dev_records, timed  # noqa: E402


def device_ring(ctx, dev, ring):
    """The ring on the device: (pairs, FusePairIn array, FuseLinkIn array, what keeps the tensors alive, the host's ring)."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pairs, keep, host_pairs = [], [], []
    k = len(ring["pairs"])
    pin, lin = (S.FusePairIn * k)(), (S.FuseLinkIn * k)()
    for i, (P, L) in enumerate(zip(ring["pairs"], ring["links"])):
        pair = S.ImagePair(ctx, ring["K"], ring["Kinv"], 2, P["n"])
        pair.fillXU(dev_records(dev, P["sift"]))
        rep = S.AlignReport(); rep.status = int(L["status"])
        t = [d(P["points"]), d(P["valid"]), d(P["pose"]), d(L["index"]), d(L["sim"]), d(L["inlier"]), d(L["err"]),
             d(np.frombuffer(bytes(rep), np.uint8).copy())]
        pin[i] = S.FusePairIn(pair._h.value, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        lin[i] = S.FuseLinkIn(*[x.data_ptr() for x in t[3:]])
        pairs.append(pair); keep.append(t)
        host_pairs.append(dict(P, X0=pair.get_XU(S.BUF_X0), X1=pair.get_XU(S.BUF_X1), ld=P["n"]))
    return pairs, pin, lin, keep, dict(ring, pairs=host_pairs)


def measure(ctx, dev, k, n, seed, reps, host=True, iterations=5):
    t0 = time.perf_counter()
    sc, ring = RS.build(k, n, seed)
    pairs, pin, lin, keep, host_ring = device_ring(ctx, dev, ring)
    built = time.perf_counter() - t0
    N = k * n
    rparams = S.fuse_ring_params(max_iterations=iterations)
    chain_outs, ring_outs = S._fuse_buffers(torch, dev, k, N), S._fuse_buffers(torch, dev, k, N)
    rep = torch.empty(C.sizeof(S.FuseRingReport), dtype=torch.uint8, device=dev)
    co, ro = S.FuseOut(*[t.data_ptr() for t in chain_outs]), S.FuseOut(*[t.data_ptr() for t in ring_outs])
    L = S.lib()

    def chain():
        assert L.sfm_fuse_chain(ctx._h, pin, k, lin, C.byref(rparams.fuse), C.byref(co)) == S.OK, L.sfm_last_error()

    def fuse_ring():
        assert L.sfm_fuse_ring(ctx._h, pin, k, lin, C.byref(rparams), C.byref(ro), rep.data_ptr()) == S.OK, L.sfm_last_error()

    chain(); fuse_ring()
    torch.cuda.synchronize()
    first = [t.clone() for t in ring_outs]
    t_chain, t_ring = [], []
    for _ in range(reps):
        t_chain.append(timed(chain))
        t_ring.append(timed(fuse_ring))
    same = all(bool((x == y).all()) for x, y in zip((first[q] for q in (1, 3, 8, 10)), (ring_outs[q] for q in (1, 3, 8, 10))))
    res, cres = S._fuse_results(ring_outs, k, N), S._fuse_results(chain_outs, k, N)
    r = S.FuseRingReport.from_buffer_copy(rep.cpu().numpy().tobytes())
    report = {f: getattr(r, f) for f, _ in S.FuseRingReport._fields_}
    ch, rg = float(np.median(t_chain)), float(np.median(t_ring))
    line = (f"ring: k={k} N={N} n={n} (scene built in {built:.1f} s) chain {cres['counts']} | ring {res['counts']} status {report['status']} "
            f"proposals {report['seam_proposals']} ineligible {report['seam_ineligible']} seam tracks {report['seam_tracks']} "
            f"({report['seam_refined']} refined) second call equal: {same} | fuse_chain ms " + " ".join(f"{t:.3f}" for t in t_chain) +
            " | fuse_ring ms " + " ".join(f"{t:.3f}" for t in t_ring))
    if host:
        HL = RS.host_lib()
        t_host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            want = RS.run_host(HL, S, host_ring, max_iterations=iterations)
            t_host.append(1e3 * (time.perf_counter() - t0))
        equal = want["counts"] == res["counts"] and all(np.array_equal(want[q], res[q]) for q in ("track", "track_offset", "obs_cam", "obs_record", "flags")) \
            and np.array_equal(want["points"].view(np.uint8), res["points"].view(np.uint8)) \
            and all(want["report"][f] == report[f] for f in report if not f.startswith("closure"))
        line += " | host build ms " + " ".join(f"{t:.1f}" for t in t_host) + f" (outputs equal: {equal})"
    line += f" | medians fuse_chain {ch:.3f} ms, fuse_ring {rg:.3f} ms = chain + {1e3 * (rg - ch):.0f} us ({rg / ch:.2f}x), {1e6 * rg / N:.2f} ns per node"
    if host:
        line += f"; host build {float(np.median(t_host)):.1f} ms = {float(np.median(t_host)) / rg:.0f}x"
    print(line, flush=True)
    for p in pairs:
        p.close()


def chain_bench(title, root):
    """profiles/fuse_bench.py of the tree at `root` in a child process (it imports that tree's package and library)."""
    print(f"\n## {title}", flush=True)
    r = subprocess.run([sys.executable, os.path.join("profiles", "fuse_bench.py")], cwd=root, capture_output=True, text=True, timeout=600)
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        raise SystemExit(f"fuse_bench.py failed in {root}:\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--ring-only", action="store_true", help="leave out the runs of profiles/fuse_bench.py")
    ap.add_argument("--parent", default=None, help="a directory with the parent commit's sources and build: fuse_bench.py runs there too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print("## profiles/fuse_ring_bench.py: sfm_fuse_chain and sfm_fuse_ring on the same rings, this tree", flush=True)
    print(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    for k in [int(x) for x in a.pairs.split(",") if x]:
        measure(ctx, dev, k, a.n, a.seed, a.reps, host=not a.no_host, iterations=a.iterations)
    if a.ring_only:
        return
    ctx.close()
    chain_bench("profiles/fuse_bench.py, this tree, a child process of the same run", ROOT)
    if a.parent:
        chain_bench("profiles/fuse_bench.py, the parent commit (git archive <parent commit>, make of its library and libfusecheck.so), a child process "
                    "of the same run", os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
