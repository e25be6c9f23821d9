"""Cost of one sfm_adjust_ring call next to sfm_adjust_chain on the same table, and against the host build of the same arithmetic
(tests/hostcheck/libringadjustcheck.so) on this machine's CPU: HIP events around the enqueued calls, one process.  For every ring
of k pairs (fuse_ring_bench.py's: ring_scene.build(k, 2155, seed, pairs="all"), true links, the override path): the device's own
sfm_fuse_ring table, a warm-up, then `reps` repetitions of [sfm_adjust_ring at 0 iterations | at `iterations` | sfm_adjust_chain
at `iterations` on the same table], alternating; medians, the per-iteration time ((t_n - t_0) / iterations actually run) and,
from it, the cost per column of the folded factor next to 6i's 7.2 us.  The ctypes structs of a call are built once, outside the
events.  Behind the rings the script runs profiles/chain_adjust_bench.py -- sfm_adjust_chain on that script's own chains -- in a
child process: on this tree, and with --parent DIR on the parent commit too (a directory that holds the parent's sources and
build), so that both stand in one output from one session: sfm_adjust_chain must not move by more than the spread of the parent's
repetitions.
    python profiles/ring_adjust_bench.py [--parent DIR] > profiles/ring_adjust_bench.txt
Kernel split: rocprofv3 --kernel-trace --stats -- python profiles/ring_adjust_bench.py --pairs 630 --reps 1 --no-host --ring-only"""
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
import ring_adjust_scene as RAS  # noqa: E402
from align_bench import timed  # noqa: E402
from fuse_ring_bench import device_ring  # noqa: E402


def measure(ctx, dev, k, n, seed, reps, W, iterations, host=True):
    t0 = time.perf_counter()
    sc, ring = RS.build(k, n, seed)
    pairs, pin, lin, keep, host_ring = device_ring(ctx, dev, ring)
    built = time.perf_counter() - t0
    N = k * n
    L = S.lib()
    fouts = S._fuse_buffers(torch, dev, k, N)
    for t in fouts:
        t.zero_()
    frep = torch.zeros(C.sizeof(S.FuseRingReport), dtype=torch.uint8, device=dev)
    fo = S.FuseOut(*[t.data_ptr() for t in fouts])
    fparams = S.fuse_ring_params()
    assert L.sfm_fuse_ring(ctx._h, pin, k, lin, C.byref(fparams), C.byref(fo), frep.data_ptr()) == S.OK, L.sfm_last_error()
    torch.cuda.synchronize()
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = fouts
    table = (root, cams, off, ocam, orec, pts, flags, counts)
    handles = (C.c_void_p * k)(*[p._h.value for p in pairs])
    hp = C.cast(handles, C.POINTER(C.c_void_p))
    rin = S.AdjustRingIn(hp, *[t.data_ptr() for t in table], frep.data_ptr())
    cin = S.AdjustChainIn(hp, *[t.data_ptr() for t in table])
    routs, couts = S.adjust_ring_buffers(dev, k, N), S.adjust_chain_buffers(dev, k, N)
    ro, co = S.AdjustRingOut(*[t.data_ptr() for t in routs]), S.AdjustChainOut(*[t.data_ptr() for t in couts])
    p0, pn = S.adjust_ring_params(max_iterations=0, max_track_views=W), S.adjust_ring_params(max_iterations=iterations, max_track_views=W)
    pc = S.adjust_chain_params(max_iterations=iterations, max_track_views=W)

    def ring0():
        assert L.sfm_adjust_ring(ctx._h, C.byref(rin), k, C.byref(p0), C.byref(ro)) == S.OK, L.sfm_last_error()

    def ringn():
        assert L.sfm_adjust_ring(ctx._h, C.byref(rin), k, C.byref(pn), C.byref(ro)) == S.OK, L.sfm_last_error()

    def chain():
        assert L.sfm_adjust_chain(ctx._h, C.byref(cin), k, C.byref(pc), C.byref(co)) == S.OK, L.sfm_last_error()

    ring0(); ringn(); chain()
    torch.cuda.synchronize()
    first = [t.clone() for t in routs]
    t_0, t_n, t_c = [], [], []
    for _ in range(reps):
        t_0.append(timed(ring0)); t_n.append(timed(ringn)); t_c.append(timed(chain))
    ringn()
    torch.cuda.synchronize()
    same = all(bool((x == y).all()) for x, y in zip(first, routs))
    T = int(counts[0].item())
    got = S.adjust_ring_results(routs, k, N, T)
    crep = S.adjust_chain_results(couts, k, N, T)["reports"][0]
    rep = got["report"]
    m0, mn, mc = float(np.median(t_0)), float(np.median(t_n)), float(np.median(t_c))
    it = max(int(rep["iterations"]), 1)
    per_it = (mn - m0) / it
    cols = 6 * (k - 1)
    line = (f"ring: k={k} N={N} n={n} W={W} (scene built in {built:.1f} s) T={T} report {rep} second call equal: {same} | adjust_chain on the same table: "
            f"{crep} | adjust_ring 0 it ms " + " ".join(f"{t:.3f}" for t in t_0) + f" | {iterations} it ms " + " ".join(f"{t:.3f}" for t in t_n) +
            " | adjust_chain ms " + " ".join(f"{t:.3f}" for t in t_c))
    if host:
        HL = RAS.host_lib()
        arrays = [t.cpu().numpy().copy() for t in table] + [frep.cpu().numpy().copy()]
        t0 = time.perf_counter()
        want = RAS.run_host(HL, S, host_ring, arrays, max_iterations=iterations, max_track_views=W)
        t_host = 1e3 * (time.perf_counter() - t0)
        equal = want["report"].tobytes() == rep.tobytes() and all(np.array_equal(want[q].view(np.uint8), got[q].view(np.uint8)) for q in ("cams", "points", "used", "err"))
        line += f" | host build {t_host:.1f} ms (outputs equal: {equal}, band claim held: {want['band']})"
    line += (f" | medians: adjust_ring {m0:.3f} ms at 0 iterations, {mn:.3f} ms at {iterations} ({rep['iterations']} run): {per_it:.3f} ms per iteration = "
             f"{1e3 * per_it / cols:.2f} us per column of {cols} (whole iteration; 6i: 7.2 us per column of the factor alone); adjust_chain {mc:.3f} ms "
             f"({crep['iterations']} run)")
    print(line, flush=True)
    for p in pairs:
        p.close()


def chain_bench(title, root):
    """profiles/chain_adjust_bench.py of the tree at `root` in a child process (it imports that tree's package and library)."""
    print(f"\n## {title}", flush=True)
    r = subprocess.run([sys.executable, os.path.join("profiles", "chain_adjust_bench.py")], cwd=root, capture_output=True, text=True, timeout=900)
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        raise SystemExit(f"chain_adjust_bench.py failed in {root}:\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="36,256,630")
    ap.add_argument("--n", type=int, default=2155)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views", type=int, default=8, help="max_track_views")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--ring-only", action="store_true", help="leave out the runs of profiles/chain_adjust_bench.py")
    ap.add_argument("--parent", default=None, help="a directory with the parent commit's sources and build: chain_adjust_bench.py runs there too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print("## profiles/ring_adjust_bench.py: sfm_adjust_ring and sfm_adjust_chain on the same ring tables, this tree", flush=True)
    print(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units", flush=True)
    for k in [int(x) for x in a.pairs.split(",") if x]:
        measure(ctx, dev, k, a.n, a.seed, a.reps, a.views, a.iterations, host=not a.no_host)
    if a.ring_only:
        return
    ctx.close()
    chain_bench("profiles/chain_adjust_bench.py, this tree, a child process of the same run", ROOT)
    if a.parent:
        chain_bench("profiles/chain_adjust_bench.py, the parent commit (git archive <parent commit>, make of its library and libchainadjustcheck.so), a "
                    "child process of the same run", os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
