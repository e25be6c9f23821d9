"""Cost of one sfm_close_ring call against sfm_fuse_chain on the same chain and against the host build of the same arithmetic
(tests/hostcheck/libringcheck.so) on this machine's CPU: HIP events around the enqueued calls, one process, a warm-up of both
calls, then three repetitions of each, alternating; medians.  The ctypes arrays of a call are built once, outside the events.
Rings: tests/ring_scene.py, k views on a circle, every link composed with a small similarity (2e-4 rad, 0.1 % in s and t), on the
override path (pairs that only have fillXU; points, flags, poses and links uploaded).  Up to --fuse-up-to links every pair of the
ring exists with --n records and sfm_fuse_chain runs over the first k - 1 links; beyond that only pair k - 1 exists.  A second row
per ring has a last pair of --seam records: what the seam kernel costs.  With --dino the ring of the 36 committed dino frames
through fillXU, estimateE, ONE sfm_refine_pairs and ONE sfm_align_pairs over its 36 links.
    python profiles/close_ring_bench.py [--dino] [--out profiles/close_ring_bench.txt]
Kernel split, two steps: rocprofv3 --kernel-trace --stats -d DIR -o ring -- python profiles/close_ring_bench.py --links 4096
--ring-only --reps 1 --out /dev/null, then python profiles/close_ring_bench.py --split-db DIR/.../ring_results.db, which needs no
GPU and writes the ring kernels' average durations to profiles/close_ring_split.txt (--split-out)."""
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
import fuse_scene as FS  # noqa: E402
import ring_scene as RS  # noqa: E402
from align_bench import dev_records, timed  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def report_rows(dev, status, inliers):
    size = C.sizeof(S.AlignReport)
    rows = np.zeros((len(status), size), np.uint8)
    for i in range(len(status)):
        r = S.AlignReport(); r.status = int(status[i]); r.num_inliers = int(inliers[i])
        rows[i] = np.frombuffer(bytes(r), np.uint8)
    return up(dev, rows.ravel()), size


def ring_call(ctx, dev, sc, inp):
    """(call, pair, outs, host input): one sfm_close_ring over the uploaded links and last pair, its ctypes arrays built once."""
    k, L = inp["k"], inp["last"]
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, L["n"])
    pair.fillXU(dev_records(dev, L["sift"]))
    keep = [up(dev, L["points"]), up(dev, L["valid"]), up(dev, inp["sims"].ravel())]
    reports, size = report_rows(dev, inp["status"], inp["inliers"])
    lin = (S.RingLinkIn * k)(*[S.RingLinkIn(keep[2].data_ptr() + 52 * i, reports.data_ptr() + size * i) for i in range(k)])
    pin = S.FusePairIn(pair._h.value, keep[0].data_ptr(), keep[1].data_ptr(), None)
    outs = S._ring_buffers(dev, k, L["n"])
    o = S.RingOut(*[t.data_ptr() for t in outs])
    params = S.ring_params()
    lib = S.lib()

    def call():
        assert lib.sfm_close_ring(ctx._h, lin, k, C.byref(pin), C.byref(params), C.byref(o)) == S.OK, lib.sfm_last_error()
    call.keep = (keep, reports, lin, pin, o, params)
    return call, pair, outs, dict(inp, last=dict(L, X1=pair.get_XU(S.BUF_X1), ld=L["n"]))


def fuse_call(ctx, dev, sc, sims):
    """One sfm_fuse_chain over the ring's k pairs and its first k - 1 links on the override path."""
    k = sc["k"]
    pairs, keep = [], []
    for v in range(k):
        P = sc["pairs"][v]
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, P["n"])
        pair.fillXU(dev_records(dev, P["sift"]))
        pairs.append(pair)
        keep.append((up(dev, P["points"]), up(dev, P["valid"]), up(dev, P["pose"])))
    d_sims = up(dev, np.ascontiguousarray(sims, np.float32).ravel())
    reports, size = report_rows(dev, np.zeros(k, np.int32), sc["inliers"])
    link = [(up(dev, sc["index"][v]), up(dev, sc["pairs"][v]["good"].astype(np.uint8)), up(dev, np.full(sc["n"], FS.ERR, np.float32))) for v in range(k - 1)]
    N = sum(p.num_points for p in pairs)
    pin = (S.FusePairIn * k)(*[S.FusePairIn(p._h.value, a.data_ptr(), b.data_ptr(), c.data_ptr()) for p, (a, b, c) in zip(pairs, keep)])
    lin = (S.FuseLinkIn * (k - 1))(*[S.FuseLinkIn(i.data_ptr(), d_sims.data_ptr() + 52 * v, m.data_ptr(), e.data_ptr(), reports.data_ptr() + size * v)
                                     for v, (i, m, e) in enumerate(link)])
    outs = S._fuse_buffers(torch, dev, k, N)
    fo = S.FuseOut(*[t.data_ptr() for t in outs])
    params = S.fuse_params()
    lib = S.lib()

    def call():
        assert lib.sfm_fuse_chain(ctx._h, pin, k, lin, C.byref(params), C.byref(fo)) == S.OK, lib.sfm_last_error()
    call.keep = (keep, d_sims, reports, link, pin, lin, fo, params, outs)
    return call, pairs, N


def measure(ctx, dev, k, n, seam, reps, fuse_up_to, ring_only):
    sc = RS.build(k, n, 31, pairs="all" if k <= fuse_up_to and not ring_only else "last")
    deltas = RS.small_similarities(k, 32, rot=2e-4, scale=1e-3, trans=1e-3)
    sims = RS.perturbed(sc["sims"], deltas)
    rows = [("last pair %d records" % n, sc, RS.ring_input(sc, sims=sims))]
    if seam != n and not ring_only:
        big = RS.build(k, seam, 31)                       # a ring of its own (the views' places follow the point count): its own links
        rows.append(("last pair %d records" % seam, big, RS.ring_input(big, sims=RS.perturbed(big["sims"], deltas))))
    fuse, fpairs = None, []
    if k <= fuse_up_to and not ring_only:
        fuse, fpairs, N = fuse_call(ctx, dev, sc, sims)
        fuse()
    HL = RS.host_lib()
    for what, scene, inp in rows:
        call, pair, outs, host_in = ring_call(ctx, dev, scene, inp)
        call()
        torch.cuda.synchronize()
        first = [t.clone() for t in outs]
        t_ring, t_fuse = [], []
        for _ in range(reps):
            t_ring.append(timed(call))
            if fuse is not None:
                t_fuse.append(timed(fuse))
        got = S._ring_results(outs, k, inp["last"]["n"])
        same = all(bool((x.view(torch.uint8) == y.view(torch.uint8)).all()) for x, y in zip(first, outs))
        line = f"synthetic ring k={k}, {what}: status {got[3]['status']} seam {got[3]['seam_count']} second call equal: {same} | close_ring ms " + " ".join(f"{t:.3f}" for t in t_ring)
        med = float(np.median(t_ring))
        if ring_only:
            say(line + f" | median {med:.3f} ms")
            pair.close()
            continue
        t_host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            want = RS.run_host(HL, S, host_in)
            t_host.append(1e3 * (time.perf_counter() - t0))
        equal = want[3] == got[3] and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want[:3], got[:3]))
        line += " | host build ms " + " ".join(f"{t:.2f}" for t in t_host) + f" (outputs equal: {equal})"
        line += f" | medians close_ring {med:.3f} ms = {1e3 * med / k:.2f} us per link; host build {float(np.median(t_host)):.2f} ms = {float(np.median(t_host)) / med:.1f}x"
        if t_fuse:
            fu = float(np.median(t_fuse))
            line += f"; fuse_chain on the same chain ({N} nodes) {fu:.3f} ms, close_ring = {med / fu:.2f}x of it"
        say(line)
        pair.close()
    for p in fpairs:
        p.close()


def dino(ctx, dev, reps):
    from align_bench import dino_links
    links, pairs = dino_links(ctx, dev)
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, a.num_points, params.num_hypotheses) for a, _, _, _ in links]
    S.align_pairs_enqueue([l[0] for l in links], [l[1] for l in links], [l[2] for l in links], params, aouts)
    k = len(links)
    outs = S._ring_buffers(dev, k, pairs[k - 1].num_points)
    call = lambda: S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], pairs[k - 1], S.ring_params(), outs)
    call()
    t = [timed(call) for _ in range(reps)]
    got = S._ring_results(outs, k, pairs[k - 1].num_points)
    status = [S.AlignReport.from_buffer_copy(a[4].cpu().numpy().tobytes()).status for a in aouts]
    bad = [i for i, s in enumerate(status) if s == S.REFINE_DEGENERATE]
    say(f"dino ring: k={k} report {got[3]} | degenerate links {len(bad)}: {bad} | close_ring ms " + " ".join(f"{x:.3f}" for x in t) + " (with the Python wrapper's arrays inside the events)")
    for p in pairs:
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", default="36,630,4096")
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--seam", type=int, default=2155)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fuse-up-to", type=int, default=630)
    ap.add_argument("--dino", action="store_true")
    ap.add_argument("--ring-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "close_ring_bench.txt"))
    ap.add_argument("--split-db", help="rocprofv3's database of a --ring-only run: write the kernel split and stop")
    ap.add_argument("--split-out", default=os.path.join(ROOT, "profiles", "close_ring_split.txt"))
    a = ap.parse_args()
    if a.split_db:
        import sqlite3
        rows = list(sqlite3.connect(a.split_db).execute("select name, count(*), avg(end - start) from kernels where name like 'sfm::ring%' group by name order by name"))
        with open(a.split_out, "w") as f:
            f.write(f"# kernel split of sfm_close_ring, rocprofv3 --kernel-trace --stats, a run of its own ({os.path.basename(a.split_db)}); average per launch\n")
            for name, calls, avg in rows:
                f.write(f"{name.split('(')[0]}: {avg / 1e3:.1f} us over {calls} launches\n")
        return
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    say(f"# {torch.cuda.get_device_properties(0).multi_processor_count} compute units")
    for k in [int(x) for x in a.links.split(",") if x]:
        measure(ctx, dev, k, a.n, a.seam, a.reps, a.fuse_up_to, a.ring_only)
    if a.dino:
        dino(ctx, dev, a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
