"""GPU: the facade of sfm_intersect_tracks (SfM::intersect_tracks of host/sfm.h) through host/fuse_chain_demo on written feature
files of the dino frames 0, 1 and 2.  Behind an adjustment (`<iterations> > 0`, plain or `loop`) the demo re-intersects the tracks
the last adjustment did not use under its cameras and prints one `intersect:` line (on stderr) with the call's eight counts: they
are the Python call's on the same records.  The forms without an adjustment print no such line.  The numbers of the real frames
are printed, with no bar on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "intersect: %d tracks, %d intersected, %d refined, %d kept, %d copied, %d from the linear start, %d without a start, %d promoted"


def python_counts(gpu, made, fouts, frep, iters, loop):
    """adjust_chain, then (loop, a ring that closed) adjust_ring, then intersect_tracks under the last adjustment's cameras and points
    with its used flags as d_skip: the counts in d_counts' order."""
    torch, dev, ctx = gpu
    k, N = len(made), sum(p.num_points for p in made)
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = fouts
    adj = S.adjust_chain_buffers(dev, k, N)
    S.adjust_chain_enqueue(ctx, made, (root, cams, off, ocam, orec, pts, flags, counts), S.adjust_chain_params(max_iterations=iters), adj)
    ctx.synchronize()
    if loop and S.FuseRingReport.from_buffer_copy(frep.cpu().numpy().tobytes()).status == S.RING_CLOSED:
        adj = S.adjust_ring_buffers(dev, k, N)
        S.adjust_ring_enqueue(ctx, made, (root, cams, off, ocam, orec, pts, flags, counts, frep), S.adjust_ring_params(max_iterations=iters), adj)
        ctx.synchronize()
    got = S.intersect_tracks(made, fouts[:7] + (adj[1],) + fouts[8:], cams=adj[0], skip=adj[2])
    return tuple(got["counts"][c] for c in S.INTERSECT_COUNTS)


def test_fuse_chain_demo_prints_the_python_calls_intersect_line(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "fuse_chain_demo")
    assert os.path.exists(demo), "fuse_chain_demo not built (make)"
    k, iters = 3, 3
    feats = [dino_extract(gpu, v) for v in range(k)]
    files = []
    for v, (d, n) in enumerate(feats):
        files.append(str(tmp_path / f"f{v}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    made, idx = [], []
    for v in range(k):
        (da, na), (db, nb) = feats[v], feats[(v + 1) % k]
        da = da.clone()
        ctx.match(da, na, db, nb)
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, na)
        pair.fillXU(da)
        pair.estimateE(S.default_params(na))
        made.append(pair)
        d_index = torch.empty(na, dtype=torch.int32, device=dev)
        S.align_index_from_matches(ctx, da, na, d_index)
        idx.append(d_index)
    S.refine_pairs(made, max_iterations=20)
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, params.num_hypotheses) for p in made]
    S.align_pairs_enqueue(made, made[1:] + made[:1], idx, params, aouts)
    N = sum(p.num_points for p in made)
    # `loop`: the ring closed and fused over all k corrected links
    routs = S._ring_buffers(dev, k, made[k - 1].num_points)
    S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], made[k - 1], S.ring_params(), routs)
    fouts = S._fuse_buffers(torch, dev, k, N)
    frep = torch.zeros(C.sizeof(S.FuseRingReport), dtype=torch.uint8, device=dev)
    S.fuse_ring_enqueue(ctx, made, [(idx[i], routs[0][13 * i:13 * i + 13], a[1], a[2], a[4]) for i, a in enumerate(aouts)], S.fuse_ring_params(), fouts, frep)
    ctx.synchronize()
    want_loop = LINE % python_counts(gpu, made, fouts, frep, iters, True)
    # the plain form: the chain fused over the first k - 1 measured links
    couts = S._fuse_buffers(torch, dev, k, N)
    S.fuse_chain_enqueue(ctx, made, [(idx[i], a[0], a[1], a[2], a[4]) for i, a in enumerate(aouts[:k - 1])], S.fuse_params(), couts)
    ctx.synchronize()
    want_plain = LINE % python_counts(gpu, made, couts, None, iters, False)
    for p in made:
        p.close()
    ply = str(tmp_path / "cloud.ply")
    args = [demo, str(k)] + files + files[1:] + files[:1]
    for tail, want in (([str(iters), "loop"], want_loop), ([str(iters)], want_plain)):
        run = subprocess.run(args + [ply] + tail, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = re.findall(r"^intersect: .*$", run.stderr, flags=re.M)
        print(f"fuse_chain_demo {' '.join(tail)}: {lines}; Python: {want}")
        assert lines == [want] and "intersect:" not in run.stdout
    # the forms without an adjustment print no such line
    for tail in (["0", "loop"], ["0", "ring"], ["0"], []):
        r = subprocess.run(args + [ply] + tail, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "intersect:" not in r.stdout + r.stderr, tail
