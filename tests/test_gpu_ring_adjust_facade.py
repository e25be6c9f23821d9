"""GPU: the facade of sfm_adjust_ring (SfM::adjust_ring of host/sfm.h) through host/fuse_chain_demo on written feature files of
the dino frames 0, 1 and 2 taken as a ring of three pairs, (0, 1), (1, 2) and (2, 0): with `loop` and adjust_iterations > 0 the
`ring adjust:` line it prints is the Python call's report over the corrected links of the same records, where the ring closed;
where it did not, no such line is printed.  The numbers of the real frames are printed, with no bar on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract
from test_gpu_ring_facade import STATUS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_chain_demo_loop_prints_the_python_calls_ring_adjust_line(gpu, tmp_path):
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
    routs = S._ring_buffers(dev, k, made[k - 1].num_points)
    S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], made[k - 1], S.ring_params(), routs)
    N = sum(p.num_points for p in made)
    fouts = S._fuse_buffers(torch, dev, k, N)
    frep = torch.zeros(C.sizeof(S.FuseRingReport), dtype=torch.uint8, device=dev)
    S.fuse_ring_enqueue(ctx, made, [(idx[i], routs[0][13 * i:13 * i + 13], a[1], a[2], a[4]) for i, a in enumerate(aouts)], S.fuse_ring_params(), fouts, frep)
    got = S.adjust_ring(made, fouts, frep, max_iterations=iters)
    rep = got["report"]
    for p in made:
        p.close()
    print(f"dino 0, 1, 2 as a ring: fuse_ring {STATUS[rep['ring_status']]}; adjust_ring {rep}")
    ply = str(tmp_path / "loop.ply")
    args = [demo, str(k)] + files + files[1:] + files[:1]
    run = subprocess.run(args + [ply, str(iters), "loop"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = re.findall(r"^ring adjust: .*$", run.stdout, flags=re.M)
    if rep["ring_status"] == S.RING_CLOSED:
        want = ("ring adjust: %d cameras, %d tracks, %d seam tracks, rms %.6g -> %.6g px, %d iterations" %
                (rep["num_cameras"], rep["num_tracks"], rep["num_seam_tracks"], rep["initial_rms_px"], rep["final_rms_px"], rep["iterations"]))
        print(f"fuse_chain_demo loop {iters}: {lines}; Python: {want}")
        assert lines == [want] and rep["num_cameras"] == k - 1
    else:
        assert lines == [] and all(rep[f] == 0 for f in rep.dtype.names if f != "ring_status")
    # `loop 0`, `ring` and the plain form print no such line
    for tail in (["0", "loop"], [str(iters), "ring"], [str(iters)]):
        r = subprocess.run(args + [ply] + tail, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ring adjust:" not in r.stdout, tail
