"""GPU: the facade of sfm_fuse_ring (SfM::fuse_ring of host/sfm.h) through host/fuse_chain_demo on written feature files of the
dino frames 0, 1 and 2 taken as a ring of three pairs, (0, 1), (1, 2) and (2, 0): with the trailing `loop` the fuse: and seam:
lines it prints are the Python call's numbers over the corrected links of the same records, and the cloud holds one point per
track.  The seam numbers of the real frames are printed, with no bar on them."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract
from test_gpu_ring_facade import STATUS, fuse_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_chain_demo_loop_prints_the_python_calls_numbers(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "fuse_chain_demo")
    assert os.path.exists(demo), "fuse_chain_demo not built (make)"
    k = 3
    feats = [dino_extract(gpu, v) for v in range(k)]
    files = []
    for v, (d, n) in enumerate(feats):                          # the records before any match, as an extraction leaves them
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
    outs = S._ring_buffers(dev, k, made[k - 1].num_points)
    S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], made[k - 1], S.ring_params(), outs)
    corrected = [(outs[0][13 * i:13 * i + 13],) + tuple(a[1:]) for i, a in enumerate(aouts)]
    got = S.fuse_ring(made, idx, corrected)
    chain = S.fuse_chain(made, idx[:k - 1], corrected[:k - 1])
    ring_status = S._ring_results(outs, k, made[k - 1].num_points)[3]["status"]
    for p in made:
        p.close()
    rep, counts = got["report"], got["counts"]
    print(f"dino 0, 1, 2 as a ring: close_ring {STATUS[ring_status]}; fuse_ring {counts}, {rep}; fuse_chain over the same links {chain['counts']}")
    # what the report must satisfy whatever the frames give
    assert rep["seam_refined"] + rep["seam_kept"] == rep["seam_tracks"] <= rep["seam_proposals"] - rep["seam_ineligible"]
    assert counts["refined"] + counts["kept"] == counts["tracks"] == chain["counts"]["tracks"] - rep["seam_tracks"]
    if rep["status"] != S.RING_CLOSED:
        assert rep["seam_proposals"] == 0 and counts == chain["counts"]
    ply = str(tmp_path / "loop.ply")
    args = [demo, str(k)] + files + files[1:] + files[:1]
    run = subprocess.run(args + [ply, "0", "loop"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = ("seam: %s, closure s %.6g rot %.6g rad t %.6g, %d proposals, %d ineligible, %d seam tracks, %d refined, %d kept" %
            (STATUS[rep["status"]], math.exp(rep["closure_log_scale"]), rep["closure_rotation_rad"], rep["closure_t"], rep["seam_proposals"],
             rep["seam_ineligible"], rep["seam_tracks"], rep["seam_refined"], rep["seam_kept"]))
    lines = re.findall(r"^seam: .*$", run.stdout, flags=re.M)
    print(f"fuse_chain_demo loop: {lines}; Python: {want}")
    assert lines == [want]
    assert re.findall(r"^fuse: .*$", run.stdout, flags=re.M) == [fuse_line(counts)]
    assert len(re.findall(r"^ring: .*$", run.stdout, flags=re.M)) == 1
    # one point per track (every pair of a ring whose first k - 1 links are valid lies in the first segment; WritePLY leaves out the
    # points that are all zero or not a number)
    first = [t for t in range(counts["tracks"]) if got["root"][got["obs_cam"][got["track_offset"][t]] >> 1] == 0]
    cloud = [got["points"][:3, t] for t in first]
    cloud = [p for p in cloud if p.any() and not np.isnan(p).any()]
    assert f"fused cloud: {len(cloud)} points -> {ply}" in run.stdout.splitlines()
    if counts["segments"] == 1:
        assert len(first) == counts["tracks"]
    want_ply = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(cloud) +
                "".join("%.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])) for p in cloud))
    assert open(ply).read() == want_ply
    # with adjust_iterations the ring's table goes through SfM::adjust_chain as it is: the seam tracks stay out of it
    run = subprocess.run(args + [ply, "3", "loop"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and re.findall(r"^seam: .*$", run.stdout, flags=re.M) == [want], run.stdout + run.stderr
    assert len(re.findall(r"^chain adjust: .*$", run.stdout, flags=re.M)) == counts["segments"]
    # loop wants a ring as `ring` does
    r = subprocess.run([demo, "2", files[0], files[1], files[1], files[0], "x.ply", "0", "loop"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr
