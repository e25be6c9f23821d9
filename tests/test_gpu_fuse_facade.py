"""GPU: the facade of sfm_fuse_chain (SfM::fuse_chain of host/sfm.h) through host/fuse_chain_demo on written feature files of
the dino frames 0 .. 3 -- the fuse: line it prints is the Python call's counts on the same records, and the fused cloud holds one
point per track of the first segment."""
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_chain_demo_prints_the_python_calls_counts(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "fuse_chain_demo")
    assert os.path.exists(demo), "fuse_chain_demo not built (make)"
    feats = [dino_extract(gpu, k) for k in range(4)]
    files = []
    for k, (d, n) in enumerate(feats):                          # the records before any match, as an extraction leaves them
        files.append(str(tmp_path / f"f{k}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    made, idx = [], []
    for (da, na), (db, nb) in zip(feats[:-1], feats[1:]):
        ctx.match(da, na, db, nb)
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, na)
        pair.fillXU(da)
        pair.estimateE(S.default_params(na))
        made.append(pair)
    S.refine_pairs(made, max_iterations=20)
    for (da, na) in feats[:-2]:
        d_index = torch.empty(na, dtype=torch.int32, device=dev)
        S.align_index_from_matches(ctx, da, na, d_index)
        idx.append(d_index)
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, params.num_hypotheses) for p in made[:-1]]
    S.align_pairs_enqueue(made[:-1], made[1:], idx, params, aouts)
    got = S.fuse_chain(made, idx, aouts)
    c = got["counts"]
    first = sum(1 for t in range(c["tracks"]) if got["root"][got["obs_cam"][got["track_offset"][t]] >> 1] == 0)
    for p in made:
        p.close()
    ply = str(tmp_path / "fused.ply")
    r = subprocess.run([demo, "3", files[0], files[1], files[2], files[1], files[2], files[3], ply], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ("fuse: %d tracks, %d observations, %d refined, %d kept, %d segments, longest track %d views" %
            (c["tracks"], c["observations"], c["refined"], c["kept"], c["segments"], c["longest_track"]))
    lines = re.findall(r"^fuse: .*$", r.stdout, flags=re.M)
    print(f"fuse_chain_demo: {lines}; Python: {want}")
    assert lines == [want]
    assert f"fused cloud: {first} points -> {ply}" in r.stdout.splitlines()
    head = open(ply).read(200)
    assert head.startswith("ply") and f"element vertex {first}" in head
    # a_2 must hold the records of b_1's view
    r = subprocess.run([demo, "2", files[0], files[2], files[1], files[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "not the records of one view" in r.stderr
