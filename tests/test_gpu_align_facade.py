"""GPU: the facade of sfm_align_pairs (SfM::align_pairs of host/sfm.h) through host/align_pairs_demo on written feature files of
the dino frames 0, 1, 2 -- the align: line it prints is the Python call's report on the same records, the chained cloud holds
both pairs' used points, and feature files that are not one view's records are refused."""
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_pairs_demo_prints_the_python_calls_link(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "align_pairs_demo")
    assert os.path.exists(demo), "align_pairs_demo not built (make)"
    feats = [dino_extract(gpu, k) for k in (0, 1, 2)]
    files = []
    for k, (d, n) in enumerate(feats):                          # the records before any match, as an extraction leaves them
        files.append(str(tmp_path / f"f{k}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    (d0, n0), (d1, n1), (d2, n2) = feats
    ctx.match(d0, n0, d1, n1)
    ctx.match(d1, n1, d2, n2)
    pa, pb = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0), S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n1)
    pa.fillXU(d0); pb.fillXU(d1)
    pa.estimateE(S.default_params(n0)); pb.estimateE(S.default_params(n1))
    S.refine_pairs([pa, pb], max_iterations=20)
    d_index = torch.empty(n0, dtype=torch.int32, device=dev)
    S.align_index_from_matches(ctx, d0, n0, d_index)
    (sim, _, _, _, rep), = S.align_pairs([pa], [pb], [d_index])
    used = int(pa.get_reprojection_errors()[1].sum()) + int(pb.get_reprojection_errors()[1].sum())
    pa.close(); pb.close()
    ply = str(tmp_path / "cloud.ply")
    r = subprocess.run([demo, "2", files[0], files[1], files[1], files[2], ply], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ("align: %d candidates, %d inliers, s %.5f, rms %.4f -> %.4f px, %d iterations" %
            (rep["num_candidates"], rep["num_inliers"], sim[0], rep["initial_rms_px"], rep["final_rms_px"], rep["iterations"]))
    got = re.findall(r"^align: .*$", r.stdout, flags=re.M)
    print(f"align_pairs_demo: {got}; Python: {want}")
    assert got == [want]
    assert f"chained cloud: {used} points -> {ply}" in r.stdout.splitlines()
    head = open(ply).read(200)
    assert head.startswith("ply") and f"element vertex {used}" in head
    # a_2 must hold the records of b_1's view
    r = subprocess.run([demo, "2", files[0], files[2], files[1], files[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "not the records of one view" in r.stderr
