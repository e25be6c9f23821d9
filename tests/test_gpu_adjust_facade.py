"""GPU: the facade of sfm_adjust_views (SfM::adjust_views of host/sfm.h) through host/register_views_demo on written feature
files of the dino frames 0, 1, 2 -- the adjust: line it prints is the Python call's report on the same records, and the line
behind it the Python call's second triangulation with the adjusted cameras."""
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV, to_dev
from view_points_scene import dino_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_views_demo_prints_the_python_calls_adjustment(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "register_views_demo")
    assert os.path.exists(demo), "register_views_demo not built (make)"
    feats = [dino_extract(gpu, k) for k in (0, 1, 2)]
    files = []
    for k, (d, n) in enumerate(feats):                          # the records before any match, as an extraction leaves them
        files.append(str(tmp_path / f"f{k}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    (d0, n0), (d1, n1), (d2, n2) = feats
    ctx.match(d0, n0, d1, n1)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    S.refine_pairs([pair], max_iterations=20)
    ctx.match(d0, n0, d2, n2)
    S.register_views([pair], [d0])
    (points, flags, _, _), = S.triangulate_views([pair], [d0])
    (poses, _, _, _, rep), = S.adjust_views([pair], [(d0, to_dev(torch, dev, points), to_dev(torch, dev, flags))])
    _, _, _, counts = pair.triangulate_view(d0, poses=to_dev(torch, dev, poses))
    pair.close()
    r = subprocess.run([demo, "20", *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ("adjust: %d points (%d / %d in views 2 / 3), rms %.4f -> %.4f px, %d iterations" %
            (rep["num_points"], rep["num_view2"], rep["num_view3"], rep["initial_rms_px"], rep["final_rms_px"], rep["iterations"]))
    got = re.findall(r"^adjust: .*$", r.stdout, flags=re.M)
    print(f"register_views_demo: {got}; Python: {want}")
    assert got == [want] and rep["num_view3"] >= 6 and rep["status"] != S.REFINE_DEGENERATE
    lines = r.stdout.splitlines()
    k = lines.index(want)
    assert lines[k - 1].startswith("view3 points: ")
    assert lines[k + 1] == "adjusted view3 points: %d new, %d refined, %d kept, %d rejected" % (
        counts[S.VP_NEW], counts[S.VP_REFINED], counts[S.VP_KEPT], counts[S.VP_NEW_REJECTED])
