"""GPU: the facade of sfm_triangulate_views (SfM::triangulate_views of host/sfm.h) through host/register_views_demo on written
feature files of the dino frames 0, 1, 2 -- the counts it prints are the Python call's on the same records; and host/sfm_main
with a third image: the merged cloud it reports is what the PLY holds."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV
from view_points_scene import dino_extract

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_views_demo_prints_the_python_calls_counts(gpu, tmp_path):
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
    (_, flags, _, counts), = S.triangulate_views([pair], [d0])
    pair.close()
    r = subprocess.run([demo, "20", *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^view3 points: (\d+) new, (\d+) refined, (\d+) kept, (\d+) rejected$", r.stdout, flags=re.M)
    assert m, r.stdout
    got = tuple(int(x) for x in m.groups())
    want = (int(counts[S.VP_NEW]), int(counts[S.VP_REFINED]), int(counts[S.VP_KEPT]), int(counts[S.VP_NEW_REJECTED]))
    print(f"register_views_demo: {m.group(0)}; Python: {want}")
    assert got == want and want[0] + want[1] > 0
    assert np.array_equal(np.bincount(flags, minlength=5), counts[:5])


def test_sfm_main_writes_the_merged_cloud(tmp_path):
    app = os.path.join(ROOT, "cuda-sfm_amd", "host", "sfm_main")
    assert os.path.exists(app), "sfm_main not built (make)"
    frames = [os.path.join(ROOT, "tests", "golden", "dino", f"dino_grey_00{k}.pgm") for k in (0, 1, 2)]
    ply = str(tmp_path / "cloud.ply")
    r = subprocess.run([app, frames[0], frames[1], ply, "", "0", "0", "1.0", "1.5", "2360", "20", frames[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    first = int(re.search(r"^sfm_main: .* (\d+) points -> ", r.stdout, flags=re.M).group(1))
    new, refined, kept, rejected = (int(x) for x in re.search(r"^view3 points: (\d+) new, (\d+) refined, (\d+) kept, (\d+) rejected$", r.stdout,
                                                              flags=re.M).groups())
    merged = int(re.search(r"^merged cloud: (\d+) points -> ", r.stdout, flags=re.M).group(1))
    vertices = int(re.search(rb"element vertex (\d+)", open(ply, "rb").read(4096)).group(1))
    print(f"two-view cloud {first} points, view3 points {new} / {refined} / {kept} / {rejected}, merged {merged}, PLY {vertices}")
    assert merged == vertices == first + new and refined + kept <= first        # refined and kept points were used points already
