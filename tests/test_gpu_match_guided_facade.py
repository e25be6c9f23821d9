"""GPU: the facade of sfm_match_guided (MatchSiftDataGuided of host/cudaSift.h, SfM::Image_pair::fundamental of host/sfm.h) through
host/guided_match_demo on written feature files of the dino frames 0 and 1 -- its plain: and guided: lines are the Python calls'
counts on the same records."""
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


def counts(d, n):
    rec = d[:n].cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)
    matched = rec["match"] >= 0
    return n, int(matched.sum()), int((matched & (rec["score"] > np.float32(0.85)) & (rec["ambiguity"] < np.float32(0.95))).sum())


def test_guided_match_demo_prints_the_python_calls_counts(gpu, tmp_path):
    torch, dev, ctx = gpu
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "guided_match_demo")
    assert os.path.exists(demo), "guided_match_demo not built (make)"
    (d0, n0), (d1, n1) = [dino_extract(gpu, k) for k in (0, 1)]
    files = []
    for k, (d, n) in enumerate(((d0, n0), (d1, n1))):           # the records before any match, as an extraction leaves them
        files.append(str(tmp_path / f"f{k}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    d0 = d0.clone()
    ctx.match(d0, n0, d1, n1)
    torch.cuda.synchronize()
    plain = counts(d0, n0)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    rep = pair.refine(max_iterations=20)
    S.match_guided(ctx, d0, n0, d1, n1, pair.fundamental(refined=True), band_px=4.0)
    torch.cuda.synchronize()
    guided = counts(d0, n0)
    pair.close()
    r = subprocess.run([demo, files[0], files[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ["plain: %d records, %d matched, %d pass 0.85 / 0.95" % plain, "guided: %d records, %d matched, %d pass 0.85 / 0.95" % guided]
    got = re.findall(r"^(?:plain|guided): .*$", r.stdout, flags=re.M)
    print(f"guided_match_demo: {got}; Python: {want}; refinement used {rep['num_used']} points")
    assert got == want
    r = subprocess.run([demo, files[0]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
