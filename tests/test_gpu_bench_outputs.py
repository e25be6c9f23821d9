"""bench.py as a plain run (one timed region, the line) with --dump-outputs: the files hold what a caller of the timed path receives
for the step the line names -- the same winner, E bit for bit and inlier mask as one estimateE with that step's seed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_step(gpu, tmp_path):
    torch, dev, ctx = gpu
    import cuda_sfm_amd as S
    from cuda_sfm_amd import synth
    n, H = 4096, 65536
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--hyps", str(H),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert not any(k in rec for k in ("cpu_baseline", "variants", "extra")), "a plain run measures the headline only (--full adds the rest)"

    E, mask, best = (np.load(out / f"{name}.npy") for name in ("E", "inlier_mask", "best"))
    assert E.dtype == np.float32 and E.shape == (3, 3)
    assert mask.dtype == np.float32 and mask.shape == (n,)
    assert best.dtype == np.float64 and best.shape == (2,)
    res = rec["result"]
    assert [int(best[0]), int(best[1])] == [res["best_hypothesis"], res["inliers"]] and int(mask.sum()) == res["mask_sum"]

    scene = synth.two_view_scene(n)                       # the bench's inputs, again: the step the line names, one estimateE
    pair = S.ImagePair(ctx, scene["K"], scene["Kinv"], 2, n)
    pair.fillXU(torch.from_numpy(scene["sift"].view(np.uint8).reshape(n, 576)).to(dev))
    pair.estimateE(S.default_params(n, num_hypotheses=H, seed=res["sampler_seed_of_this_result"]))
    assert list(pair.get_best()) == [int(best[0]), int(best[1])]
    assert np.array_equal(pair.get_E().view(np.uint32), E.view(np.uint32))
    assert np.array_equal(pair.get_inlier_mask().astype(np.float32), mask)
    pair.close()
