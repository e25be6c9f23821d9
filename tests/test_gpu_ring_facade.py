"""GPU: the facade of sfm_close_ring (SfM::close_ring of host/sfm.h) through host/fuse_chain_demo on written feature files of the
dino frames 0, 1 and 2 taken as a ring of three pairs, (0, 1), (1, 2) and (2, 0) -- the ring: line it prints is the Python call's
report on the same records, its fuse: line the Python fusion over the corrected links, and without the trailing `ring` the demo
prints what the Python chain over the measured links gives."""
import math
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
STATUS = ("closed", "open", "rejected")


def fuse_line(c):
    return ("fuse: %d tracks, %d observations, %d refined, %d kept, %d segments, longest track %d views" %
            (c["tracks"], c["observations"], c["refined"], c["kept"], c["segments"], c["longest_track"]))


def test_fuse_chain_demo_prints_the_python_calls_ring_report(gpu, tmp_path):
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
        # every pair matches its own copy of the first view's records: view 0 is pair 0's first view and, through pair 2, a second one
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
    ctx.synchronize()
    rep = S._ring_results(outs, k, made[k - 1].num_points)[3]
    chain = S.fuse_chain(made, idx[:k - 1], aouts[:k - 1])
    measured = chain["counts"]
    corrected = S.fuse_chain(made, idx[:k - 1], [(outs[0][13 * i:13 * i + 13],) + tuple(a[1:]) for i, a in enumerate(aouts[:k - 1])])["counts"]
    for p in made:
        p.close()
    args = [demo, str(k)] + files + files[1:] + files[:1]
    with_ring = subprocess.run(args + [str(tmp_path / "ring.ply"), "0", "ring"], capture_output=True, text=True, timeout=300)
    plain = subprocess.run(args + [str(tmp_path / "plain.ply")], capture_output=True, text=True, timeout=300)
    assert with_ring.returncode == 0 and plain.returncode == 0, with_ring.stdout + with_ring.stderr + plain.stdout + plain.stderr
    want = ("ring: %s, drift s %.6g rot %.6g rad, seam rms %.6g -> %.6g px (link %.6g), %d records" %
            (STATUS[rep["status"]], math.exp(rep["drift_log_scale"]), rep["drift_rotation_rad"], rep["seam_rms_open_px"], rep["seam_rms_closed_px"],
             rep["seam_rms_link_px"], rep["seam_count"]))
    lines = re.findall(r"^ring: .*$", with_ring.stdout, flags=re.M)
    print(f"fuse_chain_demo: {lines}; Python: {want}; report {rep}")
    assert lines == [want]
    assert re.findall(r"^fuse: .*$", with_ring.stdout, flags=re.M) == [fuse_line(corrected)]
    # without the argument the whole output is what the demo printed before it had one: k timer lines of the facade's matcher, the
    # fuse: line of the chain over the measured links, the cloud's line -- and the cloud itself, WritePLY's bytes of the Python
    # chain's first segment
    first = [t for t in range(measured["tracks"]) if chain["root"][chain["obs_cam"][chain["track_offset"][t]] >> 1] == 0]
    cloud = [chain["points"][:3, t] for t in first]
    cloud = [p for p in cloud if p.any() and not np.isnan(p).any()]
    ply = str(tmp_path / "plain.ply")
    lines = plain.stdout.splitlines()
    assert [l for l in lines if " time = " not in l] == [fuse_line(measured), f"fused cloud: {len(cloud)} points -> {ply}"]
    timers = [l for l in lines if " time = " in l]
    assert len(timers) == k and all(re.fullmatch(r"MatchSiftData time = +[0-9.]+ ms", l) for l in timers) and lines[:k] == timers
    want_ply = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(cloud) +
                "".join("%.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])) for p in cloud))
    assert open(ply).read() == want_ply
    # the argument wants a ring: b_k must hold the records of a_1's view, and k >= 3
    r = subprocess.run([demo, str(k)] + files + files[1:] + files[1:2] + ["x.ply", "0", "ring"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "not the records of one view" in r.stderr
    r = subprocess.run([demo, "2", files[0], files[1], files[1], files[0], "x.ply", "0", "ring"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage:" in r.stderr
