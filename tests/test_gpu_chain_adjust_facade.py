"""GPU: sfm_adjust_chain behind the whole device chain (fillXU -> estimateE -> sfm_refine_pairs -> sfm_align_pairs ->
sfm_fuse_chain -> sfm_adjust_chain, no overrides) on the synthetic five views and on the dino frames 0 .. 3, against the host build
and the fp64 twin on the read-back state; and the facade (SfM::adjust_chain of host/sfm.h) through host/fuse_chain_demo."""
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV, to_dev
import chain_adjust_reference as CR
import chain_adjust_scene as CS
import fuse_scene as FS
from view_points_scene import dino_extract
from test_gpu_align import chain as refined_chain, read_buffers
from test_gpu_fuse import aligned, read_back_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_ROT, BAR_T, BAR_RMS = 1e-4, 1e-3, 1e-4                                     # the host-build bars of tests/test_chain_adjust_host.py


def fuse_on_device(gpu, made, idx, aouts):
    """sfm_fuse_chain with its outputs left on the device: (tensors in the order of sfm_fuse_out, the dict fuse_chain returns)."""
    torch, dev, ctx = gpu
    k, N = len(made), sum(p.num_points for p in made)
    outs = S._fuse_buffers(torch, dev, k, N)
    links = [(idx[i], a[0], a[1], a[2], a[4]) for i, a in enumerate(aouts)]
    S.fuse_chain_enqueue(ctx, made, links, S.fuse_params(), outs)
    ctx.synchronize()
    return outs, S._fuse_results(outs, k, N)


def against_host_and_twin(HL, state, fused, got, what, hold_to_twin=True):
    """The device's result against the host build (the same bytes: the bars of tests/test_gpu_chain_adjust.py are equality) and
    against the twin, both on the read-back state: within the host-build bars, or (hold_to_twin False) printed only."""
    k, N = len(state["pairs"]), sum(P["n"] for P in state["pairs"])
    host = CS.run_host(HL, S, state, CS.fused_arrays(fused, k, N))
    twin = CR.adjust_chain(state["pairs"], state["K"], fused)
    for key in ("cams", "points", "used", "err", "reports"):
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(host[key]).tobytes(), (what, key)
    assert np.array_equal(got["used"] != 0, twin["used"])
    cams = got["cams"].astype(np.float64)
    drot = max(CS.rotation_angle(cams[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(k))
    dt = float(np.abs(cams[:, 1, 9:] - twin["cams"][:, 1, 9:]).max())
    roots = [p for p in range(k) if got["reports"][p]["root"] == p]
    drms = max(abs(float(got["reports"][p]["final_rms_px"]) - twin["reports"][p]["final_rms_px"]) for p in roots)
    print(f"{what}: device - twin: rot {drot:.3g} rad, t {dt:.3g} (largest |t| component {np.abs(cams[:, 1, 9:]).max():.3g}), rms {drms:.3g} px")
    assert not hold_to_twin or (drot <= BAR_ROT and dt <= BAR_T and drms <= BAR_RMS)
    return twin


def test_full_chain_on_the_device(gpu):
    """5 views, n = 1024 (6h's chain).  Every SFM_BUF_* of every pair is unchanged; the rms falls; the twin on the read-back state
    agrees; the points' median distance to the truth is printed next to the fused points' (no bar: 6g's gauge argument)."""
    torch, dev, ctx = gpu
    HL = CS.host_lib()
    sc, _ = FS.build(1024, 61, views=5)
    made, reports = refined_chain(gpu, sc)
    idx = [to_dev(torch, dev, L["index"]) for L in sc["links"]]
    aouts = aligned(gpu, made, idx)
    outs, fused = fuse_on_device(gpu, made, idx, aouts)
    before = [read_buffers(p, ctx) for p in made]
    got = S.adjust_chain(made, outs)
    for p, bufs in zip(made, before):
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    state = read_back_chain(torch, made, idx, aouts, sc["K"], sc["Kinv"])
    rep = got["reports"][0]
    print(f"full chain: {fused['counts']}; adjust: {rep}")
    assert rep["root"] == 0 and rep["num_cameras"] == 4 and rep["status"] != S.REFINE_DEGENERATE and rep["num_tracks"] > 1000
    assert rep["final_rms_px"] < rep["initial_rms_px"]
    for p in range(3):
        assert got["cams"][p + 1, 0].tobytes() == got["cams"][p, 1].tobytes()
    against_host_and_twin(HL, state, fused, got, "full chain")
    truth = FS.truth_in_pair0(sc, state, fused)
    ok = np.isfinite(truth).all(1) & (got["used"] != 0)
    dist = lambda P: np.linalg.norm(P[:3].T[ok].astype(np.float64) - truth[ok], axis=1) / truth[ok, 2]
    print(f"  |X - truth| / depth over {ok.sum()} used tracks: median fused {np.median(dist(fused['points'])):.4g}, adjusted {np.median(dist(got['points'])):.4g}")
    for p in made:
        p.close()


def test_dino_frames_0_to_3_and_the_demo(gpu, tmp_path):
    """Real frames: pairs (0, 1), (1, 2), (2, 3): the counts and the rms are printed and the device equals the host build on the
    read-back state.  The twin's cameras are printed, not held to a bar: the first link has 27 inliers and s = 0.056, the chain is
    not converged after 10 iterations (rms 0.399 -> 0.341 px, 7 steps accepted, status MAX_ITER) and along the weak directions the
    fp32 and fp64 chains are 3.9e-4 rad and 1.97 in t (its components reach 42) apart where their rms differs by 1.7e-4 px.  The `chain adjust:`
    line of fuse_chain_demo is the Python call's report on the same records, and without the new argument the demo prints what it
    printed before."""
    torch, dev, ctx = gpu
    HL = CS.host_lib()
    demo = os.path.join(ROOT, "cuda-sfm_amd", "host", "fuse_chain_demo")
    assert os.path.exists(demo), "fuse_chain_demo not built (make)"
    feats = [dino_extract(gpu, k) for k in range(4)]
    files = []
    for k, (d, n) in enumerate(feats):
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
    aouts = aligned(gpu, made, idx)
    outs, fused = fuse_on_device(gpu, made, idx, aouts)
    got = S.adjust_chain(made, outs)
    state = read_back_chain(torch, made, idx, aouts, DINO_K, DINO_KINV)
    roots = [p for p in range(3) if got["reports"][p]["root"] == p]
    print(f"dino 0..3: fuse {fused['counts']}; adjust " + "; ".join(str(got["reports"][p]) for p in roots))
    against_host_and_twin(HL, state, fused, got, "dino 0..3", hold_to_twin=False)
    for p in roots:
        r = got["reports"][p]
        assert r["status"] == S.REFINE_DEGENERATE or r["final_rms_px"] <= r["initial_rms_px"]
    assert np.isfinite(got["points"]).all()
    for p in made:
        p.close()
    args = [demo, "3", files[0], files[1], files[2], files[1], files[2], files[3]]
    plain = subprocess.run(args + [str(tmp_path / "plain.ply")], capture_output=True, text=True, timeout=300)
    with_adjust = subprocess.run(args + [str(tmp_path / "adjusted.ply"), "10"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and with_adjust.returncode == 0, plain.stdout + plain.stderr + with_adjust.stdout + with_adjust.stderr
    want = ["chain adjust: segment %d: %d cameras, %d tracks, rms %.6g -> %.6g px, %d iterations" %
            (r["root"], r["num_cameras"], r["num_tracks"], r["initial_rms_px"], r["final_rms_px"], r["iterations"]) for r in (got["reports"][p] for p in roots)]
    lines = re.findall(r"^chain adjust: .*$", with_adjust.stdout, flags=re.M)
    print(f"fuse_chain_demo: {lines}; Python: {want}")
    assert lines == want
    # without the new argument: no such line, and everything else as with it (the cloud's file name and the facade's timer lines aside)
    assert "chain adjust:" not in plain.stdout
    strip = lambda text: [l.replace("plain.ply", "X").replace("adjusted.ply", "X") for l in text.splitlines()
                          if not l.startswith("chain adjust:") and " time = " not in l]
    assert strip(plain.stdout) == strip(with_adjust.stdout)
    a, b = open(tmp_path / "plain.ply", "rb").read(), open(tmp_path / "adjusted.ply", "rb").read()
    assert len(a) > 0 and len(b) > 0 and (a != b or all(got["reports"][p]["accepted"] == 0 for p in roots))
