"""Cost of sfm_register_view: HIP events around enqueued calls (no host sync inside), after the calls' inputs are on the device.
  dino: frames 0, 1, 2 of tests/golden/dino (extract, match 0-1, fillXU, estimateE, refine, match 0-2), the defaults
        (4096 hypotheses, 10 LM iterations);
  synthetic: a third view over two_view_scene's points (exact 3-D points through d_points, 0.5 px noise, 30 % outliers) with
        m candidates and H hypotheses, plus a max_iterations = 0 run (gate + RANSAC only).
Prints one line per case.  Kernel split: run once under `rocprofv3 --kernel-trace --stats -- python profiles/register_bench.py`."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
from cuda_sfm_amd import synth  # noqa: E402
from helpers import DINO_K, DINO_KINV, DINO_SIFT, read_pnm_grey  # noqa: E402
import register_scene as RS  # noqa: E402


def timed(pair, d_sift, p, calls):
    for _ in range(3):
        pair.register_enqueue(d_sift, p)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        pair.register_enqueue(d_sift, p)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls, pair.get_register_report()


def line(name, us, rep):
    return (f"{name}: {us:.1f} us per call; candidates {rep['num_candidates']}, ransac inliers {rep['ransac_inliers']}, "
            f"final inliers {rep['num_inliers']}, iterations {rep['iterations']}, rms {rep['initial_rms_px']:.4f} -> "
            f"{rep['final_rms_px']:.4f} px")


def dino(ctx, dev, calls):
    def extract(k):
        img = read_pnm_grey(os.path.join(ROOT, "tests", "golden", "dino", f"dino_grey_{k:03d}.pgm"))
        h, w = img.shape
        pitch = (w + 127) // 128 * 128
        pad = np.zeros((h, pitch), np.float32); pad[:, :w] = img
        d = torch.zeros((32768, 576), dtype=torch.uint8, device=dev)
        n, _ = ctx.extract_sift(d, 32768, torch.from_numpy(pad).to(dev), w, h, pitch, **DINO_SIFT)
        return d, n
    (d0, n0), (d1, n1), (d2, n2) = extract(0), extract(1), extract(2)
    ctx.match(d0, n0, d1, n1)
    pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, n0)
    pair.fillXU(d0)
    pair.estimateE(S.default_params(n0))
    pair.refine(max_iterations=20)
    ctx.match(d0, n0, d2, n2)
    for it in (10, 0):
        us, rep = timed(pair, d0, S.register_params(max_iterations=it), calls)
        print(line(f"dino 0-1-2 n={n0} H=4096 max_iterations={it}", us, rep), flush=True)
    pair.close()


def synthetic(ctx, dev, m, H, calls):
    sc = synth.two_view_scene(m, seed=7)
    d_sift = torch.from_numpy(sc["sift"].view(np.uint8).reshape(m, 576)).to(dev)
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, m)
    pair.fillXU(d_sift)
    rec, _ = RS.third_view(sc, seed=7, noise_px=0.5, outlier_frac=0.3)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(m, 576)).to(dev)
    d_pts = torch.from_numpy(RS.homogeneous(sc["points3d"])).to(dev)
    for it in (10, 0):
        us, rep = timed(pair, d_rec, S.register_params(points=d_pts, num_hypotheses=H, max_iterations=it), calls)
        print(line(f"synthetic m={m} H={H} max_iterations={it}", us, rep), flush=True)
    pair.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--no-dino", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    if not a.no_dino:
        dino(ctx, dev, a.calls)
    for m in (4096, 16384):
        for H in (4096, 65536):
            synthetic(ctx, dev, m, H, a.calls)


if __name__ == "__main__":
    main()
