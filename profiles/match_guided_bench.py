"""Cost of one sfm_match_guided call beside sfm_match on the same records: HIP events around the enqueued calls, warmed up,
medians of three alternating repetitions in one run (each repetition: `inner` calls of one kind between two events, then the
next kind).  Records: tests/match_guided_scene.scene(n, n, 7) (half of the descriptors in groups of four), its true F, a band
of 4 px.  sfm_match runs under SFM_MATCH_EXACT (the same kernel without the gate) and under AUTO (what a caller gets).
    python profiles/match_guided_bench.py > profiles/match_guided_bench.txt
Kernel split, in a run of its own: rocprofv3 --kernel-trace --stats -- python profiles/match_guided_bench.py --sizes 4096 --reps 1"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
import match_guided_scene as MS  # noqa: E402

NAMES = {S.MATCH_EXACT: "exact", S.MATCH_PREFILTER: "pre-filter", S.MATCH_FUSED: "fused"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--band", type=float, default=4.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# {torch.cuda.get_device_name(0)}; band {a.band} px; medians of {a.reps} alternating repetitions, HIP events")
    print("# n x n | guided ms | sfm_match EXACT ms | sfm_match AUTO ms (kernel) | guided / EXACT | guided / AUTO | queries matched guided / plain")
    for n in a.sizes:
        sc = MS.scene(n, n, 7)
        up = lambda r: torch.from_numpy(np.array(r, copy=True).view(np.uint8).reshape(len(r), 576)).to(dev)
        d1, d2 = up(sc["sift1"]), up(sc["sift2"])
        dF = torch.from_numpy(np.asarray(sc["F"], np.float32).reshape(9).copy()).to(dev)
        inner = max(8, min(200, int(2e10 / (float(n) * n * 128))))         # ~40 calls at 2048^2, 8 at 16384^2

        def guided():
            S.match_guided(ctx, d1, n, d2, n, dF, band_px=a.band)

        def plain(kernel):
            def call():
                ctx.match(d1, n, d2, n)
            call.kernel = kernel
            return call
        kinds = [("guided", guided), ("exact", plain(S.MATCH_EXACT)), ("auto", plain(S.MATCH_AUTO))]
        times = {k: [] for k, _ in kinds}
        picked = None
        for rep in range(a.reps + 1):                                    # repetition 0 warms up
            for name, call in kinds:
                ctx.set_match_kernel(getattr(call, "kernel", S.MATCH_AUTO))
                call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    call()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) / inner)
                if name == "auto":
                    picked = ctx.last_match_kernel()
        ctx.set_match_kernel(S.MATCH_AUTO)
        guided(); torch.cuda.synchronize()
        g = int((d1.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)["match"] >= 0).sum())
        ctx.match(d1, n, d2, n); torch.cuda.synchronize()
        p = int((d1.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)["match"] >= 0).sum())
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(f"{n} x {n} | {med['guided']:.4f} | {med['exact']:.4f} | {med['auto']:.4f} ({NAMES.get(picked, picked)}) | "
              f"{med['guided'] / med['exact']:.3f} | {med['guided'] / med['auto']:.3f} | {g} / {p}   (inner {inner}; all repetitions: "
              + "; ".join(f"{k} " + " ".join(f"{x:.4f}" for x in v) for k, v in times.items()) + ")", flush=True)


if __name__ == "__main__":
    main()
