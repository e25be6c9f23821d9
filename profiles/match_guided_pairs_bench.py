"""Cost of one sfm_match_guided_pairs call beside the loop of sfm_match_guided calls over the same records: HIP events around
the enqueued calls, warmed up, medians of three alternating repetitions in one run (each repetition: `inner` rounds of one kind
between two events, then the other kind).  Both kinds go through ctypes with arguments built beforehand, so a round of the loop
costs the host one foreign call per job.  Records: tests/match_guided_scene.scene(n, n, seed) for eight seeds, its true F, a band
of 4 px; every job has its own copy of the first set (the call writes it), jobs of one seed share the second set and the F.
Shapes (jobs x n): 36 and 630 x 2155, 36 x 256, 8 x 4600, 1 x 2155.
    python profiles/match_guided_pairs_bench.py > profiles/match_guided_pairs_bench.txt"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
import match_guided_scene as MS  # noqa: E402

L = S.lib()
SEEDS = 8


def alternate(kinds, inner, reps):
    """{name: [ms per round]}: repetition 0 warms up; every repetition times `inner` rounds of each kind in turn"""
    times = {k: [] for k, _ in kinds}
    for rep in range(reps + 1):
        for name, call in kinds:
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
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", type=str, nargs="+", default=["36x2155", "630x2155", "36x256", "8x4600", "1x2155"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    params = S.match_guided_params(band_px=4.0)
    print(f"# {torch.cuda.get_device_name(0)}; band 4.0 px; medians of {a.reps} alternating repetitions, HIP events")
    print("# jobs x n | sfm_match_guided_pairs ms | loop of sfm_match_guided ms | loop / batched | batched us per job | loop us per job | margin against the repetitions' spreads")
    up = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), 576)).to(dev)
    for shape in a.shapes:
        count, n = (int(v) for v in shape.split("x"))
        scenes = [MS.scene(n, n, 7 + s) for s in range(min(SEEDS, count))]
        second = [up(sc["sift2"]) for sc in scenes]
        Fs = [torch.from_numpy(np.asarray(sc["F"], np.float32).reshape(9).copy()).to(dev) for sc in scenes]
        first = [up(scenes[k % len(scenes)]["sift1"]) for k in range(count)]
        tuples = [(first[k], n, second[k % len(scenes)], n, Fs[k % len(scenes)]) for k in range(count)]
        jobs = S.match_guided_jobs(tuples)
        single = [(ctx._h, t[0].data_ptr(), n, t[2].data_ptr(), n, t[4].data_ptr(), C.byref(params)) for t in tuples]
        inner = max(3, min(100, 1500 // count))

        def batched():
            assert L.sfm_match_guided_pairs(ctx._h, jobs, count, C.byref(params)) == S.OK

        def loop():
            for args in single:
                L.sfm_match_guided(*args)
        batched(); torch.cuda.synchronize()
        got = [f.clone() for f in first[:SEEDS]]
        for f in first[:SEEDS]:
            f[:, 24:44] = 0                                    # the five match fields (bytes 24 .. 43 of a record)
        loop(); torch.cuda.synchronize()
        assert all(torch.equal(g, f) for g, f in zip(got, first)), "sfm_match_guided_pairs and the loop differ"
        times = alternate([("batched", batched), ("loop", loop)], inner, a.reps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(max(v) - min(v)) for k, v in times.items()}
        print(f"{count} x {n} | {med['batched']:.4f} | {med['loop']:.4f} | {med['loop'] / med['batched']:.2f} | {1e3 * med['batched'] / count:.2f} | {1e3 * med['loop'] / count:.2f} | "
              f"margin {med['loop'] - med['batched']:+.4f} ms against spreads {spread['batched']:.4f} / {spread['loop']:.4f} ms   (inner {inner}; all repetitions: "
              + "; ".join(f"{k} " + " ".join(f"{x:.4f}" for x in v) for k, v in times.items()) + ")", flush=True)
        del first, second, tuples, jobs, single


if __name__ == "__main__":
    main()
