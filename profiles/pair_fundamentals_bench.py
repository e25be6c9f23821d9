"""Cost of one sfm_pair_fundamentals call beside the loop of sfm_pair_fundamental calls over the same pairs: HIP events around the
enqueued calls, warmed up, medians of three alternating repetitions in one run (each repetition: `inner` rounds of one kind
between two events, then the other kind).  Both kinds go through ctypes with arguments built beforehand, so a round of the loop
costs the host one foreign call per pair.  Pairs: synth.two_view_scene(256) after estimateE, refined = 0; 1, 36 and 630 pairs.
    python profiles/pair_fundamentals_bench.py > profiles/pair_fundamentals_bench.txt"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cuda_sfm_amd as S  # noqa: E402
from cuda_sfm_amd import synth  # noqa: E402

L = S.lib()


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
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 36, 630])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    print(f"# {torch.cuda.get_device_name(0)}; medians of {a.reps} alternating repetitions, HIP events")
    print("# pairs | sfm_pair_fundamentals ms | loop of sfm_pair_fundamental ms | loop / batched | batched us per pair | loop us per pair | margin against the repetitions' spreads")
    pairs, keep = [], []
    for k in range(max(a.counts)):
        sc = synth.two_view_scene(256, seed=900 + k % 8)
        d = torch.from_numpy(sc["sift"].view(np.uint8).reshape(256, 576)).to(dev)
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, 256)
        pair.fillXU(d)
        pair.estimateE(S.default_params(256, num_hypotheses=256))
        pairs.append(pair); keep.append(d)
    for count in a.counts:
        inner = max(3, min(200, 2000 // count))
        handles = (C.c_void_p * count)(*[p._h.value for p in pairs[:count]])
        table = torch.empty((count, 9), dtype=torch.float32, device=dev)
        each = torch.empty((count, 9), dtype=torch.float32, device=dev)
        single = [(pairs[k]._h, 0, each[k].data_ptr()) for k in range(count)]

        def batched():
            assert L.sfm_pair_fundamentals(handles, count, 0, table.data_ptr()) == S.OK

        def loop():
            for args in single:
                L.sfm_pair_fundamental(*args)
        batched(); loop(); torch.cuda.synchronize()
        assert torch.equal(table, each), "sfm_pair_fundamentals and the loop differ"
        times = alternate([("batched", batched), ("loop", loop)], inner, a.reps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(max(v) - min(v)) for k, v in times.items()}
        print(f"{count} | {med['batched']:.4f} | {med['loop']:.4f} | {med['loop'] / med['batched']:.2f} | {1e3 * med['batched'] / count:.2f} | {1e3 * med['loop'] / count:.2f} | "
              f"margin {med['loop'] - med['batched']:+.4f} ms against spreads {spread['batched']:.4f} / {spread['loop']:.4f} ms   (inner {inner}; all repetitions: "
              + "; ".join(f"{k} " + " ".join(f"{x:.4f}" for x in v) for k, v in times.items()) + ")", flush=True)


if __name__ == "__main__":
    main()
