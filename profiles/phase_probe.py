"""Where block 0 of ransac_score_prefilter spends its time (sfm_ransac_last_phases), per shard size and grid width.
python profiles/phase_probe.py LABEL [reserved1 [reserved3 [samples]]]: 2^20 hypotheses only, with those lab-bench switches
(include/sfm_amd_ab.h), `samples` launches stamped, each line tagged LABEL and carrying the drain (ring_drained - first_block_scanned)
and the epilogue (first_pass_done - ring_drained) -- profiles/r09_phase_probe.txt; paired passes also carry the time from the end
of the first pair's first scan to the start of its second and the ring entries held there (profiles/r12_phase_probe.txt)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import cuda_sfm_amd_ab as S            # the lab-bench flavour (make ab): switches, probes, traces
from cuda_sfm_amd_ab import synth

dev = torch.device("cuda", 0)
ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
n = 4096
scene = synth.two_view_scene(n)
d_sift = torch.from_numpy(scene["sift"].view(np.uint8).reshape(n, 576)).to(dev)
pair = S.ImagePair(ctx, scene["K"], scene["Kinv"], 2, n)
pair.fillXU(d_sift)
label = sys.argv[1] if len(sys.argv) > 1 else None
r1, r3, samples = (int(sys.argv[k]) if len(sys.argv) > k else d for k, d in ((2, 0), (3, 0), (4, 1)))
cases = ((1048576, 0),) * samples if label else ((131072, 0), (131072, 64), (262144, 0), (1048576, 0), (1048576, 64))
for H, cols in cases:
    p = S.default_params(n, num_hypotheses=H, seed=3, kernel=S.KERNEL_PREFILTER)
    p.reserved[1], p.reserved[2], p.reserved[3] = r1, cols, r3
    for _ in range(10):
        pair.estimateE(p)
    ctx.kernel_timing(True) if hasattr(ctx, "kernel_timing") else None
    pair.estimateE(p)
    t = [int(v) for v in pair.last_phases()]
    boundary_ticks, held = t[3] >> 32, t[6] >> 32          # paired passes: first scan's end -> second scan's start; ring entries held at second scans
    t[3] &= 0xFFFFFFFF; t[6] &= 0xFFFFFFFF
    us = lambda k: round(t[k] / 100.0, 2)
    tag = {"build": label, "reserved": [0, r1, cols, r3], "drain_us": round((t[7] - t[4]) / 100.0, 2), "epilogue_us": round((t[5] - t[7]) / 100.0, 2)} if label else {}
    print(json.dumps({**tag, "hypotheses": H, "grid": pair.last_launch()["grid"], "block0_lifetime_us": us(1), "tile_staged_us": us(2), "first_pass_prepared_us": us(3),
                      "first_block_scanned_us": us(4), "ring_drained_us": us(7), "first_pass_done_us": us(5), "passes_of_wave0": t[6], "scan_boundary_us": round(boundary_ticks / 100.0, 2), "entries_held_at_second_scans": held,
                      "shader_mhz": round(100.0 * t[0] / max(t[1], 1))}), flush=True)
