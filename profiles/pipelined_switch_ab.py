"""The pipelined step (two slots, two streams: what bench.py times) through the lab-bench library under two values of reserved[1],
alternating, a fresh process per run under its own time limit; the first failure ends the job.  One JSON line per run.
usage: python profiles/pipelined_switch_ab.py HYPOTHESES SWITCH_A SWITCH_B [REPETITIONS] [OUT_FILE]     (profiles/r12_h524288_pairs_ab.txt)
       python profiles/pipelined_switch_ab.py run HYPOTHESES SWITCH          one run: 20 steps of warm-up, 200 timed"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if sys.argv[1] == "run":
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import cuda_sfm_amd_ab as S
    from cuda_sfm_amd_ab import synth
    H, sw = int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda", 0)
    n = 4096
    scene = synth.two_view_scene(n)
    d_sift = torch.from_numpy(scene["sift"].view(np.uint8).reshape(n, 576)).to(dev)
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.own_stream()
    pair = S.ImagePair(ctx, scene["K"], scene["Kinv"], 2, n)
    pair.fillXU(d_sift)
    p = S.default_params(n, num_hypotheses=H, kernel=S.KERNEL_PREFILTER)
    p.reserved[1] = sw
    for _ in range(20):
        pair.estimateE_pipelined(p)
    pair.flush(); ctx.synchronize(); torch.cuda.synchronize()
    steps = 200
    t0 = time.perf_counter()
    for _ in range(steps):
        pair.estimateE_pipelined(p)
    pair.flush(); ctx.synchronize(); torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    launch = pair.last_launch()
    print(json.dumps({"hypotheses": H, "reserved1": sw, "ms_per_step": dt * 1e3, "lds_bytes": launch["lds_bytes"], "grid": launch["grid"], "best": list(pair.get_best())}))
    sys.exit(0)

H, switches = int(sys.argv[1]), (int(sys.argv[2]), int(sys.argv[3]))
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
out = open(sys.argv[5], "w") if len(sys.argv) > 5 else None
for rep in range(reps):
    for sw in switches:
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "run", str(H), str(sw)], cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            print("FAILED", sw, r.returncode, r.stdout[-1500:], r.stderr[-3000:], flush=True)
            sys.exit(1)
        msg = json.dumps({"rep": rep, **json.loads(lines[-1])})
        print(msg, flush=True)
        if out:
            out.write(msg + "\n"); out.flush()
