"""Another checkout of this project (already built) against this tree, alternately, on one box: bench.py headline, bench.py --config c4
and profiles/enqueue_probe.py, a fresh process per run under its own time limit; the first failure ends the job.  One JSON line per
result line of a run.  usage: python profiles/ab_two_trees.py OTHER_TREE [REPETITIONS] [OUT_FILE] [PROGRAM,PROGRAM...]   (profiles/r10_slot_ab.txt)
Without a program list: the first three of PROGRAMS (round 10's set); round 11 added the other bench sizes and --dump-outputs."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = (("parent", os.path.abspath(sys.argv[1])), ("this", ROOT))
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
PROGRAMS = (("bench_headline", ["bench.py"]), ("bench_c4", ["bench.py", "--config", "c4"]), ("enqueue_probe", ["profiles/enqueue_probe.py"]),
            ("bench_c3", ["bench.py", "--config", "c3"]), ("bench_h524288", ["bench.py", "--hyps", "524288"]), ("bench_h131072", ["bench.py", "--hyps", "131072"]),
            ("bench_serial", ["bench.py", "--serial"]))
KEEP = ("ms_per_step", "serial_ms_per_step", "value", "unit", "hypotheses", "pipelined_enqueue_us_per_step", "pipelined_total_us_per_step",
        "serial_enqueue_us_per_step", "serial_total_us_per_step")
PROGRAMS = tuple(pr for pr in PROGRAMS if pr[0] in sys.argv[4].split(",")) if len(sys.argv) > 4 else PROGRAMS[:3]

out = open(OUT, "w") if OUT else None
for name, cmd in PROGRAMS:
    for rep in range(REPS):
        for tree, path in TREES:
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable] + cmd, cwd=path, capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            for ln in lines:
                rec = json.loads(ln)
                msg = json.dumps({"program": name, "rep": rep, "tree": tree, **{k: rec[k] for k in KEEP if k in rec}})
                print(msg, flush=True)
                if out:
                    out.write(msg + "\n"); out.flush()
            if r.returncode != 0 or not lines:
                print("FAILED", name, tree, r.returncode, r.stdout[-1500:], r.stderr[-3000:], flush=True)
                sys.exit(1)
