"""How much of each lane-solve launch runs under the OTHER slot's scoring launch, out of a rocprofv3 --kernel-trace of bench.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 50
    python profiles/r07_overlap_from_trace.py DIR [last_n_solves]

For the last `last_n_solves` (default 50: the timed steps of the last region) ransac_solve_lanes1_qr launches: the fraction of the
launch's interval that lies inside ransac_score_prefilter intervals of another stream (the other slot's), and the mean durations
of both kernels over the same stretch.  Prints one JSON line."""
import csv
import glob
import json
import os
import sys


def rows(directory):
    out = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                r = {k.lower(): v for k, v in r.items()}
                out.append((r["kernel_name"], int(r["start_timestamp"]), int(r["end_timestamp"]), r.get("stream_id") or r.get("queue_id", ""), r.get("process_id", r.get("pid", ""))))
    return out


def main():
    directory = sys.argv[1]
    last_n = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    all_rows = rows(directory)
    assert all_rows, f"no kernel trace under {directory}"
    # the process with the most solve launches is the bench itself (a one-rank exchange probe may run as a child)
    by_pid = {}
    for name, s, e, q, pid in all_rows:
        if "ransac_solve_lanes1_qr" in name:
            by_pid[pid] = by_pid.get(pid, 0) + 1
    pid = max(by_pid, key=by_pid.get)
    solves = sorted((s, e, q) for name, s, e, q, p in all_rows if p == pid and "ransac_solve_lanes1_qr" in name)[-last_n:]
    t0 = solves[0][0]
    scores = sorted((s, e, q) for name, s, e, q, p in all_rows if p == pid and "ransac_score_prefilter" in name and e >= t0)
    fractions = []
    for s, e, q in solves:
        covered = 0
        for ss, se, sq in scores:
            if sq != q and se > s and ss < e:
                covered += min(e, se) - max(s, ss)
        fractions.append(min(1.0, covered / max(1, e - s)))
    fractions.sort()
    span = (max(e for _, e, _ in scores) - t0) / max(1, len(solves))
    print(json.dumps({
        "trace": directory, "solve_launches": len(solves), "score_launches": len(scores),
        "solve_under_other_slots_scoring": {"mean": sum(fractions) / len(fractions), "median": fractions[len(fractions) // 2], "min": fractions[0], "max": fractions[-1]},
        "solve_mean_us": sum(e - s for s, e, _ in solves) / len(solves) / 1e3,
        "score_mean_us": sum(e - s for s, e, _ in scores) / len(scores) / 1e3,
        "us_per_step_in_trace": span / 1e3,
    }))


if __name__ == "__main__":
    main()
