"""CPU: the host arithmetic of a batched sfm_process_pairs call (csrc/pairs_batch.hpp, host-compiled into
tests/hostcheck/libpairsplancheck.so): where a job's nine arrays lie in the workspace, and which jobs share a matcher launch.
The lengths the arrays must have are written down HERE from what the many-pairs kernels index (PairJob's comments,
pose.hip: choose_pose_pairs writes chosen[25]), not taken from the layout function."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("m_idx", "X0", "X1", "counts", "Ecand", "key", "mask", "points", "chosen")
NS = (8, 9, 127, 128, 129, 2155, 8192)
HS = (1, 7, 269, 4096)
BASE = 0x7F12_3456_0000 + 3 * 256              # what hipMalloc returns is at least 256-byte aligned


@pytest.fixture(scope="module")
def L():
    h = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpairsplancheck.so"))
    h.ppcheck_carve.argtypes = [C.c_uint64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    h.ppcheck_carve.restype = None
    h.ppcheck_runs.argtypes = [C.c_int, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_int)] * 6
    return h


def needed_bytes(n, H):
    ld = (n + 127) // 128 * 128
    return {"m_idx": n * 4, "X0": 3 * ld * 4, "X1": 3 * ld * 4, "counts": H * 4, "Ecand": H * 36, "key": 16, "mask": n,
            "points": 4 * n * 4, "chosen": 26 * 4}


def carve(L, base, jobs):
    n = (C.c_int * len(jobs))(*[j[0] for j in jobs]); H = (C.c_uint32 * len(jobs))(*[j[1] for j in jobs])
    out = (C.c_uint64 * (10 * len(jobs)))()
    L.ppcheck_carve(base, len(jobs), n, H, out)
    out = np.array(out, dtype=np.uint64).reshape(len(jobs), 10)
    return [dict(zip(ARRAYS, (int(v) for v in row[:9]))) for row in out], [int(row[9]) for row in out]


def check_job(addr, need, lo, hi):
    """One job's arrays inside [lo, hi): aligned, in the documented order, each long enough before the next one starts."""
    assert all(addr[a] % 256 == 0 for a in ARRAYS), addr
    assert [a for a in sorted(ARRAYS, key=lambda a: addr[a])] == list(ARRAYS)
    ends = [addr[a] + need[a] for a in ARRAYS]
    assert addr["m_idx"] >= lo and ends[-1] <= hi
    for a, end, nxt in zip(ARRAYS, ends, list(ARRAYS[1:])):
        assert end <= addr[nxt], (a, nxt)


@pytest.mark.parametrize("n,H", list(itertools.product(NS, HS)))
def test_job_arrays_are_aligned_disjoint_and_long_enough(L, n, H):
    assert L.ppcheck_align() == 256
    need = needed_bytes(n, H)
    (null,), (size,) = carve(L, 0, [(n, H)])
    (real,), (used,) = carve(L, BASE, [(n, H)])
    assert used == size and size % 256 == 0                    # the sizing pass over a null base says what the real pass takes
    assert {a: real[a] - BASE for a in ARRAYS} == null
    check_job(real, need, BASE, BASE + used)
    assert real["mask"] - real["key"] == 256                   # the key and the chosen pose keep 256-byte slots of their own
    assert BASE + used - real["chosen"] == 256
    # two jobs back to back: the second starts where the first ended, and nothing overlaps
    other = (NS[(NS.index(n) + 3) % len(NS)], HS[(HS.index(H) + 1) % len(HS)])
    both, used2 = carve(L, BASE, [(n, H), other])
    assert both[0] == real and used2[0] == used
    assert both[1]["m_idx"] == BASE + used
    check_job(both[1], needed_bytes(*other), BASE + used, BASE + used2[1])
    assert used2[1] == used + carve(L, 0, [other])[1][0]


def runs_of(L, views, ns, db_rows, picks):
    k = len(views)
    arr = lambda v: (C.c_int * k)(*v)
    begin, end, kernel = arr([0] * k), arr([0] * k), arr([0] * k)
    r = L.ppcheck_runs(k, (C.c_uint64 * k)(*views), arr(ns), arr(db_rows), arr(picks), begin, end, kernel)
    return [(begin[i], end[i], kernel[i]) for i in range(r)]


def test_match_runs_break_at_another_view_another_n_and_the_prefilter(L):
    A, B, fused, pf = 0x1000, 0x2000, 3, L.ppcheck_prefilter_id()
    assert fused != pf
    # first views A A A B A A; the third A has another n; the kernel choice says pre-filter for the fifth
    runs = runs_of(L, [A, A, A, B, A, A], [500, 500, 460, 500, 500, 500], [601, 602, 603, 604, 605, 606], [fused, fused, fused, fused, pf, fused])
    assert [(b, e) for b, e, _ in runs] == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert [e - 1 for _, e, _ in runs] == [1, 2, 3, 4, 5]      # the record writer: the last member of each run
    assert [k for _, _, k in runs] == [fused, -1, -1, -1, -1]  # a single pair goes through the matcher rule of sfm_match
    # a run ends where the kernel choice changes, and a second view without rows is never part of one
    runs = runs_of(L, [A] * 6, [500] * 6, [601, 602, 603, 604, 0, 606], [fused, fused, 1, 1, fused, fused])
    assert runs == [(0, 2, fused), (2, 4, 1), (4, 5, -1), (5, 6, -1)]
    assert runs_of(L, [], [], [], []) == []
