"""CPU: the Levenberg-Marquardt control the one-block solvers share (LmControl in csrc/refine_math.hpp, host-compiled into
tests/hostcheck/librefinecheck.so) against a model of its rules written here -- the rules of the two numpy twins
(tests/refine_reference.py, tests/register_reference.py).  Seeded random sequences of iteration outcomes ("the solve failed" /
"the tentative state costs nc, nsq") are replayed through both; every report field must be equal exactly (fp64 on both sides)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "hostcheck", "librefinecheck.so")
CONVERGED, MAX_ITER, DEGENERATE = 0, 1, 2          # SFM_REFINE_* of include/sfm_amd.h
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def L():
    h = C.CDLL(LIB)
    h.rc_lm_replay.argtypes = [C.c_double] * 3 + [C.c_int, C.c_int, C.c_double, C.c_int, i32p, f64p, f64p, f64p, i32p]
    h.rc_lm_replay.restype = None
    return h


def model(lambda0, cost0, sq0, degenerate, max_iterations, min_rel, events):
    """-> (lambda, cost, sq, iterations, accepted, status, events consumed), why the chain ended"""
    lam, cost, sq = np.float64(lambda0), np.float64(cost0), np.float64(sq0)
    iters = accepted = used = 0
    status, why = (DEGENERATE, "degenerate") if degenerate else (MAX_ITER, "events")
    for failed, nc, nsq in events:
        if status == DEGENERATE:
            break
        if iters >= max_iterations:
            why = "max_iterations"
            break
        used += 1
        iters += 1
        if not failed and nc < cost:
            with np.errstate(all="ignore"):
                rel = (cost - nc) / cost
            cost, sq, accepted, lam = np.float64(nc), np.float64(nsq), accepted + 1, lam / 10.0
            if not (rel >= min_rel):
                status, why = CONVERGED, "converged"
                break
        else:
            lam = lam * 10.0
            if lam > 1e16:
                why = "overflow_failed" if failed else "overflow_rejected"
                break
    return (float(lam), float(cost), float(sq), iters, accepted, status, used), why


def replay(L, lambda0, cost0, sq0, degenerate, max_iterations, min_rel, events):
    n = len(events)
    failed = np.ascontiguousarray([e[0] for e in events], np.int32)
    nc = np.ascontiguousarray([e[1] for e in events], np.float64)
    nsq = np.ascontiguousarray([e[2] for e in events], np.float64)
    dout, iout = np.zeros(3, np.float64), np.zeros(4, np.int32)
    L.rc_lm_replay(lambda0, cost0, sq0, int(degenerate), max_iterations, min_rel, n,
                   failed.ctypes.data_as(i32p), nc.ctypes.data_as(f64p), nsq.ctypes.data_as(f64p),
                   dout.ctypes.data_as(f64p), iout.ctypes.data_as(i32p))
    return (float(dout[0]), float(dout[1]), float(dout[2]), int(iout[0]), int(iout[1]), int(iout[2]), int(iout[3]))


def same(a, b):
    """exact equality field by field, NaN equal to NaN (compared as bit patterns)"""
    return np.array_equal(np.array(a[:3], np.float64).view(np.uint64), np.array(b[:3], np.float64).view(np.uint64)) and a[3:] == b[3:]


def random_case(rng):
    """one (arguments, events); the kind of sequence is drawn so that every way a chain can end turns up often"""
    kind = rng.integers(0, 8)
    lambda0 = float(10.0 ** rng.uniform(-6, 3))
    cost0 = float(10.0 ** rng.uniform(-3, 6))
    sq0 = cost0 * float(rng.uniform(1.0, 3.0))
    max_iterations = int(rng.integers(0, 40))
    min_rel = float(np.float32(10.0 ** rng.uniform(-9, -2)))
    n = int(rng.integers(0, 60))
    degenerate = False
    p_fail, lo, hi = 0.15, 0.5, 1.3                     # a tentative cost is the last one times a factor in [lo, hi)
    if kind == 1:                                       # only rejected steps: lambda overflows on the reject path
        p_fail, lo, hi, max_iterations, n = 0.0, 1.0, 2.0, 64, 64
    elif kind == 2:                                     # only failed solves: lambda overflows on that path
        p_fail, max_iterations, n = 1.0, 64, 64
    elif kind == 3:                                     # decreases that fall below min_rel
        p_fail, lo, hi, min_rel = 0.05, 1.0 - 1e-4, 1.0 + 1e-5, float(np.float32(10.0 ** rng.uniform(-6, -3)))
    elif kind == 4:                                     # min_rel = 0: no finite decrease converges
        min_rel, lo, hi = 0.0, 0.9, 1.05
    elif kind == 5:                                     # more events than iterations allowed
        max_iterations, n = int(rng.integers(1, 12)), 40
    elif kind == 6:
        degenerate = bool(rng.integers(0, 2))
    events, last = [], cost0
    for _ in range(n):
        failed = bool(rng.random() < p_fail)
        nc = last * float(rng.uniform(lo, hi))
        if kind == 7 and rng.random() < 0.15:           # a cost that is not a number, or not finite
            nc = float(rng.choice([np.nan, np.inf]))
        elif not failed and nc < last:
            last = nc
        events.append((failed, nc, nc * float(rng.uniform(1.0, 3.0))))
    if kind == 7 and rng.random() < 0.2:
        cost0 = float("nan")
    return (lambda0, cost0, sq0, degenerate, max_iterations, min_rel, events)


def test_lm_control_matches_the_model_on_random_sequences(L):
    rng = np.random.default_rng(20261017)
    ends = {}
    for _ in range(4000):
        case = random_case(rng)
        want, why = model(*case)
        got = replay(L, *case)
        assert same(got, want), f"{case[:6]} events {case[6]}: control {got}, model {want} ({why})"
        ends[why] = ends.get(why, 0) + 1
    for why in ("max_iterations", "converged", "overflow_rejected", "overflow_failed", "events", "degenerate"):
        assert ends.get(why, 0) >= 20, f"only {ends.get(why, 0)} sequences ended by {why}: {ends}"


def test_lm_control_named_cases(L):
    ev = lambda *costs: [(False, c, 2.0 * c) for c in costs]
    fail = (True, 0.0, 0.0)
    cases = {
        "no iterations allowed": (1e-3, 10.0, 20.0, False, 0, 1e-6, ev(5.0)),
        "degenerate start": (1e-3, 10.0, 20.0, True, 20, 1e-6, ev(5.0)),
        "min_rel 0 never converges": (1e-3, 10.0, 20.0, False, 20, 0.0, ev(9.0, 9.0 - 1e-12, 8.0)),
        "an equal cost is a rejection": (1e-3, 10.0, 20.0, False, 20, 1e-6, ev(10.0, 10.0)),
        "NaN tentative cost is a rejection": (1e-3, 10.0, 20.0, False, 20, 1e-6, ev(float("nan"), 9.0)),
        "NaN start cost rejects everything": (1.0, float("nan"), 1.0, False, 40, 1e-6, ev(*[1.0] * 40)),
        "infinite start cost: the first finite step converges": (1e-3, float("inf"), 1.0, False, 20, 1e-6, ev(9.0, 8.0)),
        "overflow by failed solves": (1e-3, 10.0, 20.0, False, 40, 1e-6, [fail] * 40),
        "overflow by rejections": (1e-3, 10.0, 20.0, False, 40, 1e-6, ev(*[11.0] * 40)),
        "overflow by both": (1e-3, 10.0, 20.0, False, 40, 1e-6, [fail, (False, 11.0, 1.0)] * 20),
        "small decrease converges": (1e-3, 10.0, 20.0, False, 20, 1e-6, ev(9.0, 9.0 - 1e-9, 1.0)),
        "max_iterations": (1e-3, 10.0, 20.0, False, 3, 1e-6, ev(9.0, 8.0, 7.0, 6.0)),
    }
    expect_why = {"no iterations allowed": "max_iterations", "degenerate start": "degenerate", "min_rel 0 never converges": "events",
                  "NaN start cost rejects everything": "overflow_rejected", "overflow by failed solves": "overflow_failed",
                  "infinite start cost: the first finite step converges": "converged",
                  "overflow by rejections": "overflow_rejected", "small decrease converges": "converged", "max_iterations": "max_iterations"}
    for name, case in cases.items():
        want, why = model(*case)
        got = replay(L, *case)
        assert same(got, want), f"{name}: control {got}, model {want}"
        if name in expect_why:
            assert why == expect_why[name], f"{name}: the model ended by {why}"
    # two of them spelled out, so that the model itself is pinned: 1e-3 * 10^20 > 1e16 after exactly 20 steps up
    got = replay(L, *cases["overflow by failed solves"])
    assert got[3:] == (20, 0, MAX_ITER, 20) and got[0] > 1e16
    got = replay(L, *cases["small decrease converges"])
    assert got[3:] == (2, 2, CONVERGED, 2) and got[1] == 9.0 - 1e-9
