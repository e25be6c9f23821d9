"""CPU: the buffer-range rules of the batched calls (csrc/buffer_ranges.hpp) and the job order of their launches
(csrc/job_order.hpp), host-compiled into tests/hostcheck/libbufferrangescheck.so, against a brute-force restatement over all
pairs of ranges written here.  Random sets with addresses from a small interval in steps of four bytes: overlaps, touching
ranges, equal starts, null pointers and empty ranges are all common."""
import ctypes as C
import itertools
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x10000


@pytest.fixture(scope="module")
def L():
    h = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libbufferrangescheck.so"))
    u64p, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    h.br_first_in_set.argtypes = h.br_first_across_owners.argtypes = [u64p, u64p, ip, ip, C.c_int, ip, ip]
    h.br_bytes_until_known.argtypes = [C.c_int, C.c_uint64]; h.br_bytes_until_known.restype = C.c_uint64
    h.jo_order.argtypes = [ip, C.c_int, ip]
    return h


def call(fn, ranges):
    """ranges: list of (addr, bytes, out, owner).  None, or the indices (a, b) the function names."""
    n = len(ranges)
    addr = (C.c_uint64 * n)(*[r[0] for r in ranges]); size = (C.c_uint64 * n)(*[r[1] for r in ranges])
    out = (C.c_int * n)(*[int(r[2]) for r in ranges]); owner = (C.c_int * n)(*[r[3] for r in ranges])
    a, b = C.c_int(-1), C.c_int(-1)
    return (a.value, b.value) if fn(addr, size, out, owner, n, C.byref(a), C.byref(b)) else None


def overlap(x, y):
    """A null pointer and an empty range lie on nothing; ranges that only touch do not overlap."""
    return bool(x[0] and y[0] and x[1] and y[1] and x[0] < y[0] + y[1] and y[0] < x[0] + x[1])


def conflict(x, y):
    return overlap(x, y) and (x[2] or y[2])


def scan_in_set(ranges):
    """The declaration-order scan: the outputs in order, each against every input, then against the outputs after it."""
    for o, x in enumerate(ranges):
        if not x[2]:
            continue
        for i, y in enumerate(ranges):
            if not y[2] and overlap(x, y):
                return o, i
        for q in range(o + 1, len(ranges)):
            if ranges[q][2] and overlap(x, ranges[q]):
                return o, q
    return None


def random_sets(count, seed):
    rng = random.Random(seed)
    for _ in range(count):
        span = rng.choice((16, 64, 256, 1024))            # in units of four bytes: from "everything collides" to "mostly apart"
        ranges = []
        for owner in range(rng.randint(1, 8)):
            for _ in range(rng.randint(2, 10)):
                addr = 0 if rng.random() < 0.05 else BASE + 4 * rng.randrange(span)
                size = 0 if rng.random() < 0.05 else 4 * rng.randint(1, 6)
                ranges.append((addr, size, rng.random() < 0.5, owner))
        yield rng, ranges


def test_rule_inside_one_set(L):
    refused = passed = 0
    for _, ranges in random_sets(3000, 1):
        for owner in sorted({r[3] for r in ranges}):
            one = [r for r in ranges if r[3] == owner]
            got = call(L.br_first_in_set, one)
            brute = any(conflict(x, y) for x, y in itertools.combinations(one, 2))
            assert (got is not None) == brute, one
            assert got == scan_in_set(one), one
            refused += brute; passed += not brute
        assert call(L.br_first_in_set, ranges) == scan_in_set(ranges), ranges        # the owners play no part in this rule
    assert refused > 1000 and passed > 1000, (refused, passed)


def repaired(ranges):
    """The same set without a conflict inside any owner (the sweep's precondition): the output of each one is made null."""
    ranges = list(ranges)
    for owner in sorted({r[3] for r in ranges}):
        idx = [k for k, r in enumerate(ranges) if r[3] == owner]
        while True:
            hit = scan_in_set([ranges[k] for k in idx])
            if hit is None:
                break
            k = idx[hit[0]]
            ranges[k] = (0,) + ranges[k][1:]
    return ranges


def test_sweep_across_owners(L):
    refused = passed = 0
    for rng, raw in random_sets(3000, 2):
        ranges = repaired(raw)
        for owner in {r[3] for r in ranges}:
            assert call(L.br_first_in_set, [r for r in ranges if r[3] == owner]) is None
        rng.shuffle(ranges)                                                        # the order of the list plays no part
        got = call(L.br_first_across_owners, ranges)
        brute = any(x[3] != y[3] and conflict(x, y) for x, y in itertools.combinations(ranges, 2))
        assert (got is not None) == brute, ranges
        if got is not None:
            x, y = ranges[got[0]], ranges[got[1]]
            assert got[0] != got[1] and x[3] != y[3] and conflict(x, y), (ranges, got)
        refused += brute; passed += not brute
    assert refused > 500 and passed > 500, (refused, passed)


def test_sweep_alone_does_not_replace_the_rule_inside_an_owner(L):
    """The documented precondition: inputs [0, 100) of owner 0 and [10, 50) of owner 1, output [20, 30) of owner 0.  The output lies
    on owner 1's input, but the range that ends last at its start is its own owner's input: the sweep passes, the rule inside
    owner 0 refuses."""
    ranges = [(BASE, 100, False, 0), (BASE + 10, 40, False, 1), (BASE + 20, 10, True, 0)]
    assert call(L.br_first_across_owners, ranges) is None
    assert call(L.br_first_in_set, [ranges[0], ranges[2]]) == (1, 0)
    ok = [(BASE, 100, False, 0), (BASE + 10, 40, False, 1), (BASE + 120, 10, True, 0)]     # with the precondition met
    assert call(L.br_first_in_set, [ok[0], ok[2]]) is None and call(L.br_first_across_owners, ok) is None
    hit = [(BASE + 200, 100, False, 0), (BASE + 10, 40, False, 1), (BASE + 20, 10, True, 0)]
    assert call(L.br_first_in_set, [hit[0], hit[2]]) is None and call(L.br_first_across_owners, hit) == (2, 1)


def test_sweep_with_every_range_its_own_owner(L):
    """The form sfm_fuse_chain uses: nothing is exempt, so the call is refused exactly when an output overlaps anything."""
    refused = passed = 0
    for _, raw in random_sets(2000, 3):
        ranges = [r[:3] + (k,) for k, r in enumerate(raw)]
        got = call(L.br_first_across_owners, ranges)
        brute = any(conflict(x, y) for x, y in itertools.combinations(ranges, 2))
        assert (got is not None) == brute, ranges
        if got is not None:
            assert got[0] != got[1] and conflict(ranges[got[0]], ranges[got[1]]), (ranges, got)
        refused += brute; passed += not brute
    assert refused > 300 and passed > 300, (refused, passed)


def test_touching_equal_null_and_empty(L):
    out, inp = (BASE, 16, True, 0), (BASE + 16, 16, False, 1)
    for fn in (L.br_first_in_set, L.br_first_across_owners):
        assert call(fn, [out, inp]) is None                                        # hi == lo of the next: not an overlap
        assert call(fn, [out, (BASE + 15, 16, False, 1)]) is not None
        assert call(fn, [out, (BASE, 1, False, 1)]) is not None                    # equal starts
        assert call(fn, [(0, 16, True, 0), (0, 16, False, 1)]) is None             # null pointers
        assert call(fn, [out, (BASE + 4, 0, False, 1)]) is None                    # an empty range inside another
        assert call(fn, [(BASE, 16, False, 0), (BASE, 16, False, 1)]) is None      # inputs may be shared
    assert call(L.br_first_across_owners, [out, (BASE, 16, True, 0)]) is None      # one owner: not the sweep's business


def test_one_byte_until_the_length_is_known(L):
    for per in (1, 4, 16, 576):
        assert L.br_bytes_until_known(0, per) == 1
        for n in (1, 2, 257, 1 << 20):
            assert L.br_bytes_until_known(n, per) == n * per


def test_job_order(L):
    rng = random.Random(4)
    for count in (1, 2, 257):
        for top in (1, 3, 1000):                                                   # top 1: all keys equal; 3: many ties
            keys = [rng.randrange(top) for _ in range(count)]
            order = (C.c_int * count)()
            L.jo_order((C.c_int * count)(*keys), count, order)
            order = list(order)
            assert sorted(order) == list(range(count))                             # a permutation
            assert all(keys[order[k]] >= keys[order[k + 1]] for k in range(count - 1))               # decreasing in key
            assert all(order[k] < order[k + 1] for k in range(count - 1) if keys[order[k]] == keys[order[k + 1]])     # stable
            assert keys[order[0]] == max(keys)                                     # entry 0 is the largest
            assert order == sorted(range(count), key=lambda i: -keys[i])           # (Python's sort is stable)
