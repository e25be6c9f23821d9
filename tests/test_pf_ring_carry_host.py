"""The survivor ring carried across the two scans of a paired pass (csrc/ransac_prefilter.hip): an entry's tag says in bit 3 which scan
wrote it, and the flush decides the entry on its own row of the pair's 64-row table (prefilter_math.hpp: pf_ring_row) instead of on the
row of whichever scan is in progress.  Host-compiled (tests/hostcheck/pfringcheck.hip): the row for every bit position, half and scan,
the address part of the tag, and the validity test against the (hoff, nvalid) form it replaces."""
import ctypes as C
import functools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDRESSES = (0, 16, 0x4000, 0x4000 + 31 * 16, 0xFFF0)      # LDS byte addresses of a point: multiples of 16
PPS = (0, 1, 15)                                           # two-step indices: 1024 points are 16 of them


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpfringcheck.so"))
    L.pfring_pack_code.restype = C.c_uint
    L.pfring_tag.restype = C.c_uint
    L.pfring_tag.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int]
    L.pfring_tag_address.restype = C.c_uint
    L.pfring_tag_address.argtypes = [C.c_uint]
    L.pfring_row.argtypes = [C.c_int, C.c_uint]
    L.pfring_lut_row_step.argtypes = [C.c_int, C.c_uint]
    L.pfring_admits.argtypes = [C.c_int, C.c_uint, C.c_int]
    L.pfring_admits_scanwise.argtypes = [C.c_int, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def test_row_of_every_bit_half_and_scan():
    L = lib()
    rows = set()
    for b in range(32):
        for half in (0, 1):
            for scan in (0, 1):
                for addr in ADDRESSES:
                    for pp in PPS:
                        tag = L.pfring_tag(addr, half, pp, scan)
                        want = (L.pfring_pack_code(b) & 31) + 4 * half + 32 * scan
                        assert L.pfring_row(b, tag) == want, (b, half, scan, addr, pp)
                        # the table the flush reads: the same row, and pf_pack_code's step
                        assert L.pfring_lut_row_step(b, tag) == want | ((L.pfring_pack_code(b) >> 5) << 8), (b, half, scan, addr, pp)
                rows.add(want)
    # the 16 accumulators of a lane half x 2 halves x 2 scans cover the 64 rows of the pair's table (the two steps of an accumulator share a row)
    assert rows == set(range(64))


def test_the_scan_bit_leaves_the_address_alone():
    L = lib()
    for addr in ADDRESSES:
        for half in (0, 1):
            for pp in PPS:
                t0, t1 = L.pfring_tag(addr, half, pp, 0), L.pfring_tag(addr, half, pp, 1)
                assert t1 == t0 | 8 and t0 & 8 == 0
                assert L.pfring_tag_address(t0) == L.pfring_tag_address(t1) == addr + (pp << 10)
                assert t0 & 4 == t1 & 4 == 4 * half


@pytest.mark.parametrize("nvalid_unit", [1, 31, 32, 33, 63, 64])
def test_admits_the_rows_the_scanwise_test_admitted(nvalid_unit):
    L = lib()
    nscan = 2 if nvalid_unit > 32 else 1
    admitted = set()
    for scan in range(nscan):
        for b in range(32):
            for half in (0, 1):
                tag = L.pfring_tag(0x4000, half, 3, scan)
                row = C.c_int(-1)
                old = L.pfring_admits_scanwise(b, tag, nvalid_unit, scan, C.byref(row))
                assert L.pfring_admits(b, tag, nvalid_unit) == old, (b, half, scan)
                assert L.pfring_row(b, tag) == row.value
                if old:
                    admitted.add(row.value)
    assert admitted == set(range(nvalid_unit))
