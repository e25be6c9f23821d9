"""CPU: sfm_match_guided_pairs -- the export in the header, EXPORTS, exports.map, INTEGRATION and the library; the refusals that
need no device; the C++ facade (MatchSiftDataGuidedPairs of host/cudaSift.h) and host/guided_pairs_demo.cpp compiled by the plain
host compiler; the resource pin of match_guided_pairs.hip; the documents; and the launch planner (csrc/match_guided_plan.hpp)
through a host-compiled probe (tests/hostcheck/libmatchguidedplancheck.so): its units, splits and workspace on ragged lists, and
its extremes -- a job of 2^31 - 1 queries and a list whose unit total passes 2^31 - 1."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
read = lambda *p: open(os.path.join(ROOT, *p)).read()
NAME = "sfm_match_guided_pairs"
LIBDIR = os.path.join(ROOT, "cuda-sfm_amd", "lib")
IMAX = 2 ** 31 - 1
RECORD = 64                                   # bytes of a device table entry as the tests plan it (any size serves the planner)


# ---- build, surfaces, resources ---------------------------------------------------------------------------------------------------
def test_export_is_declared_listed_and_documented():
    header, integ, exports_map = read("include", "sfm_amd.h"), read("INTEGRATION.md"), read("cuda-sfm_amd", "csrc", "exports.map")
    assert re.search(r"global:\s*sfm_\*;", exports_map)                  # the version script exports every sfm_ name
    assert re.search(r"^int %s\(sfm_ctx \*ctx, const sfm_match_guided_job \*jobs, int num_jobs," % NAME, header, re.M)
    assert re.search(r"typedef struct sfm_match_guided_job \{\s*sfm_sift_point\s*\*d_sift1; int32_t n1;", header)
    assert "#define SFM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", header)
    assert NAME in S.EXPORTS and NAME in integ
    assert hasattr(S.lib(), NAME) and callable(S.match_guided_pairs)
    assert C.sizeof(S.MatchGuidedJob) == 40                              # two (pointer, int32) pairs with their padding, one pointer


def test_refusals_that_need_no_device(tmp_path):
    """a C probe against the library: the prototype is the header's, and a null context, list or parameter block is refused before
    anything else is looked at"""
    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include "sfm_amd.h"', 'int main(void) {',
        '  int (*f)(sfm_ctx *, const sfm_match_guided_job *, int, const sfm_match_guided_params *) = sfm_match_guided_pairs;',
        '  sfm_match_guided_job job = { NULL, 0, NULL, 0, NULL }; sfm_match_guided_params p;',
        '  sfm_match_guided_default_params(&p);',
        '  printf("%d %d %d %d\\n", f(NULL, &job, 1, &p), f(NULL, NULL, 0, &p), f(NULL, &job, 0, NULL), f(NULL, &job, -1, &p));',
        '  return 0;', '}']))
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lsfm_amd", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(S.E_INVALID)] * 4
    assert S.lib().sfm_match_guided_pairs(None, None, 3, None) == S.E_INVALID
    with pytest.raises(S.SfmError) as e:
        S.match_guided_pairs(None, [(None, 0, None, 0, None)])
    assert e.value.code == S.E_INVALID


def test_facade_and_demo_compile(tmp_path):
    """MatchSiftDataGuidedPairs(SiftData *const *, SiftData *const *, const float *, int, float) beside MatchSiftDataGuided, and the
    demo: plain C++ on the facade headers"""
    src = tmp_path / "facade.cpp"
    src.write_text("\n".join([
        '#include "sfm.h"', 'int main(int argc, char **) {',
        '  double (*f)(SiftData *const *, SiftData *const *, const float *, int, float) = MatchSiftDataGuidedPairs;',
        '  return argc > 100 && f(nullptr, nullptr, nullptr, 0, 4.0f) > 0.0 ? 1 : 0;', '}']))
    host = os.path.join(ROOT, "cuda-sfm_amd", "host")
    link = ["-L", LIBDIR, "-lsfm_amd", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", host, str(src), "-o", str(tmp_path / "facade")] + link, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "facade")]).returncode == 0
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", os.path.join(host, "guided_pairs_demo.cpp"), "-o", str(tmp_path / "demo")] + link, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "demo")], capture_output=True, text=True)             # no arguments: the usage line, no device
    assert r.returncode == 2 and "usage" in r.stderr
    assert "guided_pairs_demo" in read("Makefile") and os.path.exists(os.path.join(host, "guided_pairs_demo"))


def test_kernel_resources():
    """build/match_guided_pairs.usage.txt (written next to the object): exactly the two instances, no scratch; match_guided.hip keeps
    exactly its three kernels"""
    path = os.path.join(ROOT, "build", "match_guided_pairs.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it with the library"
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", open(path).read(), re.S):
        found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4, 5))
    print("match_guided_pairs.hip (VGPRs, scratch, waves per SIMD, LDS):", found)
    assert len(found) == 2 and all("match_guided_jobs_kernel" in k for k in found), found
    assert any("ILi4E" in k for k in found) and any("ILi8E" in k for k in found), found
    for vgprs, scratch, waves, lds in found.values():
        assert scratch == 0
        assert waves >= 2 and lds == 69636                # the single kernel's: two LDS stage buffers and the rows' positions
    single = set(re.findall(r"Function Name: (\S+)", read("build", "match_guided.usage.txt")))
    assert len(single) == 3 and not any("jobs" in k for k in single), single


def test_documents():
    design = read("DESIGN.md")
    m = re.search(r"^##+ *6p\b.*?(?=^##+ *7\b|\Z)", design, re.S | re.M)
    assert m, "DESIGN.md has no section 6p"
    sec = m.group(0)
    assert re.search(r"^##+ *6o\b", design, re.M).start() < m.start() < re.search(r"^##+ *7\b", design, re.M).start()
    for word in (NAME, "match_guided_jobs_kernel", "match_guided_plan.hpp", "match_guided_body.inc", "2^31 - 1", "SFM_E_INVALID", "SFM_E_NOMEM", "ticket",
                 "binary search", "Nobody measured", "Expected", "measured", "match_guided_pairs_bench", "Out of scope", "MatchSiftDataGuidedPairs", "guided_pairs_demo"):
        assert word in sec, word
    for name in ("6n", "6o"):
        s = re.search(r"^##+ *%s\b.*?(?=^##+ *(?:6o|6p|7)\b|\Z)" % name, design, re.S | re.M).group(0)
        assert "since built: §6p" in s, name
    readme = read("README.md")
    assert NAME in readme and "guided_pairs_demo" in readme
    assert os.path.exists(os.path.join(ROOT, "profiles", "match_guided_pairs_bench.py"))


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def probe():
    path = os.path.join(ROOT, "tests", "hostcheck", "libmatchguidedplancheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.mgp_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    h.mgp_first_across_owners.argtypes = [C.c_void_p] * 4 + [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h.mgp_largest_allocation.restype = C.c_uint64
    return h


def plan(num_cus, sizes):
    """-> (code, jobs: list of dicts, launches: list of two dicts, totals dict, message, largest allocation in bytes)"""
    h = probe()
    n = len(sizes)
    n1 = np.array([s[0] for s in sizes], np.int32); n2 = np.array([s[1] for s in sizes], np.int32)
    pj = np.zeros((max(n, 1), 8), np.int64); pl = np.zeros((2, 6), np.int64); tot = np.zeros(3, np.uint64)
    what = C.create_string_buffer(256)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    h.mgp_reset_largest_allocation()
    rc = h.mgp_plan(num_cus, vp(n1), vp(n2), n, RECORD, vp(pj), vp(pl), vp(tot), what, 256)
    largest = int(h.mgp_largest_allocation())
    jk = ("launch", "nsplit", "rows_per_split", "qblocks", "first_unit", "slot", "tickets_off", "partials_off")
    lk = ("wv", "jobs", "qblocks", "units", "want", "table_off")
    jobs = [dict(zip(jk, (int(v) for v in pj[k]))) for k in range(n)]
    launches = [dict(zip(lk, (int(v) for v in pl[c]))) for c in range(2)]
    totals = dict(zip(("tickets_off", "tickets_bytes", "workspace_bytes"), (int(v) for v in tot)))
    return rc, jobs, launches, totals, what.value.decode(), largest


def ceil_div(a, b):
    return -(-a // b)


def check_plan(num_cus, sizes):
    """every property the kernel and the merge rely on, computed here in Python integers from the sizes alone"""
    rc, jobs, launches, totals, what, largest = plan(num_cus, sizes)
    assert rc == S.OK, what
    assert largest <= 64 * (len(sizes) + 1)                # the probe's two arrays of num_jobs entries, nothing else
    pieces = []                                            # (begin, end, what) of everything in the workspace
    for c, wv in ((0, 4), (1, 8)):
        mine = [k for k, (n1, n2) in enumerate(sizes) if n1 > 0 and n2 > 0 and (n1 > 4500) == (wv == 8)]
        L = launches[c]
        assert L["wv"] == wv and L["jobs"] == len(mine)
        for k in mine:
            assert jobs[k]["launch"] == c
        if not mine:
            assert L["units"] == 0
            continue
        total_q = sum(ceil_div(sizes[k][0], 32 * wv) for k in mine)
        assert L["qblocks"] == total_q
        want = max(1, ceil_div(2 * num_cus, total_q))      # about two rounds of blocks over the CUs in total
        assert L["want"] == want
        assert sorted(jobs[k]["slot"] for k in mine) == list(range(len(mine)))
        # units: contiguous in the order of the list, each (job, query block, split) once
        at = 0
        for k in mine:
            n1, n2 = sizes[k]
            j = jobs[k]
            assert j["qblocks"] == ceil_div(n1, 32 * wv)
            assert 1 <= j["nsplit"] <= min(want, ceil_div(n2, 64))
            assert j["rows_per_split"] % 32 == 0
            assert j["nsplit"] * j["rows_per_split"] >= n2 > (j["nsplit"] - 1) * j["rows_per_split"]
            # the split count is what the budget gives, rounded as exact_match_plan rounds it
            first = min(want, ceil_div(n2, 64))
            rps = ceil_div(ceil_div(n2, first), 32) * 32
            assert (j["rows_per_split"], j["nsplit"]) == (rps, ceil_div(n2, rps))
            assert j["first_unit"] == at
            units = j["qblocks"] * j["nsplit"]
            if units <= 4096:                              # the kernel's decode: split-major inside the job
                seen = {((u // j["qblocks"]), u % j["qblocks"]) for u in range(units)}
                assert seen == {(s, q) for s in range(j["nsplit"]) for q in range(j["qblocks"])}
            at += units
            # lengths from what the merge indexes: tickets[qblock], three arrays of words indexed split * n1 + p1
            pieces.append((j["tickets_off"], j["tickets_off"] + 4 * j["qblocks"], f"tickets {k}"))
            pieces.append((j["partials_off"], j["partials_off"] + 3 * 4 * ((j["nsplit"] - 1) * n1 + n1), f"partials {k}"))
            assert j["tickets_off"] % 4 == 0 and j["partials_off"] % 4 == 0
            assert totals["tickets_off"] <= j["tickets_off"] and j["tickets_off"] + 4 * j["qblocks"] <= totals["tickets_off"] + totals["tickets_bytes"]
            assert j["partials_off"] >= totals["tickets_off"] + totals["tickets_bytes"]        # no partial where zeroed tickets are expected
        assert L["units"] == at <= IMAX
        pieces.append((L["table_off"], L["table_off"] + RECORD * len(mine), f"table {c}"))
        assert L["table_off"] % 8 == 0 and L["table_off"] + RECORD * len(mine) <= totals["tickets_off"]
    for k, (n1, n2) in enumerate(sizes):
        if n1 == 0 or n2 == 0:
            assert jobs[k]["launch"] == -1
    pieces.sort()
    for (b0, e0, w0), (b1, e1, w1) in zip(pieces, pieces[1:]):
        assert e0 <= b1, (w0, w1)
    assert all(e <= totals["workspace_bytes"] for _, e, _ in pieces)
    return jobs, launches, totals


RAGGED = [(1, 1), (31, 33), (33, 31), (255, 64), (257, 65), (1024, 1025), (0, 64), (64, 0), (4600, 97)]


@pytest.mark.parametrize("num_cus", [1, 64, 256, 304])
def test_plan_of_ragged_lists(num_cus):
    check_plan(num_cus, RAGGED)
    check_plan(num_cus, [(2155, 2170)])
    check_plan(num_cus, [(257, 65)] * 20 + [(2155, 2170)] + [(257, 65)] * 20)
    check_plan(num_cus, [(33 + k, 40 + (k * 37) % 300) for k in range(70)])
    check_plan(num_cus, [(4501 + 700 * k, 1 + 997 * k) for k in range(12)] + [(4500, 4500), (12000, 12000)])
    check_plan(num_cus, [(0, 0), (0, 5)])
    check_plan(num_cus, [])


def test_split_budget_is_shared():
    """alone a 2155 x 2170 job takes many splits, among forty small jobs few: one budget per launch over all its jobs"""
    alone, _, _ = check_plan(256, [(2155, 2170)])
    among, _, _ = check_plan(256, [(257, 65)] * 20 + [(2155, 2170)] + [(257, 65)] * 20)
    assert alone[0]["nsplit"] == 23 and alone[0]["rows_per_split"] == 96        # ceil(512 / 17) = 31 -> 70 rows -> 96 -> 23 splits
    assert among[20]["nsplit"] < alone[0]["nsplit"] // 2
    assert among[20]["nsplit"] == 4 and among[20]["rows_per_split"] == 544      # 17 + 40 x 3 = 137 blocks: ceil(512 / 137) = 4


def test_plan_extremes():
    """the case that aborted in host code before: a job of 2^31 - 1 queries is 2^23 query blocks of (1,8), a plan like any other
    with totals beyond 32 bits; a planner with `int` block counts cannot give these numbers.  A list whose unit total passes
    2^31 - 1 is refused.  Neither allocates anything that scales with n1."""
    jobs, launches, totals = check_plan(256, [(IMAX, 1)])
    assert jobs[0]["qblocks"] == 2 ** 23 and jobs[0]["nsplit"] == 1 and launches[1]["units"] == 2 ** 23
    assert totals["workspace_bytes"] >= 12 * IMAX + 4 * 2 ** 23 > 2 ** 32
    jobs, launches, totals = check_plan(256, [(IMAX, 64), (5, 5), (IMAX, 129)])
    assert launches[1]["qblocks"] == 2 ** 24 and launches[1]["units"] == 2 ** 24 and totals["workspace_bytes"] > 24 * IMAX
    # 255 such jobs still fit a grid, 256 do not
    jobs, launches, totals = check_plan(256, [(IMAX, 1)] * 255)
    assert launches[1]["units"] == 255 * 2 ** 23 and jobs[254]["first_unit"] == 254 * 2 ** 23 == 2 ** 31 - 2 ** 24
    assert totals["workspace_bytes"] > 255 * 12 * IMAX
    rc, _, _, _, what, largest = plan(256, [(IMAX, 1)] * 256)
    assert rc == S.E_INVALID and "units" in what and largest <= 64 * 257
    # the same limit reached through splits (a budget no device gives): 32 query blocks x 2^25 splits are 2^30 units, twice that
    # is one unit too many
    rc, jobs, launches, _, what, largest = plan(IMAX, [(8192, IMAX)])
    assert rc == S.OK and jobs[0]["qblocks"] == 32 and jobs[0]["nsplit"] == 2 ** 25 and launches[1]["units"] == 2 ** 30
    rc, _, _, _, what, largest = plan(IMAX, [(8192, IMAX)] * 2)
    assert rc == S.E_INVALID and "units" in what
    # both sizes at the limit: one split of 2^31 rows does not fit the kernel's 32-bit row counts -- refused, not wrapped
    rc, _, _, _, what, largest = plan(256, [(IMAX, IMAX)])
    assert rc == S.E_INVALID and largest <= 64 * 2


def test_overlap_rule_across_jobs_that_may_overlap_themselves():
    """buffer_ranges.hpp: first_conflict_across_overlapping_owners -- an owner's own overlap is nobody's business and hides nothing"""
    h = probe()

    def first(ranges):
        addr = np.array([r[0] for r in ranges], np.uint64); size = np.array([r[1] for r in ranges], np.uint64)
        out = np.array([r[2] for r in ranges], np.int32); own = np.array([r[3] for r in ranges], np.int32)
        a, b = C.c_int(-1), C.c_int(-1)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        hit = h.mgp_first_across_owners(vp(addr), vp(size), vp(out), vp(own), len(ranges), C.byref(a), C.byref(b))
        return tuple(sorted((a.value, b.value))) if hit else None

    assert first([(1000, 100, 1, 0), (1000, 100, 0, 0), (5000, 36, 0, 0)]) is None                 # a set matched against itself
    assert first([(1000, 100, 1, 0), (2000, 100, 0, 0), (2000, 100, 0, 1), (3000, 100, 1, 1)]) is None     # a shared second view
    assert first([(1000, 100, 1, 0), (1050, 100, 0, 1), (3000, 100, 1, 1)]) == (0, 1)              # d_sift1 inside another's d_sift2
    assert first([(1000, 100, 1, 0), (1000, 100, 1, 1)]) == (0, 1)                                 # one d_sift1 twice
    assert first([(1000, 100, 1, 0), (1096, 36, 0, 1), (3000, 100, 1, 1)]) == (0, 1)               # over another job's F
    assert first([(1000, 100, 1, 0), (1100, 36, 0, 1)]) is None                                    # ranges that only touch
    # owner 0's own input lies in front of owner 1's and reaches further: owner 1's output is still held against owner 0's
    assert first([(4000, 1000, 0, 0), (4010, 50, 0, 1), (4020, 10, 1, 1)]) == (0, 1)
    assert first([(4000, 1000, 0, 0), (4010, 50, 1, 0), (4020, 10, 0, 1)]) == (0, 1)
    assert first([(4000, 1000, 1, 0), (4000, 1000, 0, 0), (4010, 50, 0, 1), (9000, 10, 1, 1)]) == (0, 1)
    rng = np.random.default_rng(5)
    for _ in range(300):                                                                           # against the quadratic rule
        n = int(rng.integers(2, 9))
        ranges = [(int(rng.integers(0, 60)), int(rng.integers(0, 25)), int(rng.integers(0, 2)), int(rng.integers(0, 3))) for _ in range(n)]
        ranges = [(a + 1, s, o, w) for a, s, o, w in ranges]
        want = any(x[3] != y[3] and (x[2] or y[2]) and x[1] and y[1] and x[0] < y[0] + y[1] and y[0] < x[0] + x[1] for x in ranges for y in ranges)
        assert (first(ranges) is not None) == want, ranges
