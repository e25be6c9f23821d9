"""CPU: sfm_register_views (a view registered to each of many pairs in one batched call) as far as it goes without a GPU -- the
header declares it, the library exports it, every argument check that needs no device answers before the first device call,
and the compiler's resource report of the normal build holds the four batched kernels to their single-pair twins."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

import cuda_sfm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "build", "register.usage.txt")

SIMD_VGPRS = 512            # register file of a gfx950 SIMD, per lane
VGPR_GRANULE = 8            # allocation granule
# (batched kernel, its single-pair twin), by the tail of the mangled name
TWINS = [("register_gate_views_kernelEPKNS_12RegisterArgsE", "register_gate_kernelENS_12RegisterArgsE"),
         ("register_solve_views_kernelEPKNS_12RegisterArgsE", "register_solve_kernelENS_12RegisterArgsE"),
         ("register_score_views_kernelEPKNS_12RegisterArgsE", "register_score_kernelENS_12RegisterArgsE"),
         ("register_refine_views_kernelEPKNS_12RegisterArgsE", "register_refine_kernelENS_12RegisterArgsE")]


@pytest.fixture(scope="module")
def fn():
    f = S.lib().sfm_register_views
    f.restype = C.c_int
    return f


def test_declared_exported_and_wrapped():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sfm_register_views\s*\(\s*sfm_pair\s*\*\s*const\s*\*\s*pairs\s*,\s*int\s+num_pairs\s*,"
                     r"\s*const\s+sfm_sift_point\s*\*\s*const\s*\*\s*d_sifts\s*,\s*const\s+sfm_register_params\s*\*\s*p\s*,"
                     r"\s*const\s+float\s*\*\s*const\s*\*\s*d_points\s*,\s*const\s+uint8_t\s*\*\s*const\s*\*\s*d_valid\s*\)\s*;", txt)
    assert re.search(r"#define\s+SFM_ABI_VERSION\s+3\b", txt)
    assert hasattr(S.lib(), "sfm_register_views") and "sfm_register_views" in S.EXPORTS
    assert callable(S.register_views) and callable(S.register_views_enqueue)
    assert "sfm_register_views" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the dynamic symbol table has it, and the version script's global patterns cover it
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "sfm_register_views" in [line.split()[-1] for line in nm.splitlines() if line.strip()]
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "cuda-sfm_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = [g.strip() for g in re.search(r"global\s*:(.*?)local\s*:", script, flags=re.S).group(1).split(";") if g.strip()]
    assert any(fnmatch.fnmatchcase("sfm_register_views", g) for g in globs), globs


def test_argument_checks_come_before_any_device_call(fn):
    p = S.register_params()
    ref = C.byref
    fake = (C.c_void_p * 1)(0x1000)                      # never dereferenced: the checks that reject the call come first
    null = (C.c_void_p * 1)(None)
    assert fn(fake, 1, fake, None, None, None) == S.E_INVALID                    # null p
    assert fn(fake, -1, fake, ref(p), None, None) == S.E_INVALID
    assert fn(fake, 65536, fake, ref(p), None, None) == S.E_INVALID
    assert fn(None, 1, fake, ref(p), None, None) == S.E_INVALID                  # null lists
    assert fn(fake, 1, None, ref(p), None, None) == S.E_INVALID
    assert fn(null, 1, fake, ref(p), None, None) == S.E_INVALID                  # null entries
    assert fn(fake, 1, null, ref(p), None, None) == S.E_INVALID
    assert fn(fake, 1, fake, ref(S.register_params(points=0x1000)), None, None) == S.E_INVALID      # p->d_points set
    assert fn(fake, 1, fake, ref(S.register_params(valid=0x1000)), None, None) == S.E_INVALID
    assert fn(fake, 1, fake, ref(p), None, fake) == S.E_INVALID                  # d_valid without d_points
    assert fn(fake, 1, fake, ref(p), null, fake) == S.E_INVALID                  # ... without that pair's entry
    for kw in (dict(num_hypotheses=0), dict(num_hypotheses=(1 << 20) + 1), dict(threshold_px=0.0), dict(min_score=float("nan")),
               dict(max_iterations=201), dict(reserved=[0, 1, 0, 0])):
        assert fn(fake, 1, fake, ref(S.register_params(**kw)), None, None) == S.E_INVALID, kw
    assert S.lib().sfm_last_error()


def test_an_empty_list_is_not_an_error(fn):
    p = S.register_params()
    fake = (C.c_void_p * 1)(0x1000)
    assert fn(None, 0, None, C.byref(p), None, None) == S.OK
    assert fn(fake, 0, fake, C.byref(p), fake, fake) == S.OK
    assert fn(None, 0, None, None, None, None) == S.E_INVALID                    # the parameters are checked whatever the count
    assert fn(None, 0, None, C.byref(S.register_params(num_hypotheses=0)), None, None) == S.E_INVALID
    S.register_views_enqueue([], [], p)
    assert S.register_views([], []) == []


def kernel_usage():
    """{mangled kernel name: {field: value}} of build/register.usage.txt (-Rpass-analysis=kernel-resource-usage)."""
    assert os.path.exists(USAGE), "run `make`: the product build leaves the compiler's resource report next to the objects"
    out, cur = {}, None
    for line in open(USAGE):
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def waves_per_simd(vgprs):
    return min(8, SIMD_VGPRS // ((vgprs + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE))


def test_batched_kernels_keep_their_twins_resources():
    usage = kernel_usage()

    def find(tail):
        hits = [v for k, v in usage.items() if k.endswith(tail)]
        assert len(hits) == 1, (tail, sorted(usage))
        return hits[0]

    for batched, single in TWINS:
        b, s = find(batched), find(single)
        print(f"{batched}: {b['VGPRs']} VGPRs, scratch {b['ScratchSize']}; {single}: {s['VGPRs']} VGPRs")
        assert b["ScratchSize"] == 0 and s["ScratchSize"] == 0, (batched, b, s)
        assert waves_per_simd(b["VGPRs"]) >= waves_per_simd(s["VGPRs"]), (batched, b["VGPRs"], s["VGPRs"])
    assert waves_per_simd(30) == 8 and waves_per_simd(100) == 4 and waves_per_simd(186) == 2     # the rule itself
