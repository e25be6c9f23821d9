"""CPU: sfm_pair_fundamentals -- the export in the header, EXPORTS, INTEGRATION and the library; its refusals that need no device;
the C++ facade (SfM::fundamentals of host/sfm.h) compiled and linked by the plain host compiler; the resource pin of
pair_fundamentals.hip; the documents."""
import ctypes as C
import os
import re
import subprocess

import cuda_sfm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
read = lambda *p: open(os.path.join(ROOT, *p)).read()
NAME = "sfm_pair_fundamentals"


def test_export_is_declared_listed_and_documented():
    header, integ, exports_map = read("include", "sfm_amd.h"), read("INTEGRATION.md"), read("cuda-sfm_amd", "csrc", "exports.map")
    assert re.search(r"global:\s*sfm_\*;", exports_map)                  # the version script exports every sfm_ name
    assert re.search(r"^int %s\(sfm_pair \*const \*pairs, int num_pairs, int refined," % NAME, header, re.M)
    assert "#define SFM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", header)
    assert NAME in S.EXPORTS and NAME in integ
    assert hasattr(S.lib(), NAME) and callable(S.pair_fundamentals)


def test_refusals_that_need_no_device(tmp_path):
    """a C probe against the library: the prototype is the header's, and null arguments, a negative count and a bad `refined` are
    refused before any pair is looked at"""
    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include "sfm_amd.h"', 'int main(void) {',
        '  int (*f)(sfm_pair *const *, int, int, float *) = sfm_pair_fundamentals;',
        '  sfm_pair *none[1] = { NULL }; float out[9];',
        '  printf("%d %d %d %d %d %d\\n", f(NULL, 0, 1, out), f(none, 0, 1, NULL), f(none, -1, 0, out), f(none, 1, 2, out), f(none, 1, 0, out), f(none, 0, 0, out));',
        '  return 0;', '}']))
    exe = tmp_path / "probe"
    libdir = os.path.join(ROOT, "cuda-sfm_amd", "lib")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsfm_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    inv = str(S.E_INVALID)
    assert out == [inv, inv, inv, inv, inv, str(S.OK)]                   # (the last: no pair is a no-op)
    assert S.lib().sfm_pair_fundamentals(None, 3, 0, None) == S.E_INVALID


def test_facade_compiles_and_links(tmp_path):
    """SfM::fundamentals(Image_pair *const *, int, bool) beside SfM::refine_pairs: plain C++ on the facade headers"""
    src = tmp_path / "facade.cpp"
    src.write_text("\n".join([
        '#include "sfm.h"', 'int main(int argc, char **) {',
        '  std::shared_ptr<float> (*f)(SfM::Image_pair *const *, int, bool) = SfM::fundamentals;',
        '  return argc > 100 && f(nullptr, 0, true).get() ? 1 : 0;', '}']))
    libdir = os.path.join(ROOT, "cuda-sfm_amd", "lib")
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cuda-sfm_amd", "host"), str(src), "-o", str(tmp_path / "facade"),
                        "-L", libdir, "-lsfm_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "facade")]).returncode == 0


def test_kernel_resources():
    """build/pair_fundamentals.usage.txt (written next to the object): one kernel, no scratch, no LDS; match_guided.hip keeps
    exactly its three kernels"""
    path = os.path.join(ROOT, "build", "pair_fundamentals.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it with the library"
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", open(path).read(), re.S):
        found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    print("pair_fundamentals.hip (VGPRs, scratch, LDS):", found)
    assert len(found) == 1 and "pair_fundamentals_kernel" in next(iter(found))
    vgprs, scratch, lds = next(iter(found.values()))
    assert scratch == 0 and lds == 0 and vgprs <= 128
    single = set(re.findall(r"Function Name: (\S+)", read("build", "match_guided.usage.txt")))
    assert len(single) == 3 and not any("fundamentals" in k for k in single), single


def test_documents():
    design = read("DESIGN.md")
    m = re.search(r"^##+ *6o\b.*?(?=^##+ *7\b|\Z)", design, re.S | re.M)
    assert m, "DESIGN.md has no section 6o"
    sec = m.group(0)
    assert m.start() > re.search(r"^##+ *6n\b", design, re.M).start()
    for word in (NAME, "pair_fundamentals_kernel", "guided_fundamental", "bit-equal", "JobArray", "SFM_E_STATE", "Expected", "measured",
                 "pair_fundamentals_bench", "Out of scope", "sfm_match_guided_pairs"):
        assert word in sec, word
    n = re.search(r"^##+ *6n\b.*?(?=^##+ *(?:6o|7)\b|\Z)", design, re.S | re.M).group(0)
    for word in ("sfm_match_guided", "sfm_pair_fundamental", "band", "ticket", "scratch", "Out of scope", "tiles", "pre-filter", "_soa", "batched",
                 "chain stages", "16384"):
        assert word in n, word
    assert NAME in read("README.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "pair_fundamentals_bench.txt"))
