"""Per-kernel hashes of a source's device instruction text, to show which instances a change left alone.
python profiles/kernel_text_hashes.py SOURCE [NAME_FILTER]: compiles SOURCE (a path relative to the tree this script sits in) with the
Makefile's flags, --cuda-device-only -S, from the tree's root, and prints "sha256[:16] instruction-lines mangled-name" for every kernel
whose mangled name contains NAME_FILTER.  Run it in two trees and compare the lines (profiles/r12_kernel_text_hashes.txt).  Only the
lines between a kernel's label and the end of its function are hashed, with comments and local label numbers dropped."""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1]
want = sys.argv[2] if len(sys.argv) > 2 else ""
flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-DOCML_BASIC_ROUNDED_OPERATIONS",
         "-fPIC", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-pass-failed", "--cuda-device-only", "-S"]
text = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + [src, "-o", "-"], cwd=ROOT, check=True, capture_output=True, text=True).stdout
name, body = None, []
for line in text.splitlines():
    m = re.match(r"^(_Z\w+):", line)
    if m and name is None:
        name, body = m.group(1), []
        continue
    if name is None:
        continue
    code = line.split(";")[0].strip()
    if code and not code.startswith("."):
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    if code.startswith(".Lfunc_end"):
        if want in name:
            print(hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body), name)
        name = None
