"""Instruction census of a kernel from its ISA (no GPU needed): compiles one source file for gfx950 with -DSFM_CENSUS -S (the SFM_PHASE
markers of device_math.hpp become comments between scheduling barriers), cuts the named kernel out of the assembly and counts the
instructions per phase and class.

    python profiles/isa_census.py cuda-sfm_amd/csrc/ransac.hip ransac_solve_lanes1_qr [--weighted] [extra hipcc flags...]

The source is compiled with the flags the product build gives it: the Makefile's HIPFLAGS and its per-source FLAGS_<source> (ransac.hip is
built without the SLP vectoriser; a census without that flag shows ~575 packed instructions and ~300 register moves the product does not run).

--weighted: every vector instruction is also priced with the issue cost measured for its encoding (profiles/r05_valu_rate_table.txt, DESIGN
section 4; COST below) and the table gains the issue cycles of a SIMD per wavefront, per phase and in total.  A model of issue time only: no
memory latency, no scalar work, both sides of every branch and one trip of every loop.

Static counts of the instruction TEXT: a loop body counts once, both sides of a branch count.  The kernels censused here are
straight-line per phase (fully unrolled solvers) or have one hot loop whose body is a phase of its own."""
import collections
import re
import subprocess
import sys
import tempfile
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-DOCML_BASIC_ROUNDED_OPERATIONS",
         "-fPIC", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-pass-failed", "--cuda-device-only", "-S", "-DSFM_CENSUS=1", "-I" + os.path.join(ROOT, "include")]


# issue cycles of one wave64 instruction on a SIMD, by encoding (profiles/r05_valu_rate_table.txt)
COST = collections.OrderedDict([("vop12", 2.1), ("fma_f32", 2.5), ("vop3", 4.24), ("trans", 8.0)])


def makefile_flags(src):
    """The per-source flags of the product build: FLAGS_<stem> of the Makefile."""
    stem = os.path.splitext(os.path.basename(src))[0]
    with open(os.path.join(ROOT, "Makefile")) as f:
        for ln in f:
            m = re.match(r"FLAGS_%s\s*:?=\s*(.*)" % re.escape(stem), ln)
            if m:
                return m.group(1).split()
    return []


def cost_class(op):
    """Which row of COST a vector instruction is issued at; None for anything that is not a vector ALU instruction.  The assembler's
    mnemonics carry the encoding: _e32 / _sdwa / _dpp are the VOP1 / VOP2 / VOPC family, _e64 and every mnemonic without a suffix
    (v_lshl_add_u64, v_div_scale_f32, v_pk_*, v_perm_b32, ...) are VOP3 / VOP3P."""
    if not op.startswith("v_") or op.startswith("v_mfma"):
        return None
    if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_f(16|32)", op): return "trans"
    if op.startswith("v_fma_f32"): return "fma_f32"
    if op.endswith(("_e32", "_sdwa", "_dpp")) and "_f64" not in op: return "vop12"
    return "vop3"


def kernel_lines(text, kernel):
    """The instruction text of the named kernel (a substring of its mangled name) out of an assembly listing."""
    start = next(i for i, ln in enumerate(text) if re.match(r"^_Z\w*%s\w*:" % re.escape(kernel), ln))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith("s_endpgm"))
    return text[start + 1:end + 1]


def instructions(lines):
    """(phase, mnemonic) of every instruction; phase = the last ##PHASE marker (census builds), "all" without markers."""
    phase = "prologue"
    for ln in lines:
        t = ln.strip()
        m = re.match(r";\s*##PHASE (\S+)", t)
        if m:
            phase = m.group(1)
            continue
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        yield phase, t.split()[0]


def weighted_cycles(lines):
    """({cost class: count}, issue cycles) of a kernel's instruction text."""
    n = collections.Counter(c for c in (cost_class(op) for _, op in instructions(lines)) if c)
    return n, sum(COST[c] * k for c, k in n.items())


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_pk_"): return "valu_packed"
    if re.match(r"v_(fma|mul|add|sub|mac|fmac|mad)_f64|v_(rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|cvt_f64|cvt_f32_f64|trig_preop|ldexp|frexp)_f64|v_.*_f64", op): return "valu_f64"
    if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_", op): return "valu_trans"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"): return "wait_nop"
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return "branch"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith("global_") or op.startswith("flat_") or op.startswith("buffer_") or op.startswith("scratch_"): return "vmem"
    return "other"


def main():
    args = sys.argv[1:]
    weighted = "--weighted" in args
    args = [a for a in args if a != "--weighted"]
    src, kernel = args[0], args[1]
    extra = makefile_flags(src) + args[2:]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + ["-o", out, os.path.join(ROOT, src)], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read().splitlines()
    counts = collections.OrderedDict()
    costs = collections.OrderedDict()
    for phase, op in instructions(kernel_lines(text, kernel)):
        counts.setdefault(phase, collections.Counter())[classify(op)] += 1
        if cost_class(op):
            costs.setdefault(phase, collections.Counter())[cost_class(op)] += 1
    classes = ["valu", "valu_packed", "valu_f64", "valu_trans", "mfma", "salu", "branch", "wait_nop", "lds", "vmem", "other"]
    print(f"# {kernel} ({src}{' ' + ' '.join(extra) if extra else ''}): static instruction counts per phase")
    print("%-16s" % "phase" + "".join("%12s" % c for c in classes) + "%12s" % "all_valu")
    tot = collections.Counter()
    for ph, c in counts.items():
        allv = c["valu"] + c["valu_packed"] + c["valu_f64"] + c["valu_trans"] + c["mfma"]
        print("%-16s" % ph + "".join("%12d" % c[k] for k in classes) + "%12d" % allv)
        tot.update(c)
    allv = tot["valu"] + tot["valu_packed"] + tot["valu_f64"] + tot["valu_trans"] + tot["mfma"]
    print("%-16s" % "TOTAL" + "".join("%12d" % tot[k] for k in classes) + "%12d" % allv)
    if weighted:
        print(f"# issue cycles of a SIMD per wavefront, vector instructions priced by encoding: " + ", ".join(f"{k} {v}" for k, v in COST.items()))
        print("%-16s" % "phase" + "".join("%12s" % c for c in COST) + "%14s" % "issue_cycles")
        wtot = collections.Counter()
        for ph in counts:
            c = costs.get(ph, collections.Counter())
            print("%-16s" % ph + "".join("%12d" % c[k] for k in COST) + "%14.0f" % sum(COST[k] * c[k] for k in COST))
            wtot.update(c)
        print("%-16s" % "TOTAL" + "".join("%12d" % wtot[k] for k in COST) + "%14.0f" % sum(COST[k] * wtot[k] for k in COST))


if __name__ == "__main__":
    main()
