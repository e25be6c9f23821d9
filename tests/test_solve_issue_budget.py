"""The issue budget of the two lane-solve kernels the product runs (ransac_solve_lanes1_qr, ransac_solve_lanes1_qr_rec), read from the
instruction text the normal build leaves (build/ransac.s: ransac.hip compiled with the object's flags, assembly out).

The kernels are bound by vector issue, so what they may cost is held as a number: every vector instruction priced
with the issue cost measured for its encoding (profiles/isa_census.py --weighted: VOP1/VOP2 2.1 cycles, v_fma_f32 2.5, other VOP3 /
VOP3P 4.24, reciprocal / square root 8), summed over the kernel's text -- both sides of every branch, one trip of every loop.  The
budget is this build's own total plus 2 %, so that a later edit cannot grow the kernels without saying so.

Two things the build must not bring back:
  * packed fp32 instructions (the SLP vectoriser's v_pk_mul / v_pk_add / v_pk_fma / v_pk_mov pairs cost two plain instructions' issue time
    and a register move per operand; ransac.hip is built without it),
  * a 64-bit vector address add in front of the accesses of the product's path.  What remains is listed in ADD64_ALLOWED."""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "build", "ransac.s")

#            kernel (mangled-name fragment): issue cycles of a SIMD per wavefront allowed = (this build's census) x 1.02
# The figures are those of build/ransac.s, the text this test prices (the -DSFM_CENSUS build of profiles/r08_solve_census.txt, which adds
# phase markers, gives the same totals for this tree).  The parent's text priced the same way: 9213 / 10079.
BUDGET = {"22ransac_solve_lanes1_qrE": 9137 * 1.02, "26ransac_solve_lanes1_qr_recE": 10000 * 1.02}

# v_lshl_add_u64 left in each kernel, none of them on the path of a fillXU pair of up to 2^28 points (the bench's path):
#    48  the scattered-word gather of generic-z points (sfm_set_points: no 16-byte records): three row bases per view, the compiler keeps a
#        64-bit address per lane for them; the parent's source, unchanged
#     8  the 16-byte gathers of point sets beyond 2^28 points, where idx * 16 leaves 32 bits (no test reaches that size)
#     1  the loop that clears the scoring kernel's accumulators (its word index runs to 2 x hypotheses, and the library sets no limit on
#        the hypotheses of a call: a 32-bit byte offset would wrap at 2^29)
#     1  the tuple table of the reference-mode sampler (explicit indices)
#     2  the probe loops of the cell table (taken by the ~0.5 % of hypotheses whose zero-divisor cells must be looked up; the table of a
#        pair beyond 2^27 points is larger than a 32-bit byte offset reaches)
ADD64_ALLOWED = 48 + 8 + 1 + 1 + 2


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "profiles", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.exists(ASM), f"{ASM} is missing: the build (make) writes it"
    with open(ASM) as f:
        text = f.read().splitlines()
    return mod, text


@pytest.mark.parametrize("kernel", list(BUDGET))
def test_issue_cycles_within_budget(census, kernel):
    mod, text = census
    counts, cycles = mod.weighted_cycles(mod.kernel_lines(text, kernel))
    print(kernel, dict(counts), f"{cycles:.0f} issue cycles, budget {BUDGET[kernel]:.0f}")
    assert cycles <= BUDGET[kernel]


@pytest.mark.parametrize("kernel", list(BUDGET))
def test_no_packed_fp32_and_no_address_adds_beyond_the_listed(census, kernel):
    mod, text = census
    ops = collections.Counter(op for _, op in mod.instructions(mod.kernel_lines(text, kernel)))
    packed = {op: k for op, k in ops.items() if op.startswith("v_pk_") and (op.endswith("_f32") or op == "v_pk_mov_b32")}
    assert not packed, f"packed fp32 instructions are back: {packed}"
    print(kernel, "v_lshl_add_u64:", ops["v_lshl_add_u64"], "of", ADD64_ALLOWED, "; 16-byte loads:", ops["global_load_dwordx4"])
    assert ops["v_lshl_add_u64"] <= ADD64_ALLOWED
    # the sample's eight 16-byte records arrive as eight 16-byte loads in both addressing forms (+ the two loads of the tuple table)
    assert ops["global_load_dwordx4"] >= 2 * 8 + 2
