"""The register budget of tests/test_register_budget.py for the per-tile rule's two summing instances since the passes are paired:
ransac_score_prefilter<16, 0, 3> prepares two passes at once and keeps the second scan's fragments -- eight registers -- across the
first scan: 104 allocated at most (4 x 104 + 88 = 504 of 512), no accumulation registers, no scratch, no spill, no static LDS.
ransac_score_prefilter<16, 64, 3> (kPfVarSinglePass: launches between 2^21 and 2^22 partial counts) is the single-pass kernel and
stays at 96.  Both share a SIMD with the next call's lane-solve kernel."""
import pytest

from test_register_budget import USAGE, FIELDS, SIMD_VGPRS, SCORING_WAVES_PER_SIMD, SCORE_TILE, SOLVE_TILE, read_usage, allocated

SCORE_TILE_SINGLE = "ransac_score_prefilterILi16ELi64ELi3ELi0ELi0ELi0ELi0EE"


@pytest.fixture(scope="module")
def usage():
    kernels = {}
    for path in USAGE.values():
        kernels.update(read_usage(path))
    found = {}
    for want in (SCORE_TILE, SCORE_TILE_SINGLE, SOLVE_TILE):
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels of that name in the resource-usage reports"
        assert set(FIELDS) <= set(kernels[hits[0]]), f"{want}: the report lacks {set(FIELDS) - set(kernels[hits[0]])}"
        found[want] = kernels[hits[0]]
    return found


@pytest.mark.parametrize("score,cap", [(SCORE_TILE, 104), (SCORE_TILE_SINGLE, 96)])
def test_paired_and_single_pass_instances_keep_the_budget(usage, score, cap):
    u = usage[score]
    print(score, u)
    assert u["scratch"] == 0 and u["spill"] == 0 and u["agprs"] == 0 and u["lds"] == 0, f"{score}: {u}"
    assert u["vgprs"] <= cap
    assert SCORING_WAVES_PER_SIMD * allocated(u) + allocated(usage[SOLVE_TILE]) <= SIMD_VGPRS
