"""The register budget of tests/test_register_budget.py for the product's OTHER two scoring instances: launches below 2^21 partial
counts (a rank's share, configs[2]) run ransac_score_prefilter<16, 8, rule> -- the returning-atomic epilogue -- and share a SIMD with
the next call's lane-solve kernel exactly as the <16, 0, rule> instances do: 96 vector registers at most, no accumulation
registers, no scratch, no spill, no static LDS."""
import pytest

from test_register_budget import USAGE, FIELDS, SIMD_VGPRS, SCORING_WAVES_PER_SIMD, SOLVE_TILE, SOLVE_REC, read_usage, allocated

SCORE_TILE_ANSWER = "ransac_score_prefilterILi16ELi8ELi3ELi0ELi0ELi0ELi0EE"
SCORE_REC_ANSWER = "ransac_score_prefilterILi16ELi8ELi2ELi0ELi0ELi0ELi0EE"


@pytest.fixture(scope="module")
def usage():
    kernels = {}
    for path in USAGE.values():
        kernels.update(read_usage(path))
    found = {}
    for want in (SCORE_TILE_ANSWER, SCORE_REC_ANSWER, SOLVE_TILE, SOLVE_REC):
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels of that name in the resource-usage reports"
        assert set(FIELDS) <= set(kernels[hits[0]]), f"{want}: the report lacks {set(FIELDS) - set(kernels[hits[0]])}"
        found[want] = kernels[hits[0]]
    return found


@pytest.mark.parametrize("score,solve", [(SCORE_TILE_ANSWER, SOLVE_TILE), (SCORE_REC_ANSWER, SOLVE_REC)])
def test_answer_epilogue_instances_keep_the_budget(usage, score, solve):
    u = usage[score]
    print(score, u)
    assert u["scratch"] == 0 and u["spill"] == 0 and u["agprs"] == 0 and u["lds"] == 0, f"{score}: {u}"
    assert u["vgprs"] <= 96
    assert SCORING_WAVES_PER_SIMD * allocated(u) + allocated(usage[solve]) <= SIMD_VGPRS
