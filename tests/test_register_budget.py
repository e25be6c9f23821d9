"""The register budget the pre-filter scoring kernel and the lane-solve kernel share.

Pipelined calls (sfm_estimate_E_pipelined) put the NEXT call's lane-solve kernel on the chip while THIS call's scoring kernel holds every
CU with one block of 16 wavefronts, 4 per SIMD.  A solve wavefront can only be placed on a SIMD if four scoring wavefronts leave its
registers free: 4 x scoring + solve <= 512 vector registers, each allocation rounded up to the granule of 8.  A dozen registers more in
either kernel and the solve waits for scoring blocks to retire again -- nothing fails, the step is just 17 % slower.  This test reads
what the normal build made (the compiler's resource-usage report the Makefile leaves next to the objects, build/<source>.usage.txt, and
the host-compiled LDS map of tests/hostcheck) and holds both kernels to the budget."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = {src: os.path.join(ROOT, "build", src + ".usage.txt") for src in ("ransac", "ransac_prefilter")}
LDSCHECK = os.path.join(ROOT, "tests", "hostcheck", "libpfldscheck.so")

SIMD_VGPRS = 512            # unified vector / accumulation register file of a gfx950 SIMD, per lane
VGPR_GRANULE = 8            # allocation granule (the occupancy the compiler reports follows it: 96 -> 5, 104 -> 4)
CU_LDS = 160 * 1024
SCORING_WAVES_PER_SIMD = 4  # one block of 16 wavefronts per CU

# the product's four kernels, by their mangled names: (W = 16, VAR = 0, RULE, 0, 0, 0, 0) with RULE 3 = per tile, 2 = per hypothesis
# (prefilter_record.hpp: kPfRuleBandTile, kPfRuleBandPack)
SCORE_TILE = "ransac_score_prefilterILi16ELi0ELi3ELi0ELi0ELi0ELi0EE"
SCORE_REC = "ransac_score_prefilterILi16ELi0ELi2ELi0ELi0ELi0ELi0EE"
SOLVE_TILE = "22ransac_solve_lanes1_qrE"
SOLVE_REC = "26ransac_solve_lanes1_qr_recE"
PAIRINGS = [(SCORE_TILE, SOLVE_TILE), (SCORE_REC, SOLVE_REC)]

FIELDS = {"vgprs": r"\bVGPRs: (\d+)", "agprs": r"\bAGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
          "lds": r"LDS Size \[bytes/block\]: (\d+)", "spill": r"VGPRs Spill: (\d+)"}


def read_usage(path):
    """{mangled kernel name: {field: value}} out of a -Rpass-analysis=kernel-resource-usage report."""
    assert os.path.exists(path), f"{path} is missing: the build (make) writes it next to the objects"
    kernels, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = kernels.setdefault(m.group(1), {})
                continue
            if cur is None or "remark:" not in line:
                continue
            for name, pat in FIELDS.items():
                m = re.search(pat, line)
                if m:
                    cur[name] = int(m.group(1))
    return kernels


@pytest.fixture(scope="module")
def usage():
    kernels = {}
    for path in USAGE.values():
        kernels.update(read_usage(path))
    found = {}
    for want in (SCORE_TILE, SCORE_REC, SOLVE_TILE, SOLVE_REC):
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels of that name in the resource-usage reports"
        u = kernels[hits[0]]
        assert set(FIELDS) <= set(u), f"{want}: the report lacks {set(FIELDS) - set(u)}"
        found[want] = u
    return found


def allocated(u):
    """Registers a wavefront of the kernel takes from the SIMD's file: accumulation registers start at the next multiple of 4 behind
    the vector registers (none are used today), the sum is rounded up to the granule."""
    total = u["vgprs"] if u["agprs"] == 0 else (u["vgprs"] + 3) // 4 * 4 + u["agprs"]
    return (total + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE


@pytest.mark.parametrize("name", [SCORE_TILE, SCORE_REC, SOLVE_TILE, SOLVE_REC])
def test_no_scratch(usage, name):
    u = usage[name]
    print(name, u)
    assert u["scratch"] == 0 and u["spill"] == 0, f"{name} spills: {u}"


@pytest.mark.parametrize("score,solve", PAIRINGS)
def test_four_scoring_wavefronts_leave_room_for_a_solve_wavefront(usage, score, solve):
    a_score, a_solve = allocated(usage[score]), allocated(usage[solve])
    print(f"{score}: {usage[score]['vgprs']} -> {a_score}; {solve}: {usage[solve]['vgprs']} -> {a_solve}; "
          f"{SCORING_WAVES_PER_SIMD} x {a_score} + {a_solve} = {SCORING_WAVES_PER_SIMD * a_score + a_solve} of {SIMD_VGPRS}")
    assert SCORING_WAVES_PER_SIMD * a_score + a_solve <= SIMD_VGPRS
    assert usage[solve]["lds"] == 0                     # nothing else a resident scoring block could deny it


def test_scoring_block_keeps_a_cu_to_itself(usage):
    """The budget counts 4 scoring wavefronts per SIMD: one block per CU.  The block's LDS is dynamic (the code object says 0), its size
    comes from the header the launcher uses; for small tiles two blocks would fit the LDS, and then the registers keep it at one."""
    assert os.path.exists(LDSCHECK), f"{LDSCHECK} is missing: make hostcheck builds it"
    lib = C.CDLL(LDSCHECK)
    waves = lib.pfcheck_block_waves()
    assert waves == 4 * SCORING_WAVES_PER_SIMD
    for name in (SCORE_TILE, SCORE_REC):
        assert usage[name]["lds"] == 0                  # no static LDS on top of the dynamic map
        by_regs = (SIMD_VGPRS // allocated(usage[name])) * 4 // waves
        for n in (1100, 2100, 4096, 16384, 70000):      # 2, 3, 4, 16, 69 tiles
            tile = lib.pfcheck_tile_points(n)
            lds = lib.pfcheck_lds_bytes(tile)
            print(f"{name}: {n} points -> tiles of {tile}: {lds} bytes of LDS; blocks per CU: {CU_LDS // lds} by LDS, {by_regs} by registers")
            assert 0 < lds <= CU_LDS
            assert min(CU_LDS // lds, by_regs) == 1
    # the bench geometry (tiles of 1024 points) is held to one block by the LDS alone
    assert CU_LDS // lib.pfcheck_lds_bytes(lib.pfcheck_tile_points(4096)) == 1
