"""CPU: the pair's stage bookkeeping (csrc/pair_state.hpp, host-compiled into tests/hostcheck/libpairstatecheck.so) -- every
transition from every one of the 128 combinations of stages against a model of DESIGN 6d's first table written here with sets of
names, the needs of the second table, the SFM_E_STATE texts, and that no other source file assigns a stage."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-sfm_amd", "csrc")
STAGES = ("points", "E", "P", "pose", "points3d", "refined", "view")
TRANSITIONS = {"reset": 0, "points_filled": 1, "points_set": 2, "E_finalized": 3, "candidates_done": 4, "pose_chosen": 5,
               "triangulated": 6, "chain_done": 7, "refined": 8, "view_registered": 9, "view_dropped": 10, "failed_call": 11}


@pytest.fixture(scope="module")
def L():
    h = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpairstatecheck.so"))
    h.ps_apply.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    h.ps_has.argtypes = h.ps_missing.argtypes = [C.c_uint32, C.c_uint32]
    h.ps_missing.restype = h.ps_fresh.restype = h.ps_stage.restype = C.c_uint32
    h.ps_stage.argtypes = [C.c_int]
    h.ps_hint.argtypes = [C.c_uint32]; h.ps_hint.restype = C.c_char_p
    return h


def bits_of(L, names):
    return sum(L.ps_stage(STAGES.index(s)) for s in names)


def model(transition, arg, have, flags):
    """DESIGN 6d, first table: (stages, flags) after the call.  have: set of names; flags: dict of the five point-derived fields."""
    have, f = set(have), dict(flags)
    if transition == "reset":                       # clears all seven; of the flags only last_count
        have = set(); f["last_count"] = 0
    elif transition == "points_filled":             # sfm_fill_xu
        have = {"points"}
        f.update(last_count=0, key_clean=1, unit_z=arg, have_pts4=arg, have_bound=1)
    elif transition == "points_set":                # sfm_set_points: key_clean untouched
        have = {"points"}
        f.update(last_count=0, unit_z=0, have_pts4=0, have_bound=0)
    elif transition == "E_finalized":               # refined and view are NOT cleared
        have = (have - {"P", "pose", "points3d"}) | {"E"}
    elif transition == "candidates_done":
        have = (have - {"pose", "points3d"}) | {"P"}
    elif transition == "pose_chosen":
        have = (have - {"points3d"}) | {"pose"}
    elif transition == "triangulated":
        have = have | {"points3d"}
    elif transition == "chain_done":
        have = have | {"P", "pose", "points3d"}
    elif transition == "refined":
        have = have | {"refined"}
    elif transition == "view_registered":
        have = have | {"view"}
    elif transition == "view_dropped":
        have = have - {"view"}
    else:
        assert transition == "failed_call"         # nothing changes
    return have, f


FLAG_NAMES = ("unit_z", "have_pts4", "have_bound", "key_clean", "last_count")
FLAG_CASES = [dict(zip(FLAG_NAMES, v)) for v in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 4096), (0, 0, 1, 0, 7), (1, 0, 0, 1, 1), (0, 1, 0, 0, 2 ** 20))]


@pytest.mark.parametrize("transition,arg", [(t, a) for t in TRANSITIONS for a in ((0, 1) if t == "points_filled" else (0,))])
def test_transition_from_every_combination(L, transition, arg):
    seen = 0
    for k in range(8):
        for have in itertools.combinations(STAGES, k):
            for flags in FLAG_CASES:
                io = (C.c_uint32 * 6)(bits_of(L, have), *[flags[n] for n in FLAG_NAMES])
                assert L.ps_apply(TRANSITIONS[transition], arg, io) == 0
                want_have, want_flags = model(transition, arg, have, flags)
                assert io[0] == bits_of(L, want_have), (transition, have)
                assert dict(zip(FLAG_NAMES, list(io)[1:])) == want_flags, (transition, have, flags)
            seen += 1
    assert seen == 128
    assert L.ps_apply(99, 0, (C.c_uint32 * 6)()) == -1


def test_stage_values_fresh_state_and_needs(L):
    values = [L.ps_stage(k) for k in range(7)]
    assert sorted(values) == [1, 2, 4, 8, 16, 32, 64] and L.ps_fresh() == 0          # sfm_pair_create: nothing is current
    for have in range(128):
        for stages in range(128):
            assert L.ps_has(have, stages) == int(have & stages == stages)
            assert L.ps_missing(have, stages) == stages & ~have
    # the second table's one two-stage need: sfm_get_result
    e, pose = bits_of(L, ["E"]), bits_of(L, ["pose"])
    assert not L.ps_has(e, e | pose) and not L.ps_has(pose, e | pose) and L.ps_has(e | pose, e | pose)


def test_state_texts_name_the_missing_stage_and_its_call(L):
    calls = {"points": "fillXU / set_points", "E": "estimateE", "P": "computePosecandidates", "pose": "choosePose",
             "points3d": "linear_triangulation", "refined": "no refinement since the last fillXU / set_points / reset",
             "view": "no registration since the last fillXU / set_points / reset"}
    texts = set()
    for s in STAGES:
        t = L.ps_hint(bits_of(L, [s])).decode()
        assert calls[s] in t, (s, t)
        texts.add(t)
    assert len(texts) == 7 and L.ps_hint(0) == b""
    assert L.ps_hint(bits_of(L, ["E", "pose"])) == L.ps_hint(bits_of(L, ["E"]))     # the first missing stage speaks


def sources():
    for d in (CSRC, os.path.join(CSRC, "ab")):
        for f in sorted(os.listdir(d)):
            if f.endswith((".hip", ".hpp", ".cpp")):
                yield f, open(os.path.join(d, f)).read()


def test_only_the_header_assigns_a_stage():
    mutators = r"\b(reset|points_filled|points_set|E_finalized|candidates_done|pose_chosen|triangulated|chain_done|refined|view_registered|view_dropped)\(\)?"
    for name, text in sources():
        if name == "pair_state.hpp":
            continue
        assert not re.search(r"\bhave_(points|E|P|pose|points3d|refined|view)\b", text), name
        assert not re.search(r"state\.have\s*(=[^=]|\|=|&=|\^=)", text), name
        if name != "abi.hip":
            assert not re.search(r"state\." + mutators, text), name
    abi = dict(sources())["abi.hip"]
    assert "if (pair->pipe_pending) {" not in abi                       # the flush line is spelled once (SFM_FLUSH, common.hpp)
    # in abi.hip a transition follows success: on the line that tests rc, or (sfm_pair_reset, sfm_estimate_E_pipelined, the regrowth
    # inside sfm_register_view) after every check of the entry point has returned
    unguarded = []
    for line in abi.splitlines():
        m = re.search(r"state\." + mutators, line)
        if m and "if (rc == SFM_OK)" not in line:
            unguarded.append(m.group(1))
    assert sorted(unguarded) == ["E_finalized", "reset", "view_dropped"]
