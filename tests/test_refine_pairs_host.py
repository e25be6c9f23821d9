"""CPU: sfm_refine_pairs (the batched two-view bundle adjustment) as far as it goes without a GPU -- the header declares it,
the library exports it, and every argument check that needs no device answers before the first device call."""
import ctypes as C
import os
import re

import pytest

import cuda_sfm_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fn():
    f = S.lib().sfm_refine_pairs
    f.restype = C.c_int
    return f


def test_declared_exported_and_wrapped():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sfm_refine_pairs\s*\(\s*sfm_pair\s*\*\s*const\s*\*\s*pairs\s*,\s*int\s+num_pairs\s*,"
                     r"\s*const\s+sfm_refine_params\s*\*\s*p\s*,\s*const\s+uint8_t\s*\*\s*const\s*\*\s*d_masks\s*\)\s*;", txt)
    assert hasattr(S.lib(), "sfm_refine_pairs") and "sfm_refine_pairs" in S.EXPORTS
    assert callable(S.refine_pairs) and callable(S.refine_pairs_enqueue)
    assert "sfm_refine_pairs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_checks_come_before_any_device_call(fn):
    p = S.refine_params()
    fake = (C.c_void_p * 1)(0x1000)                      # never dereferenced: the checks that reject the call come first
    null = (C.c_void_p * 1)(None)
    assert fn(None, 1, C.byref(p), None) == S.E_INVALID
    assert fn(None, -1, C.byref(p), None) == S.E_INVALID
    assert fn(fake, -1, C.byref(p), None) == S.E_INVALID
    assert fn(fake, 1, None, None) == S.E_INVALID
    assert fn(null, 1, C.byref(p), None) == S.E_INVALID   # a null entry
    assert fn(fake, 65536, C.byref(p), None) == S.E_INVALID
    assert S.lib().sfm_last_error()


def test_an_empty_list_is_not_an_error(fn):
    p = S.refine_params()
    assert fn(None, 0, C.byref(p), None) == S.OK
    assert fn((C.c_void_p * 1)(0x1000), 0, C.byref(p), None) == S.OK
    assert fn(None, 0, None, None) == S.E_INVALID        # the parameters are checked whatever the count
    S.refine_pairs_enqueue([], p)
    assert S.refine_pairs([]) == []
