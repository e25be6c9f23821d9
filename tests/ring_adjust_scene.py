"""Inputs of the sfm_adjust_ring tests (helper, not a test): sfm_fuse_ring's results of a fuse_ring_scene ring as the arrays the
call reads, and the wrapper around the host build (tests/hostcheck/libringadjustcheck.so)."""
import ctypes as C
import functools
import os

import numpy as np

import chain_adjust_scene as CS
import fuse_ring_scene as FRS

ROOT = CS.ROOT
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libringadjustcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.ring_adjust_run.restype = C.c_int
    h.ring_adjust_run.argtypes = [C.c_int] + [C.c_void_p] * 9
    h.ring_adjust_first_system.restype = None
    h.ring_adjust_first_system.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 4
    h.ring_adjust_track_terms.restype = None
    h.ring_adjust_track_terms.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_void_p]
    h.ring_adjust_reduce_block.restype = None
    h.ring_adjust_reduce_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    h.ring_adjust_layout.argtypes = [C.c_int, C.c_void_p]
    return h


@functools.lru_cache(maxsize=None)
def fused_ring(k, n, seed, exact=False):
    """(scene, ring chain, sfm_fuse_ring's results by its host build) of fuse_ring_scene.build(k, n, seed)."""
    import cuda_sfm_amd as S
    kw = dict(noise_px=0.0, wrong_match=0.0, wrong_index=0.0) if exact else {}
    sc, ring = FRS.build(k, n, seed, **kw)
    return sc, ring, FRS.run_host(FRS.host_lib(), S, ring)


def ring_report_bytes(S, status=0):
    """A sfm_fuse_ring_report with the given status as the bytes the call reads."""
    r = S.FuseRingReport()
    r.status = int(status)
    r.first_invalid = -1
    return np.frombuffer(bytes(r), np.uint8).copy()


def fused_arrays(S, res, k, N, status=None):
    """fuse_ring's dict -> host arrays in the order of sfm_adjust_ring_in behind `pairs`: chain_adjust_scene.fused_arrays and the
    ring report (the dict's own status unless `status` is given)."""
    st = res["report"]["status"] if status is None else status
    return CS.fused_arrays(res, k, N) + [ring_report_bytes(S, st)]


def empty_outputs(S, k, N, fill=0):
    return [np.full(24 * k, fill, np.float32), np.full(4 * N, fill, np.float32), np.full(N, fill, np.uint8), np.full(N, fill, np.float32),
            np.full(S.ADJUST_RING_REPORT_DTYPE.itemsize, fill, np.uint8)]


def results(S, outs, k, N, T):
    cams, pts, used, err, rep = outs
    return dict(cams=cams.reshape(k, 2, 12), points=pts.reshape(4, N)[:, :T].copy(), used=used[:T].copy(), err=err[:T].copy(),
                report=rep.view(S.ADJUST_RING_REPORT_DTYPE)[0].copy())


def _tables(ring):
    pairs = ring["pairs"]
    k = len(pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = dict(X0=[f32(P["X0"]) for P in pairs], X1=[f32(P["X1"]) for P in pairs], K=[f32(P.get("K", ring["K"])) for P in pairs])
    tables = {name: (C.c_void_p * k)(*[a.ctypes.data for a in arrs]) for name, arrs in keep.items()}
    n = np.array([P["n"] for P in pairs], np.int32); ld = np.array([P["ld"] for P in pairs], np.int32)
    return keep, tables, n, ld


def run_host(HL, S, ring, fused, **kw):
    """The host build over a ring's pairs and the arrays of fused_arrays, AdjustRingParams fields kw: results' dict + `accepts` (64:
    per iteration 1 accepted, 2 rejected, 3 failed solve) + `band` (every system formed kept to the folded band)."""
    p = S.adjust_ring_params(**kw)
    k = len(ring["pairs"])
    keep, tables, n, ld = _tables(ring)
    N = int(n.sum())
    outs = empty_outputs(S, k, N)
    accepts = np.zeros(64, np.uint8)
    i = S.AdjustRingIn(None, *[a.ctypes.data for a in fused])
    o = S.AdjustRingOut(*[a.ctypes.data for a in outs])
    band = HL.ring_adjust_run(k, vp(n), vp(ld), C.cast(tables["X0"], C.c_void_p), C.cast(tables["X1"], C.c_void_p), C.cast(tables["K"], C.c_void_p),
                              C.cast(C.byref(i), C.c_void_p), C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(o), C.c_void_p), vp(accepts))
    return dict(results(S, outs, k, N, int(fused[7][0])), accepts=accepts, band=bool(band), raw=outs)


def first_system(HL, S, ring, fused, lam, **kw):
    """The host build's first reduced system at damping lam: dense (6 nb x 6 nb, block order), rhs, the folded band's solution x
    (block order) and info (band claim held, positive definite, folded band width, used tracks)."""
    p = S.adjust_ring_params(**kw)
    k = len(ring["pairs"])
    keep, tables, n, ld = _tables(ring)
    Nn = 6 * (k - 1)
    dense, rhs, x, info = np.zeros((Nn, Nn)), np.zeros(Nn), np.zeros(Nn), np.zeros(4, np.int32)
    i = S.AdjustRingIn(None, *[a.ctypes.data for a in fused])
    HL.ring_adjust_first_system(k, vp(n), vp(ld), C.cast(tables["X0"], C.c_void_p), C.cast(tables["X1"], C.c_void_p), C.cast(tables["K"], C.c_void_p),
                                C.cast(C.byref(i), C.c_void_p), C.cast(C.byref(p), C.c_void_p), float(lam), vp(dense), vp(rhs), vp(x), vp(info))
    return dense, rhs, x, info
