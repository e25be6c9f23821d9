"""Paired passes of the per-tile pre-filter rule (csrc/ransac_prefilter.hip): a lane builds the operands of its OWN hypothesis once
(prefilter_record.hpp: pf_tile_operands_full) where the single passes built them twice, once per half of the wavefront
(pf_tile_operands_half).  The one build must give each half bit for bit what that half built for itself: all 16 fp16 values of either
half, for every flag word (scan flag set or not, with and without the b-safe flag), over the tiles of the bench scene and of two
ragged ones, for a few thousand hypotheses of the keyed sampler.  Host-compiled (tests/hostcheck/pfpaircheck.hip) with the header's own
stand-ins for the hardware's reciprocal and square root."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from cuda_sfm_amd import synth
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p = C.POINTER(C.c_float)
H = 3000                                   # hypotheses per scene


def fp(a):
    return a.ctypes.data_as(f32p)


@functools.lru_cache(maxsize=None)
def libs():
    pair = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpfpaircheck.so"))
    pair.pfpair_compare.restype = C.c_long
    pair.pfpair_compare.argtypes = [f32p, C.c_int, C.c_float, C.c_float, f32p, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    pair.pfpair_box.argtypes = [f32p, C.c_float, f32p]
    host = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libhostcheck.so"))
    host.hc_pf_morton_key.restype = C.c_uint32
    host.hc_pf_morton_key.argtypes = [C.c_float] * 6
    lds = C.CDLL(os.path.join(ROOT, "tests", "hostcheck", "libpfldscheck.so"))
    return pair, host, lds


@functools.lru_cache(maxsize=None)
def scene_tiles(n, seed):
    """(E of H hypotheses, bound, [maxima of x, -x, y, -y, u, -u, v, -v per tile]): the tiles are runs of the Morton-bucket order of
    the first view (ransac_prefilter.hip: pf_bucket_of, a stable bucket ordering)."""
    _, host, lds = libs()
    sc = synth.two_view_scene(n) if seed is None else synth.two_view_scene(n, seed=seed)
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    _, _, E = O.ransac_range_fast(X0, X1, 0, H, np.float32(1e-6), 0, seed=11, want_counts=False, want_E=True)
    u, v, x, y = X0[0, :n], X0[1, :n], X1[0, :n], X1[1, :n]
    B = float(max(np.abs(a).max() for a in (u, v, x, y)))
    bucket = np.array([host.hc_pf_morton_key(float(a), float(b), -B, B, -B, B) >> 20 for a, b in zip(u, v)])
    order = np.argsort(bucket, kind="stable")
    tile = lds.pfcheck_tile_points(X0.shape[1])
    exts = []
    for first in range(0, n, tile):
        m = order[first:first + tile]
        exts.append(np.array([x[m].max(), (-x[m]).max(), y[m].max(), (-y[m]).max(), u[m].max(), (-u[m]).max(), v[m].max(), (-v[m]).max()], np.float32))
    return np.ascontiguousarray(E, np.float32).reshape(H, 9), B, exts


@pytest.mark.parametrize("thr", [1e-6, 1e-8])
@pytest.mark.parametrize("n,seed,ntiles", [(4096, None, 4), (1100, 2000, 2), (2100, 3000, 3)])
def test_one_build_equals_the_two_halves(n, seed, ntiles, thr):
    pair, _, _ = libs()
    E, B, exts = scene_tiles(n, seed)
    assert len(exts) == ntiles
    for t, ext in enumerate(exts):
        box = np.zeros(8, np.float32)
        pair.pfpair_box(fp(ext), B, fp(box))
        assert np.all(box[0::2] < box[1::2]) and np.all(np.abs(box) <= B), f"tile {t}: not a tile's box {box}"
        first_bad = (C.c_int * 4)()
        nonzero = C.c_long(0)
        bad = pair.pfpair_compare(fp(E), H, thr, B, fp(ext), first_bad, C.byref(nonzero))
        print(f"n {n} tile {t} thr {thr}: {H} hypotheses x 4 flag words x 2 halves x 16 values, {bad} differ; {nonzero.value} hypotheses with operands")
        assert bad == 0, f"tile {t}: {bad} values differ, first (hypothesis, flags, half, slot) = {list(first_bad)}"
        assert nonzero.value > H // 2


def test_untamed_and_degenerate_hypotheses():
    """entries beyond 2, NaN, the zero matrix, zero rows (a divisor that vanishes everywhere): sigma 0 or its cap, the same in both builds"""
    pair, _, _ = libs()
    E, B, exts = scene_tiles(1100, 2000)
    odd = E[:64].copy()
    odd[0, :] = 0.0
    odd[1, :6] = 0.0
    odd[2, 4] = 3.0
    odd[3, 8] = np.nan
    odd[4, :] *= 1e-20
    odd[5, [0, 1, 3, 4]] = 0.0
    first_bad = (C.c_int * 4)()
    nonzero = C.c_long(0)
    for ext in exts:
        assert pair.pfpair_compare(fp(odd), len(odd), 1e-6, B, fp(ext), first_bad, C.byref(nonzero)) == 0, list(first_bad)
