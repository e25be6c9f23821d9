"""GPU: sfm_intersect_tracks (csrc/intersect.hip) through the C ABI against the host build of the same arithmetic
(tests/hostcheck/libintersectcheck.so), byte for byte on points, flags, errors and counts, on the override path of
tests/test_gpu_fuse.py (DeviceChain: pairs that only have fillXU).  The hand-built tables of intersect_scene (tracks of 2 .. 131
views over 130 pairs; views that share one centre) with every track by wavefront, every track by lane and the default split -- the
lengths 63 .. 66 and 128, 129, 131 are where chunking, the ragged last chunk and the ordered sum can go wrong, 31 .. 33 straddle the
default split -- the three runs equal to each other; tables from the device's own sfm_fuse_ring + sfm_adjust_ring and sfm_fuse_chain
+ sfm_adjust_chain with and without d_skip = d_used; determinism, nothing in any pair changed, canaries behind the T tracks and
behind every output, every refusal with nothing written."""
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import fuse_ring_scene as RS
import fuse_scene as FS
import intersect_scene as IS
from test_gpu_align import read_buffers
from test_gpu_fuse import DeviceChain
from test_gpu_fuse_ring import DeviceRing, REPORT_BYTES

pytestmark = pytest.mark.gpu
PATTERN, SLACK = 0xA5, 64
INT32_MAX = 2 ** 31 - 1
SPLITS = (("every track by wavefront", 2), ("every track by lane", INT32_MAX), ("the default split", 0))
# Kernels against the host build: the same header functions per view and sums taken in list order.  The bar on every output is
# equality (what 6f, 6h, 6i, 6k and 6l measured with these headers): a difference is a summation-order finding to fix.
u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def HL():
    return IS.host_lib()


def filled(gpu, N):
    """Output buffers of pattern bytes, SLACK elements longer than the call may write."""
    torch, dev, ctx = gpu
    f = lambda n, dt, v: torch.full((int(n) + SLACK,), v, dtype=dt, device=dev)
    return (f(4 * N, torch.float32, -3.0), f(N, torch.uint8, PATTERN), f(N, torch.float32, -3.0), f(8, torch.int32, -7))


def untouched(outs):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, PATTERN, -3.0, -7)))


def run_device(gpu, pairs, table, N, T, outs=None, **kw):
    """The call into pattern-filled buffers: results' dict, after the canaries behind the T tracks and behind every output."""
    torch, dev, ctx = gpu
    outs = outs if outs is not None else filled(gpu, N)
    S.intersect_tracks_enqueue(ctx, pairs, table, S.intersect_params(**kw), outs)
    ctx.synchronize()
    pts, flags, err, counts = (t.cpu().numpy() for t in outs)
    assert (pts[:4 * N].reshape(4, N)[:, T:] == -3.0).all() and (pts[4 * N:] == -3.0).all()
    assert (flags[T:] == PATTERN).all() and (err[T:] == -3.0).all() and (counts[8:] == -7).all()
    return S.intersect_tracks_results([t[:n] for t, n in zip(outs, (4 * N, N, N, 8))], N, T)


def equal(a, b, what):
    for q in ("points", "flags", "err"):
        same = u8(a[q]).reshape(-1, len(a["flags"]), 4 if q != "flags" else 1) == u8(b[q]).reshape(-1, len(a["flags"]), 4 if q != "flags" else 1)
        assert same.all(), (what, q, "tracks", np.flatnonzero(~same.all((0, 2)))[:8])
    assert a["counts"] == b["counts"], (what, a["counts"], b["counts"])


# ---- the hand-built tables -----------------------------------------------------------------------------------------------------
def hand_tables():
    ch, tb, truth, depth = IS.hand_built()
    T = len(tb["flags"])
    moved = IS.displaced(tb, truth, depth, 0.05)
    mixed = moved["points"].copy()
    mixed[:, ::4] = np.nan                                                      # no C: L starts the track
    mixed[:3, 1::4] = tb["points"][:3, 1::4]                                    # the truth: the candidates tie closely
    flags = tb["flags"].copy(); flags[5] = 0; flags[20] = 7                     # no class: copied through
    skip = np.zeros(T, np.uint8); skip[2::5] = 1
    return ch, [("columns 5 % off", moved, None), ("NaN, true and skipped columns", dict(moved, points=mixed, flags=flags), skip)]


def test_hand_built_table_three_splits(gpu, HL):
    torch, dev, ctx = gpu
    ch, tables = hand_tables()
    dc = DeviceChain(gpu, ch)
    k, N = len(ch["pairs"]), sum(P["n"] for P in ch["pairs"])
    for what, tb, skip in tables:
        T = len(tb["flags"])
        arrays = IS.table_arrays(tb, k, N, skip=skip)
        want = IS.run_host(HL, S, dc.host, arrays)
        table = [to_dev(torch, dev, a) if a is not None else None for a in arrays]
        runs = [run_device(gpu, dc.pairs, table, N, T, wave_min_views=w) for _, w in SPLITS]
        print(f"intersect hand-built, {what}: {runs[0]['counts']}")
        for (name, _), got in zip(SPLITS, runs):
            equal(got, want, (what, name))
        equal(runs[0], runs[1], (what, "wavefront against lane"))
        equal(runs[1], runs[2], (what, "lane against default"))
        assert want["counts"]["intersected"] >= 20 and np.isin(np.diff(tb["track_offset"]), IS.LENGTHS).all()
    dc.close()


def test_views_that_share_one_centre_three_splits(gpu, HL):
    torch, dev, ctx = gpu
    ch, tb, truth = IS.shared_centre()
    dc = DeviceChain(gpu, ch)
    bad = tb["points"].copy()
    bad[:, ::2] = np.nan
    bad[2, 1::2] = -10.0
    for what, table_h in (("true columns", tb), ("no eligible start", dict(tb, points=bad))):
        arrays = IS.table_arrays(table_h, 3, 48)
        want = IS.run_host(HL, S, dc.host, arrays)
        table = [to_dev(torch, dev, a) if a is not None else None for a in arrays]
        for name, w in SPLITS:
            equal(run_device(gpu, dc.pairs, table, 48, len(tb["flags"]), wave_min_views=w), want, (what, name))
    assert want["counts"]["no_start"] == len(tb["flags"])
    dc.close()


# ---- tables from the device's own calls ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring(k, n, seed=17):
    return RS.build(k, n, seed)


@functools.lru_cache(maxsize=None)
def scene(n, seed=17):
    return FS.build(n, seed)


def fuse_on_device(gpu, dx, is_ring):
    """The device's own fused table of a DeviceRing / DeviceChain: the tensors in the order of sfm_fuse_out (zeroed first: what lies
    behind the T tracks is read back too) and the ring report."""
    torch, dev, ctx = gpu
    k, N = len(dx.pairs), sum(p.num_points for p in dx.pairs)
    outs = S._fuse_buffers(torch, dev, k, N)
    for t in outs:
        t.zero_()
    rep = torch.zeros(REPORT_BYTES, dtype=torch.uint8, device=dev)
    if is_ring:
        S.fuse_ring_enqueue(ctx, dx.pin(), dx.lin(), S.fuse_ring_params(), outs, rep)
    else:
        pin = [(p,) + o for p, o in zip(dx.pairs, dx.over)]
        links = [(dx.indices[i], a[0], a[1], a[2], a[4]) for i, a in enumerate(dx.links)]
        S.fuse_chain_enqueue(ctx, pin, links, S.fuse_params(), outs)
    ctx.synchronize()
    return outs, rep, k, N


def adjusted_on_device(gpu, dx, is_ring, **kw):
    """(table tensors as sfm_intersect_in takes them but for d_skip, the adjustment's d_used, k, N, T): sfm_fuse_* then sfm_adjust_* on
    the device, the adjusted cameras and points in place of the table's own."""
    torch, dev, ctx = gpu
    outs, rep, k, N = fuse_on_device(gpu, dx, is_ring)
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = outs
    if is_ring:
        adj = S.adjust_ring_buffers(dev, k, N)
        S.adjust_ring_enqueue(ctx, dx.pairs, (root, cams, off, ocam, orec, pts, flags, counts, rep), S.adjust_ring_params(**kw), adj)
    else:
        adj = S.adjust_chain_buffers(dev, k, N)
        S.adjust_chain_enqueue(ctx, dx.pairs, (root, cams, off, ocam, orec, pts, flags, counts), S.adjust_chain_params(**kw), adj)
    ctx.synchronize()
    T = int(counts[0].item())
    adj[2][T:] = 0                                                              # d_used is written for the T tracks only
    return [adj[0], off, ocam, orec, adj[1], flags, counts], adj[2], k, N, T


def check_adjusted(gpu, HL, dx, is_ring, what, **kw):
    table, used, k, N, T = adjusted_on_device(gpu, dx, is_ring, **kw)
    lens = np.diff(table[1].cpu().numpy()[:T + 1])
    for skip in (None, used):
        arrays = [t.cpu().numpy().copy() for t in table] + [skip.cpu().numpy().copy() if skip is not None else None]
        want = IS.run_host(HL, S, dx.host, arrays)
        got = run_device(gpu, dx.pairs, table + [skip], N, T)
        print(f"intersect {what}, {'d_skip = d_used' if skip is not None else 'no d_skip'}: {got['counts']}, longest track {lens.max() if T else 0}")
        equal(got, want, (what, skip is not None))
        c = got["counts"]
        assert c["tracks"] == T and c["intersected"] + c["copied"] == T and c["refined"] + c["kept"] + c["no_start"] == c["intersected"]
        if skip is not None:
            assert c["copied"] >= int(used[:T].sum().item())
    return got


@pytest.mark.parametrize("n", [63, 65, 257])
@pytest.mark.parametrize("k", [3, 5])
def test_tables_from_the_devices_own_calls(gpu, HL, k, n):
    sc, rg = ring(k, n)
    dr = DeviceRing(gpu, rg)
    check_adjusted(gpu, HL, dr, True, f"ring k={k} n={n}")
    dr.close()
    sc, ch = scene(n)
    dc = DeviceChain(gpu, FS.head(ch, k))
    check_adjusted(gpu, HL, dc, False, f"chain k={k} n={n}")
    dc.close()


def test_a_chain_with_a_cut_and_over_long_tracks(gpu, HL):
    sc, ch = scene(257, 7)
    cut = dict(ch, links=[dict(L, status=S.REFINE_DEGENERATE) if i == 2 else L for i, L in enumerate(ch["links"])])
    dc = DeviceChain(gpu, cut)
    check_adjusted(gpu, HL, dc, False, "chain of 5 x 257 cut behind pair 2")
    dc.close()
    sc, rg = RS.build(6, 257, 7)                                                # 240 tracks of more than three views
    dr = DeviceRing(gpu, rg)
    got = check_adjusted(gpu, HL, dr, True, "ring (6, 257, 7) at W = 3", max_track_views=3)
    assert got["counts"]["intersected"] >= 240
    dr.close()


# ---- call hygiene --------------------------------------------------------------------------------------------------------------
def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    sc, ch = scene(257, 7)
    dc = DeviceChain(gpu, ch)
    table, used, k, N, T = adjusted_on_device(gpu, dc, False)
    full = table + [used]
    before = [read_buffers(p, ctx) for p in dc.pairs]
    first, second = run_device(gpu, dc.pairs, full, N, T), run_device(gpu, dc.pairs, full, N, T)
    equal(first, second, "second call")
    for p, bufs in zip(dc.pairs, before):                                      # every SFM_BUF_* of every pair
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    outs = filled(gpu, N)
    params = S.intersect_params()
    pairs = dc.pairs

    def refused(code, pr=pairs, tb=full, p=params, o=outs, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.intersect_tracks_enqueue(context, pr, tb, p, o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    # a NULL argument, every required field
    refused(S.E_INVALID, p=None)
    refused(S.E_INVALID, context=None)
    refused(S.E_INVALID, tb=None)
    refused(S.E_INVALID, o=None)
    for i in range(7):
        assert "sfm_intersect_in" in refused(S.E_INVALID, tb=full[:i] + [None] + full[i + 1:])
    for i in (0, 1, 3):
        assert "d_err" in refused(S.E_INVALID, o=outs[:i] + (None,) + outs[i + 1:])
    assert "pairs[2]: null pair" in refused(S.E_INVALID, pr=pairs[:2] + [None] + pairs[3:])
    # the parameters
    assert "reserved" in refused(S.E_INVALID, p=S.intersect_params(reserved=[0, 0, 0, 1]))
    assert "wave_min_views" in refused(S.E_INVALID, p=S.intersect_params(wave_min_views=1))
    assert "wave_min_views" in refused(S.E_INVALID, p=S.intersect_params(wave_min_views=-5))
    assert "max_iterations" in refused(S.E_INVALID, p=S.intersect_params(max_iterations=51))
    assert "threshold_px" in refused(S.E_INVALID, p=S.intersect_params(threshold_px=0.0))
    # aliasing: an output on an input, an output on another output
    assert "out.d_flags overlaps in.d_skip" in refused(S.E_INVALID, tb=table + [outs[1]])
    assert "out.d_points overlaps in.d_points" in refused(S.E_INVALID, tb=full[:4] + [outs[0].data_ptr() + 64] + full[5:])
    assert "out.d_flags overlaps in.d_flags" in refused(S.E_INVALID, o=(outs[0], table[5]) + outs[2:])
    big = torch.full((8 * N,), -3.0, dtype=torch.float32, device=dev)
    assert "out.d_err overlaps out.d_points" in refused(S.E_INVALID, o=(big, outs[1], big.data_ptr() + 16 * N - 4, outs[3]))
    # the pair list
    assert "pairs[3]: the pair is listed twice" in refused(S.E_INVALID, pr=pairs[:3] + [pairs[1]] + pairs[4:])
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, ch["K"], ch["Kinv"], 2, 257)
    foreign.fillXU(to_dev(torch, dev, ch["pairs"][2]["sift"]))
    assert "pairs[2]: the pair belongs to another context" in refused(S.E_INVALID, pr=pairs[:2] + [foreign] + pairs[3:])
    bare = S.ImagePair(ctx, ch["K"], ch["Kinv"], 2, 257)                       # no points at all
    assert "pairs[2]" in refused(S.E_STATE, pr=pairs[:2] + [bare] + pairs[3:])
    assert untouched(outs) and bool((big == -3.0).all())
    # zero pairs: SFM_OK, nothing written
    S.intersect_tracks_enqueue(ctx, [], full, params, outs)
    ctx.synchronize()
    assert untouched(outs)
    equal(run_device(gpu, pairs, full, N, T, outs=outs), first, "the same buffers serve the valid call")
    for p in (bare, foreign):
        p.close()
    other.close()
    dc.close()
