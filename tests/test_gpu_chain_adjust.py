"""GPU: sfm_adjust_chain (csrc/chain_adjust.hip) through the C ABI against the host build of the same arithmetic
(tests/hostcheck/libchainadjustcheck.so), both on sfm_fuse_chain's outputs as ITS host build computes them from the device's own
normalised observations (pairs that only have fillXU).  The main grid, a ragged chain, a cut whose second segment is one pair,
over-long tracks, 70 pairs as 14 segments of five (fuse_scene's six views, joined by cuts: more pairs than one block of the
per-pair kernels has lanes) and as ONE segment of 70 cameras (chain_adjust_scene.strip: more camera blocks than a wavefront has
lanes, 420 columns of the banded factor, a band whose first column moves), head pairs whose tracks span several rounds; the
unification, degenerate segments, determinism, nothing in any pair changed, every refusal with nothing written."""
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import chain_adjust_reference as CR
import chain_adjust_scene as CS
import fuse_scene as FS
from test_gpu_align import read_buffers
from test_gpu_fuse import DeviceChain

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
PAIRS = [1, 2, 3, 5]
RECORDS = [63, 64, 65, 257]
# Kernels against the host build at 10 iterations.  The per-track arithmetic is the same header functions; the only sums taken in
# another order are the 64-track transposed sums of the system pass (fp64) against the host build's track-by-track ones.
# MEASURED on the MI355X, the largest absolute difference over the 16 cases of the grid, the five other shapes and the 70-camera
# segment below, in the
# cameras, the points, the errors, the rms and the cost: every one is 0, so the bars, 4 x the measured maximum, are equality
# (what 6f and 6h found).
MEASURED = dict(cams=0.0, points=0.0, err=0.0, rms=0.0, cost=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}
INTEGERS = ("root", "status", "iterations", "accepted", "num_cameras", "num_tracks", "num_observations", "num_over_long")


@pytest.fixture(scope="module")
def HL():
    return CS.host_lib()


@functools.lru_cache(maxsize=None)
def scene(n, seed=17):
    return FS.build(n, seed)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Fused:
    """A DeviceChain, sfm_fuse_chain's results for it by the host build, and those on the device."""

    def __init__(self, gpu, chain, change=None, res=None):
        torch, dev, ctx = gpu
        self.gpu, self.dc = gpu, DeviceChain(gpu, chain)
        self.k, self.N = len(chain["pairs"]), sum(P["n"] for P in chain["pairs"])
        self.res = res if res is not None else FS.run_host(FS.host_lib(), S, self.dc.host)      # (res: a model built without sfm_fuse_chain)
        if change is not None:
            self.res = change(self.res)
        self.arrays = CS.fused_arrays(self.res, self.k, self.N)
        self.dev = [to_dev(torch, dev, a) for a in self.arrays]
        self.T = int(self.arrays[7][0])

    def device(self, outs=None, **kw):
        torch, dev, ctx = self.gpu
        outs = outs if outs is not None else S.adjust_chain_buffers(dev, self.k, self.N)
        S.adjust_chain_enqueue(ctx, self.dc.pairs, self.dev, S.adjust_chain_params(**kw), outs)
        ctx.synchronize()
        return S.adjust_chain_results(outs, self.k, self.N, self.T)

    def host(self, HL, **kw):
        return CS.run_host(HL, S, self.dc.host, self.arrays, **kw)

    def close(self):
        self.dc.close()


def differences(got, want):
    f = lambda a: np.asarray(a, np.float64)
    d = dict(cams=float(np.abs(f(got["cams"]) - f(want["cams"])).max()), points=0.0, err=0.0)
    if got["points"].size:
        fin = np.isfinite(want["points"]) & np.isfinite(got["points"])
        d["points"] = float(np.abs(f(got["points"])[fin] - f(want["points"])[fin]).max()) if fin.any() else 0.0
        fin = np.isfinite(want["err"]) & np.isfinite(got["err"])
        d["err"] = float(np.abs(f(got["err"])[fin] - f(want["err"])[fin]).max()) if fin.any() else 0.0
    d["rms"] = float(max(np.abs(f(got["reports"][c]) - f(want["reports"][c])).max() for c in ("initial_rms_px", "final_rms_px")))
    d["cost"] = float(np.abs(f(got["reports"]["final_cost"]) - f(want["reports"]["final_cost"])).max())
    return d


def check_against_host(HL, fu, what, iterations=(0, 10), **kw):
    """d_used and the reports' integers byte for byte; at 0 iterations everything byte for byte; at 10 the differences within BARS.
    Returns the last device result."""
    worst = dict.fromkeys(MEASURED, 0.0)
    for iters in iterations:
        got, want = fu.device(max_iterations=iters, **kw), fu.host(HL, max_iterations=iters, **kw)
        assert np.array_equal(got["used"], want["used"]), (what, iters)
        for f in INTEGERS:
            assert np.array_equal(got["reports"][f], want["reports"][f]), (what, iters, f, got["reports"][f], want["reports"][f])
        assert np.array_equal(u8(got["reports"]["lambda"]), u8(want["reports"]["lambda"])), (what, iters)       # the damping: the accept sequence's trace
        assert np.array_equal(np.isinf(got["err"]), np.isinf(want["err"])) and np.array_equal(np.isnan(got["points"]), np.isnan(want["points"]))
        if iters == 0:
            for k in ("cams", "points", "err", "reports"):
                assert np.array_equal(u8(got[k]), u8(want[k])), (what, k)
        else:
            d = differences(got, want)
            worst = {k: max(worst[k], d[k]) for k in worst}
        # the unification: inside a segment camera 1 of pair p + 1 is the bytes of camera 2 of pair p
        root = got["reports"]["root"]
        for p in range(fu.k - 1):
            if root[p + 1] == root[p] and got["reports"][root[p]]["status"] != S.REFINE_DEGENERATE:
                assert got["cams"][p + 1, 0].tobytes() == got["cams"][p, 1].tobytes(), (what, p)
    rep = got["reports"][got["reports"]["root"] == np.arange(fu.k)]
    print(f"chain adjust {what}: {[(int(r['num_cameras']), int(r['num_tracks']), int(r['iterations']), int(r['accepted']), float(r['initial_rms_px']), float(r['final_rms_px'])) for r in rep]}, "
          f"differences at {iterations[-1]} iterations {worst}")
    for k, bar in BARS.items():
        assert worst[k] <= bar, (what, k, worst[k], bar)
    return got


@pytest.mark.parametrize("n", RECORDS)
@pytest.mark.parametrize("k", PAIRS)
def test_main_grid_against_the_host_build(gpu, HL, k, n):
    sc, ch = scene(n)
    fu = Fused(gpu, FS.head(ch, k))
    got = check_against_host(HL, fu, f"k={k} n={n}")
    rep = got["reports"][0]
    assert rep["num_cameras"] == k and rep["num_tracks"] == got["used"].sum()
    if rep["status"] != S.REFINE_DEGENERATE:
        assert rep["final_rms_px"] <= rep["initial_rms_px"]
    fu.close()


def test_other_shapes_against_the_host_build(gpu, HL):
    sc, ch = scene(257, 7)
    fu = Fused(gpu, FS.truncated(ch, [65, 257, 64, 257, 1]))
    check_against_host(HL, fu, "ragged 65/257/64/257/1")
    fu.close()
    # a cut whose second segment is one pair
    fu = Fused(gpu, dict(ch, links=[dict(L, status=S.REFINE_DEGENERATE) if i == 3 else L for i, L in enumerate(ch["links"])]))
    got = check_against_host(HL, fu, "cut 4 + 1")
    assert got["reports"]["root"].tolist() == [0, 0, 0, 0, 4] and got["reports"][4]["num_cameras"] == 1 and got["reports"][4]["num_tracks"] > 0
    # W = 3 on the five-pair chain: longer tracks are not used and counted
    lens = np.diff(fu.res["track_offset"])
    got = check_against_host(HL, fu, "W = 3", max_track_views=3)
    assert (lens > 3).sum() > 0 and got["reports"]["num_over_long"].sum() == (lens > 3).sum() and not got["used"][lens > 3].any()
    fu.close()
    # 70 pairs x 65 records as 14 segments: two blocks of the per-pair kernels (ONE segment of 70: test_one_segment_of_70_cameras)
    sc, ch65 = scene(65)
    fu = Fused(gpu, FS.tiled(ch65, 14))
    got = check_against_host(HL, fu, "tiled 14 x 5 x 65", iterations=(10,))
    assert got["reports"]["root"].tolist() == [5 * (i // 5) for i in range(70)]
    for s in range(1, 14):                                                     # a segment's bytes do not depend on the others
        assert got["cams"][5 * s:5 * s + 5].tobytes() == got["cams"][:5].tobytes() and got["reports"][5 * s]["final_cost"] == got["reports"][0]["final_cost"]
    fu.close()
    # 2 pairs x 1025 records: a head pair's tracks span several rounds of 64 and of 256
    sc, ch1025 = scene(1025)
    fu = Fused(gpu, FS.head(ch1025, 2))
    got = check_against_host(HL, fu, "k=2 n=1025")
    assert got["reports"][0]["num_tracks"] > 512
    fu.close()


def device_accept_sequence(fu, n):
    """The device keeps no sequence: a call with i iterations is the first i steps of a call with n, so the sequence is read from
    the reports of calls with 1 .. n iterations (a failed solve leaves `accepted` as a rejected step does)."""
    seq, before = [], 0
    for i in range(1, n + 1):
        r = fu.device(max_iterations=i)["reports"][0]
        assert r["iterations"] == i
        seq.append(1 if r["accepted"] > before else 2)
        before = int(r["accepted"])
    return seq


def test_one_segment_of_70_cameras(gpu, HL):
    """chain_adjust_scene.strip: 70 pairs x 65 records in ONE segment, tracks of 2 .. 8 views.  The solve block reduces 70 x 8 x 36
    band values, factors 420 columns (the band's first column moves from block 8 on) and steps 70 cameras; the per-pair kernels run
    two blocks.  Device against the host build: used flags, integers, accept sequence, bytes; both against the twin: used flags,
    counts, the degenerate decision; the cameras' differences are printed (the host-build bars are held on the CPU,
    tests/test_chain_adjust_host.py)."""
    chain, fused, truth = CS.strip()
    fu = Fused(gpu, chain, res=fused)
    got = check_against_host(HL, fu, "one segment of 70")
    want = fu.host(HL, max_iterations=10)
    rep = got["reports"][0]
    assert got["reports"]["root"].tolist() == [0] * 70 and rep["num_cameras"] == 70 and rep["status"] != S.REFINE_DEGENERATE
    assert rep["num_tracks"] == len(fused["flags"]) and rep["final_rms_px"] < 0.1 * rep["initial_rms_px"]
    for key in ("cams", "points", "used", "err", "reports"):
        assert np.array_equal(u8(got[key]), u8(want[key])), key
    n = int(want["reports"][0]["iterations"])
    seq, host_seq = device_accept_sequence(fu, n), [int(x) if x != 3 else 2 for x in want["accepts"][0][:n]]
    print(f"accept sequence, one segment of 70: device {seq}, host build {host_seq}")
    assert seq == host_seq and n >= 3
    twin = CR.adjust_chain(fu.dc.host["pairs"], chain["K"], fused)
    assert np.array_equal(got["used"] != 0, twin["used"])
    for f in ("num_cameras", "num_tracks", "num_observations", "num_over_long"):
        assert rep[f] == twin["reports"][0][f], f
    assert twin["reports"][0]["status"] != CR.DEGENERATE
    cams = got["cams"].astype(np.float64)
    print(f"  device - twin: rot {max(CS.rotation_angle(cams[p, 1, :9], twin['cams'][p, 1, :9]) for p in range(70)):.3g} rad, "
          f"t {np.abs(cams[:, 1, 9:] - twin['cams'][:, 1, 9:]).max():.3g} (|t| up to {np.abs(cams[:, 1, 9:]).max():.3g}), "
          f"rms {abs(float(rep['final_rms_px']) - twin['reports'][0]['final_rms_px']):.3g} px; twin accepts {twin['accepts'][0]}")
    fu.close()


def test_accept_sequence_equals_the_host_builds(gpu, HL):
    """The device keeps no sequence: a call with i iterations is the first i steps of a call with 10, so the sequence is read from
    the reports of calls with 1 .. 10 iterations and compared with the one the host build records."""
    sc, ch = scene(257, 7)
    for what, chain in (("five pairs", ch), ("two pairs", FS.head(ch, 2))):
        fu = Fused(gpu, chain)
        want = fu.host(HL, max_iterations=10)
        n = int(want["reports"][0]["iterations"])
        seq = device_accept_sequence(fu, n)
        host_seq = [int(x) if x != 3 else 2 for x in want["accepts"][0][:n]]      # (a failed solve leaves `accepted` as a rejected step does)
        print(f"accept sequence, {what}: device {seq}, host build {host_seq}")
        assert seq == host_seq and n >= 3
        fu.close()


def _only(res, keep):
    flags = np.full_like(res["flags"], 2)
    flags[list(keep)] = 1
    return dict(res, flags=flags)


def test_degenerate_segments_return_their_inputs(gpu, HL):
    sc, ch = scene(257, 7)
    two = FS.head(ch, 2)

    def few(n_short, n_long):
        def change(res):
            lens, heads = np.diff(res["track_offset"]), res["obs_cam"][res["track_offset"][:-1]] >> 1
            ok = (res["flags"] == 1) & np.isfinite(res["err"]) & (res["err"] < 2.0)
            short, long = np.flatnonzero(ok & (lens == 2) & (heads == 0)), np.flatnonzero(ok & (lens == 3))
            return _only(res, list(short[:n_short]) + list(long[:n_long]))
        return change
    for n_short, n_long, degenerate in ((16, 5, True), (16, 6, False), (9, 6, True), (10, 6, False)):
        fu = Fused(gpu, two, change=few(n_short, n_long))
        got = check_against_host(HL, fu, f"{n_short} + {n_long} tracks")
        assert got["used"].sum() == n_short + n_long
        assert (got["reports"][0]["status"] == S.REFINE_DEGENERATE) == degenerate, (n_short, n_long)
        if degenerate:
            assert got["cams"].tobytes() == np.asarray(fu.res["cams"], np.float32).tobytes() and got["reports"][0]["iterations"] == 0
            assert got["points"].tobytes() == np.asarray(fu.res["points"], np.float32).tobytes()
        fu.close()


def filled(torch, dev, k, N):
    f = lambda n, dt, v: torch.full((int(n),), v, dtype=dt, device=dev)
    return (f(24 * k, torch.float32, -3.0), f(4 * N, torch.float32, -3.0), f(N, torch.uint8, PATTERN), f(N, torch.float32, -3.0),
            f(k * S.ADJUST_CHAIN_REPORT_DTYPE.itemsize, torch.uint8, PATTERN))


def untouched(outs):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, -3.0, PATTERN, -3.0, PATTERN)))


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    sc, ch = scene(257, 7)
    fu = Fused(gpu, ch)
    before = [read_buffers(p, ctx) for p in fu.dc.pairs]
    first, second = fu.device(), fu.device()
    for key in first:
        assert np.array_equal(u8(first[key]), u8(second[key])), key
    for p, bufs in zip(fu.dc.pairs, before):                                   # every SFM_BUF_* of every pair
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    k, N = fu.k, fu.N
    outs = filled(torch, dev, k, N)
    params = S.adjust_chain_params()
    pairs, fused = fu.dc.pairs, tuple(fu.dev)

    def refused(code, pr=pairs, fz=fused, p=params, o=outs, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.adjust_chain_enqueue(context, pr, fz, p, o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    # a NULL argument
    refused(S.E_INVALID, p=None)
    refused(S.E_INVALID, context=None)
    refused(S.E_INVALID, fz=None)
    refused(S.E_INVALID, o=None)
    assert "sfm_adjust_chain_in" in refused(S.E_INVALID, fz=fused[:3] + (None,) + fused[4:])
    assert "d_err" in refused(S.E_INVALID, o=outs[:2] + (None,) + outs[3:])
    assert "pairs[2]: null pair" in refused(S.E_INVALID, pr=pairs[:2] + [None] + pairs[3:])
    # the parameters
    assert "reserved" in refused(S.E_INVALID, p=S.adjust_chain_params(reserved=[0, 0, 0, 1]))
    assert "max_track_views" in refused(S.E_INVALID, p=S.adjust_chain_params(max_track_views=1))
    assert "max_track_views" in refused(S.E_INVALID, p=S.adjust_chain_params(max_track_views=17))
    assert "max_iterations" in refused(S.E_INVALID, p=S.adjust_chain_params(max_iterations=51))
    # aliasing: an output on an input, an output on another output
    assert "out.d_cams overlaps in.d_cams" in refused(S.E_INVALID, o=(fused[1].data_ptr() + 48,) + outs[1:])
    assert "out.d_used overlaps in.d_flags" in refused(S.E_INVALID, o=outs[:2] + (fused[6],) + outs[3:])
    big = torch.full((8 * N,), -3.0, dtype=torch.float32, device=dev)
    assert "out.d_err overlaps out.d_points" in refused(S.E_INVALID, o=(outs[0], big, outs[2], big.data_ptr() + 16 * N - 4, outs[4]))
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
    S.adjust_chain_enqueue(ctx, [], fused, params, outs)
    ctx.synchronize()
    assert untouched(outs)
    S.adjust_chain_enqueue(ctx, pairs, fused, params, outs)                    # ... and the same buffers serve the valid call
    ctx.synchronize()
    got = S.adjust_chain_results(outs, k, N, fu.T)
    for key in first:
        assert np.array_equal(u8(first[key]), u8(got[key])), key
    for p in (bare, foreign):
        p.close()
    other.close()
    fu.close()
