"""GPU: sfm_fuse_ring (csrc/fuse_ring.hip) through the C ABI -- every output and the report against the host build of the same
arithmetic (tests/hostcheck/libfuseringcheck.so) on the override path (pairs that only have fillXU): rings of 3, 4 and 5 pairs of
every block-edge size, a ragged ring, first and last pairs of five node blocks, a ring of 257 pairs; OPEN and REJECTED against the
device's own sfm_fuse_chain byte for byte; determinism, nothing in any pair changed, every refusal with nothing written;
sfm_adjust_chain over the ring's table; the full six-view ring on the device against the host build and the fp64 twin
(tests/fuse_ring_reference.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import chain_adjust_scene as CS
import fuse_reference as FR
import fuse_ring_reference as RR
import fuse_ring_scene as RS
import fuse_scene as FS
import ring_scene
from test_gpu_align import chain as refined_chain, read_buffers
from test_gpu_fuse import read_back_chain
from test_fuse_ring_host import BAND, BAND_CAP, ERR_BAR, POINTS_BAR, seam_gain, seam_tracks, structure_equal

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
PAIRS = [3, 4, 5]
RECORDS = [1, 63, 64, 65, 257]                           # per pair: one node block is 256 records
# Kernels against the host build at 5 iterations: the same header functions per lane and per track, no sum whose order differs.
# MEASURED: the largest absolute difference over the 15 cases of the grid, the ragged ring, the 1025-record ends and the 257-pair
# ring on the MI355X, in the frames, the cameras, the points, the errors and the report's three closure numbers.  Every one is 0,
# so the bars, 4 x the measured maximum, are equality (what 6h found for the chain).
MEASURED = dict(frames=0.0, cams=0.0, points=0.0, err=0.0, closure=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}
INTEGERS = ("root", "track", "track_offset", "obs_cam", "obs_record", "flags")
REPORT_INTS = ("status", "first_invalid", "seam_proposals", "seam_ineligible", "seam_tracks", "seam_refined", "seam_kept")
CLOSURE = ("closure_log_scale", "closure_rotation_rad", "closure_t")
REPORT_BYTES = C.sizeof(S.FuseRingReport)


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


@functools.lru_cache(maxsize=None)
def ring(k, n, seed=17):
    return RS.build(k, n, seed)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


class DeviceRing:
    """A ring on the device on the override path: every pair only has fillXU; points, valid, pose and the k links' arrays are
    uploaded.  `host` is the same ring over the device's OWN normalised observations, for the host build and the twin."""

    def __init__(self, gpu, ring):
        torch, dev, ctx = gpu
        d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
        self.gpu, self.ctx, self.pairs, self.over, host_pairs = gpu, ctx, [], [], []
        for P in ring["pairs"]:
            pair = S.ImagePair(ctx, ring["K"], ring["Kinv"], 2, P["n"])
            pair.fillXU(to_dev(torch, dev, P["sift"]))
            self.pairs.append(pair)
            self.over.append((d(P["points"]), d(P["valid"]), d(P["pose"])))
            host_pairs.append(dict(P, X0=pair.get_XU(S.BUF_X0), X1=pair.get_XU(S.BUF_X1), ld=P["n"]))
        self.k, self.N = len(self.pairs), sum(P["n"] for P in ring["pairs"])
        self.indices, self.links = [], []
        for L in ring["links"]:
            rep = S.AlignReport(); rep.status = int(L["status"])
            self.indices.append(d(L["index"]))
            self.links.append((d(L["sim"]), d(L["inlier"]), d(L["err"]), None, d(np.frombuffer(bytes(rep), np.uint8).copy())))
        self.host = dict(ring, pairs=host_pairs)

    def run(self, **kw):
        return S.fuse_ring(self.pairs, self.indices, self.links, overrides=self.over, **kw)

    def pin(self):
        return [(p,) + o for p, o in zip(self.pairs, self.over)]

    def lin(self):
        return [(self.indices[i], a[0], a[1], a[2], a[4]) for i, a in enumerate(self.links)]

    def close(self):
        for p in self.pairs:
            p.close()


def differences(got, want):
    f = lambda a: np.asarray(a, np.float64)
    d = {k: float(np.abs(f(got[k]) - f(want[k])).max()) if got[k].size else 0.0 for k in ("frames", "cams", "points")}
    fin = np.isfinite(want["err"]) & np.isfinite(got["err"])
    d["err"] = float(np.abs(f(got["err"])[fin] - f(want["err"])[fin]).max()) if fin.any() else 0.0
    d["closure"] = max(abs(float(got["report"][q]) - float(want["report"][q])) for q in CLOSURE)
    return d


def check_against_host(HL, dr, what, iterations=(0, 5), **kw):
    """Integers and the report's integers byte for byte; at 0 iterations everything byte for byte; at 5 the differences within
    BARS.  Returns the last result."""
    worst = dict.fromkeys(MEASURED, 0.0)
    for iters in iterations:
        got = dr.run(max_iterations=iters, **kw)
        want = RS.run_host(HL, S, dr.host, max_iterations=iters, **kw)
        assert got["counts"] == want["counts"], (what, iters, got["counts"], want["counts"])
        for q in REPORT_INTS:
            assert got["report"][q] == want["report"][q], (what, iters, q, got["report"], want["report"])
        for k in INTEGERS:
            assert np.array_equal(got[k], want[k]), (what, iters, k)
        assert np.array_equal(np.isinf(got["err"]), np.isinf(want["err"])), (what, iters)
        if iters == 0:
            for k in ("frames", "cams", "points", "err"):
                assert np.array_equal(u8(got[k]), u8(want[k])), (what, k)
            for q in CLOSURE:
                assert np.float32(got["report"][q]).tobytes() == np.float32(want["report"][q]).tobytes(), (what, q)
        else:
            d = differences(got, want)
            worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"fuse ring {what}: {got['counts']}, {got['report']}, differences at {iterations[-1]} iterations {worst}")
    for k, bar in BARS.items():
        assert worst[k] <= bar, (what, k, worst[k], bar)
    if max(worst.values()) == 0.0:                                             # the same bytes, then
        for k in ("frames", "cams", "points", "err"):
            assert np.array_equal(u8(got[k]), u8(want[k])), (what, k)
    return got


@pytest.mark.parametrize("n", RECORDS)
@pytest.mark.parametrize("k", PAIRS)
def test_override_path_against_the_host_build(gpu, HL, k, n):
    sc, rg = ring(k, n)
    dr = DeviceRing(gpu, rg)
    got = check_against_host(HL, dr, f"k={k} n={n}")
    live = sum(int(FR.live_nodes(P).sum()) for P in dr.host["pairs"])
    assert got["report"]["status"] == S.RING_CLOSED and got["counts"]["segments"] == 1
    assert got["counts"]["observations"] == live + got["counts"]["tracks"] and seam_tracks(got).sum() == got["report"]["seam_tracks"]
    if n >= 63:
        assert got["report"]["seam_tracks"] > 0 and got["report"]["seam_ineligible"] > 0
    dr.close()


def test_ragged_ring_long_ends_and_a_ring_of_257_pairs(gpu, HL):
    sc, rg = ring(5, 257, 7)
    dr = DeviceRing(gpu, RS.truncated(rg, [65, 257, 64, 257, 1]))
    check_against_host(HL, dr, "ragged 65/257/64/257/1")
    dr.close()
    # pair 0 and pair k - 1 of 1025 records: five blocks of the two seam kernels
    sc, rg = ring(4, 1025)
    dr = DeviceRing(gpu, RS.truncated(rg, [1025, 65, 65, 1025]))
    got = check_against_host(HL, dr, "1025/65/65/1025")
    assert got["report"]["seam_proposals"] > 256
    dr.close()
    # 257 pairs of 65 records: two rounds of the frames kernel, walks back over many pairs
    sc, rg = ring(257, 65, 3)
    dr = DeviceRing(gpu, rg)
    got = check_against_host(HL, dr, "257 x 65")
    assert got["report"]["status"] == S.RING_CLOSED and got["report"]["seam_tracks"] > 0 and got["counts"]["longest_track"] > 8
    dr.close()


def filled(torch, dev, k, N):
    f = lambda n, dt, v: torch.full((int(n),), v, dtype=dt, device=dev)
    i32, f32 = torch.int32, torch.float32
    return (f(13 * k, f32, -3.0), f(k, i32, -9), f(24 * k, f32, -3.0), f(N, i32, -9), f(N + 1, i32, -9), f(2 * N, i32, -9), f(2 * N, i32, -9),
            f(4 * N, f32, -3.0), f(N, torch.uint8, PATTERN), f(N, f32, -3.0), f(8, i32, -9)), f(REPORT_BYTES, torch.uint8, PATTERN)


def untouched(outs, rep):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, -9, -3.0, -9, -9, -9, -9, -3.0, PATTERN, -3.0, -9))) and bool((rep == PATTERN).all())


def report_of(rep):
    r = S.FuseRingReport.from_buffer_copy(rep.cpu().numpy().tobytes())
    return {f: getattr(r, f) for f, _ in S.FuseRingReport._fields_}


@pytest.mark.parametrize("k", [3, 65, 257])
def test_open_and_rejected_rings_are_the_devices_own_chain(gpu, HL, k):
    """Into buffers filled with one pattern: every byte of sfm_fuse_out equals what sfm_fuse_chain writes on the same context for the
    k pairs and the first k - 1 links."""
    torch, dev, ctx = gpu
    sc, rg = ring(k, 65, 3)
    turned = ring_scene.compose((1.0, ring_scene.rodrigues([0.0, 5e-3, 0.0]), np.zeros(3)), ring_scene.unpack(rg["links"][k - 1]["sim"]))
    nan_t = rg["links"][k // 2]["sim"].copy(); nan_t[11] = np.nan

    def change(i, **c):
        return dict(rg, links=[dict(L, **c) if q == i else L for q, L in enumerate(rg["links"])])
    cases = [("closing link degenerate", change(k - 1, status=S.REFINE_DEGENERATE), S.RING_OPEN, k - 1),
             ("first link degenerate", change(0, status=S.REFINE_DEGENERATE), S.RING_OPEN, 0),
             ("NaN in an inner link", change(k // 2, sim=nan_t), S.RING_OPEN, k // 2),
             ("closing link turned 5e-3 rad", change(k - 1, sim=FS.sim13(*turned)), S.RING_REJECTED, -1)]
    for name, broken, status, first in cases:
        dr = DeviceRing(gpu, broken)
        params = S.fuse_ring_params()
        a, rep = filled(torch, dev, k, dr.N)
        b, _ = filled(torch, dev, k, dr.N)
        S.fuse_ring_enqueue(ctx, dr.pin(), dr.lin(), params, a, rep)
        S.fuse_chain_enqueue(ctx, dr.pin(), dr.lin()[:k - 1], params.fuse, b)
        ctx.synchronize()
        r = report_of(rep)
        want = RS.run_host(HL, S, dr.host)["report"]
        assert r["status"] == status and r["first_invalid"] == first, (name, r)
        for q in REPORT_INTS:
            assert r[q] == want[q] and (q in ("status", "first_invalid") or r[q] == 0), (name, q, r, want)
        for q in CLOSURE:
            assert np.float32(r[q]).tobytes() == np.float32(want[q]).tobytes(), (name, q, r, want)
        if status == S.RING_OPEN:
            assert (r["closure_log_scale"], r["closure_rotation_rad"], r["closure_t"]) == (0.0, 0.0, 0.0)
        else:
            assert abs(r["closure_rotation_rad"] - 5e-3) <= 1e-5
        for x, y, field in zip(a, b, S.FuseOut._fields_):
            assert torch.equal(x, y), (name, field[0])
        if status == S.RING_REJECTED:                                          # CLOSED under a wider gate
            wide = dr.run(max_closure_rotation_rad=1e-2)
            assert wide["report"]["status"] == S.RING_CLOSED and wide["report"]["seam_tracks"] > 0
        dr.close()


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    sc, rg = ring(5, 257, 7)
    dr = DeviceRing(gpu, rg)
    before = [read_buffers(p, ctx) for p in dr.pairs]
    first, second = dr.run(), dr.run()
    assert first["counts"] == second["counts"] and first["report"] == second["report"] and first["report"]["seam_tracks"] > 0
    for key in first:
        if key not in ("counts", "report"):
            assert np.array_equal(u8(first[key]), u8(second[key])), key
    for p, bufs in zip(dr.pairs, before):                                      # every SFM_BUF_* of every pair
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    k, N = 5, 5 * 257
    outs, rep = filled(torch, dev, k, N)
    params = S.fuse_ring_params()
    pin, links = dr.pin(), dr.lin()

    def refused(code, pairs=pin, lk=links, p=params, o=outs, r=rep, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.fuse_ring_enqueue(context, pairs, lk, p, o, r)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    # each argument
    assert "null" in refused(S.E_INVALID, context=None)
    assert "null" in refused(S.E_INVALID, lk=None)
    assert "null" in refused(S.E_INVALID, o=None)
    assert "null" in refused(S.E_INVALID, r=None)
    assert "null params" in refused(S.E_INVALID, p=None)
    assert "required" in refused(S.E_INVALID, o=outs[:3] + (None,) + outs[4:])
    assert "3..4096" in refused(S.E_INVALID, pairs=pin[:2], lk=links[:2])      # k = 2
    for f in range(5):                                                         # a missing field of the closing link
        assert "links[4]" in refused(S.E_INVALID, lk=links[:4] + [links[4][:f] + (None,) + links[4][f + 1:]])
    assert "links[1]" in refused(S.E_INVALID, lk=links[:1] + [(None,) + links[1][1:]] + links[2:])
    assert "pairs[3]: the pair is listed twice" in refused(S.E_INVALID, pairs=pin[:3] + [pin[1]] + pin[4:])
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, rg["K"], rg["Kinv"], 2, 257)
    foreign.fillXU(to_dev(torch, dev, rg["pairs"][2]["sift"]))
    assert "pairs[2]: the pair belongs to another context" in refused(S.E_INVALID, pairs=pin[:2] + [(foreign,) + dr.over[2]] + pin[3:])
    assert "another context" in refused(S.E_INVALID, context=other)
    # aliasing: an output on an input of a pair, of a link (the closing one too), on another output; d_report on an input, on an output
    assert "out.d_track overlaps links[4].d_index" in refused(S.E_INVALID, o=outs[:3] + (dr.indices[4],) + outs[4:])
    assert "out.d_flags overlaps pairs[4].d_valid" in refused(S.E_INVALID, o=outs[:8] + (dr.over[4][1].data_ptr() + 256,) + outs[9:])
    assert "out.d_cams overlaps links[0].d_sim" in refused(S.E_INVALID, o=outs[:2] + (dr.links[0][0].data_ptr() + 48,) + outs[3:])
    big = torch.full((8 * N,), -9, dtype=torch.int32, device=dev)
    assert "out.d_obs_record overlaps out.d_obs_cam" in refused(S.E_INVALID, o=outs[:5] + (big, big.data_ptr() + 8 * N - 4) + outs[7:])
    assert "d_report overlaps links[4].d_err" in refused(S.E_INVALID, r=dr.links[4][2].data_ptr() + 64)
    assert "d_report overlaps pairs[0].d_points" in refused(S.E_INVALID, r=dr.over[0][0])
    assert "d_report overlaps links[2].d_report" in refused(S.E_INVALID, r=dr.links[2][4])
    assert "d_report overlaps out.d_counts" in refused(S.E_INVALID, o=outs[:10] + (big,), r=big.data_ptr() + 16)
    assert "reserved" in refused(S.E_INVALID, p=S.fuse_ring_params(reserved=[0, 0, 0, 1]))
    assert "reserved" in refused(S.E_INVALID, p=S.fuse_ring_params(fuse_reserved=[0, 0, 0, 1]))
    assert "max_closure_rotation_rad" in refused(S.E_INVALID, p=S.fuse_ring_params(max_closure_rotation_rad=2.0))
    assert "max_closure_log_scale" in refused(S.E_INVALID, p=S.fuse_ring_params(max_closure_log_scale=-1.0))
    refused(S.E_INVALID, p=S.fuse_ring_params(max_iterations=51))
    # a missing refinement without both overrides
    assert "pairs[1]" in refused(S.E_STATE, pairs=pin[:1] + [dr.pairs[1]] + pin[2:])
    assert "pairs[4]" in refused(S.E_STATE, pairs=pin[:4] + [(dr.pairs[4], dr.over[4][0], dr.over[4][1], None)])
    bare = S.ImagePair(ctx, rg["K"], rg["Kinv"], 2, 257)                       # no points at all
    assert "pairs[2]" in refused(S.E_STATE, pairs=pin[:2] + [(bare,) + dr.over[2]] + pin[3:])
    assert untouched(outs, rep) and bool((big == -9).all())
    S.fuse_ring_enqueue(ctx, pin, links, params, outs, rep)                    # ... and the same buffers serve the valid call
    ctx.synchronize()
    assert not untouched(outs, rep) and int(outs[10][0]) == first["counts"]["tracks"] and report_of(rep) == first["report"]
    for p in (bare, foreign):
        p.close()
    other.close()
    dr.close()


def test_adjust_chain_over_the_ring_table(gpu, HL):
    """sfm_adjust_chain on the device over the device's ring table (k = 5 x 257, 10 iterations) against libchainadjustcheck over the
    host build's ring table: the seam tracks unused and returned bit for bit, everything else within 6i's device bars (equality)."""
    import test_gpu_chain_adjust as TA
    torch, dev, ctx = gpu
    sc, rg = ring(5, 257, 7)
    dr = DeviceRing(gpu, rg)
    k, N = dr.k, dr.N
    outs = S._fuse_buffers(torch, dev, k, N)
    rep = torch.empty(REPORT_BYTES, dtype=torch.uint8, device=dev)
    S.fuse_ring_enqueue(ctx, dr.pin(), dr.lin(), S.fuse_ring_params(), outs, rep)
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = outs
    fused = (root, cams, off, ocam, orec, pts, flags, counts)
    aouts = S.adjust_chain_buffers(dev, k, N)
    S.adjust_chain_enqueue(ctx, dr.pairs, fused, S.adjust_chain_params(max_iterations=10), aouts)
    ctx.synchronize()
    table = S._fuse_results(outs, k, N)
    T = table["counts"]["tracks"]
    got = S.adjust_chain_results(aouts, k, N, T)
    host_table = RS.run_host(HL, S, dr.host)
    res = {name: host_table[name] for name in ("root", "cams", "track_offset", "obs_cam", "obs_record", "points", "flags", "counts")}
    want = CS.run_host(CS.host_lib(), S, dr.host, CS.fused_arrays(res, k, N), max_iterations=10)
    seam = seam_tracks(table)
    assert seam.sum() == report_of(rep)["seam_tracks"] > 0 and not got["used"][seam].any()
    assert np.array_equal(u8(got["points"][:, seam]), u8(table["points"][:, seam]))
    assert np.array_equal(got["used"], want["used"]) and got["used"].sum() > 100
    for f in TA.INTEGERS:
        assert np.array_equal(got["reports"][f], want["reports"][f]), f
    d = TA.differences(got, want)
    print(f"adjust_chain over the ring table: {int(got['used'].sum())} used of {T} tracks, {int(seam.sum())} seam tracks; device - host build {d}")
    for q, bar in TA.BARS.items():
        assert d[q] <= bar, (q, d[q], bar)
    dr.close()


def test_full_ring_on_the_device(gpu, HL):
    """6 views on a 10-degree cone, n = 1024, 4096 hypotheses (test_gpu_ring's ring): fillXU -> estimateE -> refine_pairs -> ONE
    align_pairs over all six links -> close_ring -> fuse_ring over the corrected links, no overrides.  CLOSED; the device equals the
    host build and the structure the twin on the read-back state; how many of the features that fuse_chain holds twice across the
    seam are now one track; their points against the truth next to the midpoint of the two copies, held to 1.25 x the twin only
    where the twin shows the gain.  With the MEASURED links the ring is REJECTED and the bytes are fuse_chain's."""
    torch, dev, ctx = gpu
    k, n = 6, 1024
    sc = ring_scene.build(k, n, 61, pairs="all", cone_deg=10.0)
    made, _ = refined_chain(gpu, dict(sc, pairs=[sc["pairs"][v] for v in range(k)]), hyps=4096)
    idx = [to_dev(torch, dev, sc["index"][v]) for v in range(k)]
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, params.num_hypotheses) for p in made]
    S.align_pairs_enqueue(made, made[1:] + made[:1], idx, params, aouts)
    routs = S._ring_buffers(dev, k, n)
    S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], made[k - 1], S.ring_params(), routs)
    corrected = [(routs[0][13 * i:13 * i + 13], a[1], a[2], a[3], a[4]) for i, a in enumerate(aouts)]
    got = S.fuse_ring(made, idx, corrected)
    chain = S.fuse_chain(made, idx[:k - 1], corrected[:k - 1])
    ring_report = S._ring_results(routs, k, n)[3]
    assert ring_report["status"] == S.RING_CLOSED and got["report"]["status"] == S.RING_CLOSED, (ring_report, got["report"])
    state = read_back_chain(torch, made, idx, aouts, sc["K"], sc["Kinv"])
    links = routs[0].cpu().numpy().reshape(k, 13)
    state = dict(state, links=[dict(L, sim=links[i].copy()) for i, L in enumerate(state["links"])])
    host, twin = RS.run_host(HL, S, state), RR.fuse(state)
    print(f"full ring: {got['counts']}\n  {got['report']}\n  twin {twin['report']}")
    assert got["counts"] == host["counts"]
    for q in REPORT_INTS:
        assert got["report"][q] == host["report"][q], q
    for q in INTEGERS:
        assert np.array_equal(got[q], host[q]), q
    d = differences(got, host)
    print(f"  device against the host build {d}")
    for q, bar in BARS.items():
        assert d[q] <= bar, (q, d[q], bar)
    structure_equal(got, twin)
    band = np.abs(twin["err"] - 4.0) <= BAND * 4.0
    same = ~band
    scale = np.maximum(1.0, np.abs(twin["points"][2]))
    dp = (np.abs(got["points"].astype(np.float64) - twin["points"])[:3].max(0) / scale)[same].max()
    fin = np.isfinite(twin["err"]) & same
    de = (np.abs(got["err"][fin].astype(np.float64) - twin["err"][fin]) / np.maximum(1.0, twin["err"][fin])).max()
    print(f"  device against the twin: {band.sum()} of {len(band)} tracks within {BAND:.0%} of the threshold, points {dp:.3g} of the depth, err {de:.3g}")
    assert band.mean() <= BAND_CAP and np.array_equal(got["flags"][same], twin["flags"][same])
    assert dp <= POINTS_BAR and de <= ERR_BAR
    # the features fuse_chain holds twice across the seam (6j counted them): how many are one track now
    off = np.concatenate([[0], np.cumsum([P["n"] for P in state["pairs"]])]).astype(int)
    closing = state["links"][k - 1]
    twice = [(int(j), int(closing["index"][j])) for j in np.flatnonzero(closing["inlier"] != 0)
             if 0 <= closing["index"][j] < n and chain["track"][off[k - 1] + j] >= 0 and chain["track"][closing["index"][j]] >= 0
             and chain["track"][off[k - 1] + j] != chain["track"][closing["index"][j]]]
    once = sum(1 for j, m in twice if got["track"][off[k - 1] + j] == got["track"][m])
    print(f"  {len(twice)} features held twice across the seam by fuse_chain; {once} of them are one track now ({got['report']['seam_tracks']} seam "
          f"tracks, {got['report']['seam_ineligible']} ineligible proposals)")
    assert len(twice) >= 100 and once == got["report"]["seam_tracks"] > 0
    # their points against the truth (pair 0's frame: view 0's divided by pair 0's baseline), next to the midpoint of the two copies
    scene = dict(sc, pairs=sc["pairs"])
    twin_chain = FR.fuse(dict(state, links=state["links"][:k - 1]))
    n_t, one_t, two_t = seam_gain(scene, state, twin_chain, twin)
    n_d, one_d, two_d = seam_gain(scene, state, chain, got)
    print(f"  {n_d} clean refined ones: median distance to the truth, ring point {one_d:.4g} against midpoint {two_d:.4g}; twin ({n_t}) {one_t:.4g} "
          f"against {two_t:.4g}" + ("" if one_t < two_t else "   (the twin shows no gain: nothing asserted)"))
    if n_t >= 8 and one_t < two_t:
        assert n_d >= 8 and one_d <= 1.25 * one_t
    # the measured links: REJECTED, and every byte is fuse_chain's
    measured = [(a[0], a[1], a[2], a[3], a[4]) for a in aouts]
    a, rep = filled(torch, dev, k, k * n)
    b, _ = filled(torch, dev, k, k * n)
    S.fuse_ring_enqueue(ctx, made, [(idx[i], m[0], m[1], m[2], m[4]) for i, m in enumerate(measured)], S.fuse_ring_params(), a, rep)
    S.fuse_chain_enqueue(ctx, made, [(idx[i], m[0], m[1], m[2], m[4]) for i, m in enumerate(measured[:k - 1])], S.fuse_params(), b)
    ctx.synchronize()
    r = report_of(rep)
    print(f"  measured links: {r}")
    assert r["status"] == S.RING_REJECTED and r["seam_tracks"] == 0
    for x, y, field in zip(a, b, S.FuseOut._fields_):
        assert torch.equal(x, y), field[0]
    for p in made:
        p.close()
