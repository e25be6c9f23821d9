"""GPU: sfm_adjust_ring (csrc/ring_adjust.hip) through the C ABI -- every output and the report against the host build of the same
arithmetic (tests/hostcheck/libringadjustcheck.so) on the override path of tests/test_gpu_fuse_ring.py (DeviceRing), the device's
OWN sfm_fuse_ring table as input: rings of 3, 4 and 5 pairs of every block-edge size, a ragged ring, rings of 36 and 70 pairs
(a true band under the fold, the 192-row column at W = 16, more blocks than a wavefront has lanes), W = 3; the accept sequences;
degenerate and not-CLOSED rings into pattern-filled buffers; determinism, nothing in any pair changed, every refusal with nothing
written; the full six-view ring on the device against the host build and the fp64 twin (tests/ring_adjust_reference.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import fuse_ring_scene as RS
import ring_adjust_scene as RAS
import ring_scene
import fuse_scene as FS
from test_gpu_align import read_buffers
from test_gpu_fuse_ring import DeviceRing, REPORT_BYTES, u8

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
# Kernels against the host build at 10 iterations: the same header functions per lane and per track and fixed-order fp64 sums.  The
# bar on cameras, points, errors, rms and cost is equality (what 6f, 6h, 6i and 6k measured): a non-zero difference is
# a summation-order finding to fix, not a tolerance to set.
INTEGERS = ("ring_status", "status", "iterations", "accepted", "num_cameras", "num_tracks", "num_seam_tracks", "num_observations", "num_over_long")
FLOATS = ("initial_rms_px", "final_rms_px", "final_cost")
ADJ_BYTES = S.ADJUST_RING_REPORT_DTYPE.itemsize


@pytest.fixture(scope="module")
def HL():
    return RAS.host_lib()


@functools.lru_cache(maxsize=None)
def ring(k, n, seed=17):
    return RS.build(k, n, seed)


class Table:
    """The device's own sfm_fuse_ring table of a DeviceRing: the device tensors in the order sfm_adjust_ring_in takes them, and the
    same bytes read back as the host build's arrays."""

    def __init__(self, dr, **kw):
        torch, dev, ctx = dr.gpu
        self.dr, self.k, self.N = dr, dr.k, dr.N
        outs = S._fuse_buffers(torch, dev, dr.k, dr.N)
        for t in outs:
            t.zero_()                                                             # what lies behind the T tracks is compared too
        self.rep = torch.zeros(REPORT_BYTES, dtype=torch.uint8, device=dev)
        S.fuse_ring_enqueue(ctx, dr.pin(), dr.lin(), S.fuse_ring_params(**kw), outs, self.rep)
        ctx.synchronize()
        frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = outs
        self.fused = (root, cams, off, ocam, orec, pts, flags, counts, self.rep)
        self.T = int(counts[0].item())
        self.status = S.FuseRingReport.from_buffer_copy(self.rep.cpu().numpy().tobytes()).status

    def host_arrays(self, status=None):
        a = [t.cpu().numpy().copy() for t in self.fused]
        if status is not None:
            a[8] = RAS.ring_report_bytes(S, status)
        return a

    def with_status(self, status):
        """The device tensors with the report's status edited."""
        torch, dev, ctx = self.dr.gpu
        return self.fused[:8] + (to_dev(torch, dev, RAS.ring_report_bytes(S, status)),)


def filled(gpu, k, N, slack=64):
    """Output buffers of pattern bytes, `slack` elements longer than the call may write."""
    torch, dev, ctx = gpu
    f = lambda n, dt, v: torch.full((int(n) + slack,), v, dtype=dt, device=dev)
    return (f(24 * k, torch.float32, -3.0), f(4 * N, torch.float32, -3.0), f(N, torch.uint8, PATTERN), f(N, torch.float32, -3.0),
            f(ADJ_BYTES, torch.uint8, PATTERN))


def untouched(outs):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, -3.0, PATTERN, -3.0, PATTERN)))


def run_device(tab, fused=None, outs=None, **kw):
    torch, dev, ctx = tab.dr.gpu
    outs = outs if outs is not None else S.adjust_ring_buffers(dev, tab.k, tab.N)
    S.adjust_ring_enqueue(ctx, tab.dr.pairs, fused if fused is not None else tab.fused, S.adjust_ring_params(**kw), outs)
    ctx.synchronize()
    sizes = (24 * tab.k, 4 * tab.N, tab.N, tab.N, ADJ_BYTES)                     # (filled() buffers are longer)
    return S.adjust_ring_results([t[:n] for t, n in zip(outs, sizes)], tab.k, tab.N, tab.T)


def differences(got, want):
    f = lambda a: np.asarray(a, np.float64)
    d = {q: float(np.abs(f(got[q]) - f(want[q])).max()) if got[q].size else 0.0 for q in ("cams", "points")}
    fin = np.isfinite(want["err"]) & np.isfinite(got["err"])
    d["err"] = float(np.abs(f(got["err"])[fin] - f(want["err"])[fin]).max()) if fin.any() else 0.0
    for q in FLOATS:
        d[q] = abs(float(got["report"][q]) - float(want["report"][q]))
    return d


def check_against_host(HL, tab, what, iterations=(0, 10), **kw):
    """d_used, the report's integers and lambda equal; at 0 iterations every output byte equal; at 10 the bar is equality as well,
    the measured maxima printed first."""
    for iters in iterations:
        got = run_device(tab, max_iterations=iters, **kw)
        want = RAS.run_host(HL, S, tab.dr.host, tab.host_arrays(), max_iterations=iters, **kw)
        assert want["band"], (what, "a non-zero block outside the folded band")
        assert np.array_equal(got["used"], want["used"]), (what, iters)
        for q in INTEGERS:
            assert got["report"][q] == want["report"][q], (what, iters, q, got["report"], want["report"])
        assert np.float32(got["report"]["lambda"]).tobytes() == np.float32(want["report"]["lambda"]).tobytes(), (what, iters)
        assert np.array_equal(np.isinf(got["err"]), np.isinf(want["err"])), (what, iters)
        d = differences(got, want)
        print(f"adjust ring {what}, {iters} iterations: {got['report']}; device - host build {d}")
        assert max(d.values()) == 0.0, (what, iters, d)
        for q in ("cams", "points", "err"):
            assert np.array_equal(u8(got[q]), u8(want[q])), (what, iters, q)
        assert got["report"].tobytes() == want["report"].tobytes(), (what, iters)
        # one camera per view
        cams = got["cams"]
        for p in range(tab.k - 1):
            assert cams[p + 1, 0].tobytes() == cams[p, 1].tobytes(), p
        assert cams[tab.k - 1, 1].tobytes() == cams[0, 0].tobytes()
    return got


@pytest.mark.parametrize("n", [63, 64, 65, 257])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_override_path_against_the_host_build(gpu, HL, k, n):
    sc, rg = ring(k, n)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    assert tab.status == S.RING_CLOSED
    got = check_against_host(HL, tab, f"k={k} n={n}")
    assert got["report"]["num_cameras"] == k - 1 and got["report"]["ring_status"] == S.RING_CLOSED
    if n >= 257:
        assert got["report"]["status"] != S.REFINE_DEGENERATE and got["report"]["num_seam_tracks"] > 0 and got["report"]["iterations"] > 0
    dr.close()


@pytest.mark.parametrize("k,n,seed,W", [(36, 65, 3, 8), (36, 65, 3, 16), (70, 65, 3, 8), (6, 257, 7, 3)])
def test_long_rings_and_narrow_tracks_against_the_host_build(gpu, HL, k, n, seed, W):
    """(36, 65, 3): a true band under the fold (16 and 32 of 35 block diagonals; at W = 16 a column of the factor has 192 rows);
    (70, 65, 3): more blocks than a wavefront has lanes; W = 3 on six pairs: 240 over-long tracks."""
    sc, rg = ring(k, n, seed)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    got = check_against_host(HL, tab, f"k={k} n={n} W={W}", max_track_views=W)
    rep = got["report"]
    assert rep["status"] != S.REFINE_DEGENERATE and rep["iterations"] == 10 and rep["final_rms_px"] < rep["initial_rms_px"]
    assert rep["num_seam_tracks"] > 0 and rep["num_over_long"] > 0
    dr.close()


def test_ragged_ring_against_the_host_build(gpu, HL):
    sc, rg = ring(5, 257, 7)
    dr = DeviceRing(gpu, RS.truncated(rg, [65, 257, 64, 257, 1]))
    check_against_host(HL, Table(dr), "ragged 65/257/64/257/1")
    dr.close()


def test_accept_sequences_equal_the_host_builds(gpu, HL):
    """Calls with 1 .. 10 iterations on (6, 257, 7): iterations, accepted, status and lambda after every one of them, and the
    sequence they spell, equal the host build's."""
    sc, rg = ring(6, 257, 7)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    full = RAS.run_host(HL, S, dr.host, tab.host_arrays(), max_iterations=10)
    seq, last = [], 0
    for i in range(1, 11):
        got = run_device(tab, max_iterations=i)["report"]
        want = RAS.run_host(HL, S, dr.host, tab.host_arrays(), max_iterations=i)["report"]
        assert got.tobytes() == want.tobytes(), (i, got, want)
        if got["iterations"] == i:
            seq.append(1 if got["accepted"] > last else 2)
        last = got["accepted"]
    host_seq = [int(x) for x in full["accepts"][:full["report"]["iterations"]]]
    print(f"accepts: device {seq}, host build {host_seq}")
    assert [2 if s == 3 else s for s in host_seq] == seq                       # (a failed solve shows as an iteration without a commit)
    dr.close()


def _returned_bit_for_bit(tab, outs, used_zero):
    k, N, T = tab.k, tab.N, tab.T
    cams_in, pts_in = tab.fused[1].cpu().numpy(), tab.fused[5].cpu().numpy().reshape(4, N)
    cams, pts, used, err, rep = (t.cpu().numpy() for t in outs)
    assert cams[:24 * k].tobytes() == cams_in.tobytes()
    assert pts[:4 * N].reshape(4, N)[:, :T].tobytes() == np.ascontiguousarray(pts_in[:, :T]).tobytes()
    if used_zero:
        assert not used[:T].any()
    # nothing written behind the outputs, or behind the T tracks
    assert (cams[24 * k:] == -3.0).all() and (pts[4 * N:] == -3.0).all() and (used[N:] == PATTERN).all() and (err[N:] == -3.0).all()
    assert (rep[ADJ_BYTES:] == PATTERN).all() and (used[T:N] == PATTERN).all() and (err[T:N] == -3.0).all()
    assert (pts[:4 * N].reshape(4, N)[:, T:] == -3.0).all()
    return rep[:ADJ_BYTES].view(S.ADJUST_RING_REPORT_DTYPE)[0]


def test_degenerate_ring_returns_its_inputs(gpu, HL):
    sc, rg = ring(36, 65, 3)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    outs = filled(gpu, tab.k, tab.N)
    got = run_device(tab, outs=outs, max_track_views=3)
    rep = _returned_bit_for_bit(tab, outs, used_zero=False)
    want = RAS.run_host(HL, S, dr.host, tab.host_arrays(), max_track_views=3)
    assert rep["status"] == S.REFINE_DEGENERATE and rep["iterations"] == 0 and rep["ring_status"] == S.RING_CLOSED
    assert rep.tobytes() == want["report"].tobytes() and np.array_equal(got["used"], want["used"]) and np.array_equal(u8(got["err"]), u8(want["err"]))
    dr.close()


@pytest.mark.parametrize("k", [3, 65])
def test_not_closed_rings_return_their_inputs(gpu, HL, k):
    """A report edited to OPEN and to REJECTED, and a genuinely REJECTED fusion (the gates narrowed): inputs bit for bit, d_used
    zero, the report the ring status and zeros, nothing written behind the outputs."""
    sc, rg = ring(k, 65, 3)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    assert tab.status == S.RING_CLOSED
    cases = [("edited OPEN", tab, tab.with_status(S.RING_OPEN), S.RING_OPEN), ("edited REJECTED", tab, tab.with_status(S.RING_REJECTED), S.RING_REJECTED)]
    turned = ring_scene.compose((1.0, ring_scene.rodrigues([0.0, 5e-3, 0.0]), np.zeros(3)), ring_scene.unpack(rg["links"][k - 1]["sim"]))
    broken = dict(rg, links=[dict(L, sim=FS.sim13(*turned)) if q == k - 1 else L for q, L in enumerate(rg["links"])])
    dr2 = DeviceRing(gpu, broken)
    tab2 = Table(dr2)
    assert tab2.status == S.RING_REJECTED
    cases.append(("REJECTED fusion", tab2, tab2.fused, S.RING_REJECTED))
    for name, tb, fused, status in cases:
        outs = filled(gpu, tb.k, tb.N)
        got = run_device(tb, fused=fused, outs=outs)
        rep = _returned_bit_for_bit(tb, outs, used_zero=True)
        assert rep["ring_status"] == status and all(rep[f] == 0 for f in rep.dtype.names if f != "ring_status"), (name, rep)
        arrays = [t.cpu().numpy().copy() for t in fused]
        want = RAS.run_host(HL, S, tb.dr.host, arrays)
        assert rep.tobytes() == want["report"].tobytes() and np.array_equal(u8(got["err"]), u8(want["err"])), name
    dr.close()
    dr2.close()


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    sc, rg = ring(5, 257, 7)
    dr = DeviceRing(gpu, rg)
    tab = Table(dr)
    before = [read_buffers(p, ctx) for p in dr.pairs]
    first, second = run_device(tab), run_device(tab)
    assert first["report"]["iterations"] > 0 and first["report"]["num_seam_tracks"] > 0
    for key in first:
        assert np.array_equal(u8(first[key]), u8(second[key])), key
    for p, bufs in zip(dr.pairs, before):                                      # every SFM_BUF_* of every pair
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    k, N = tab.k, tab.N
    outs = filled(gpu, k, N)
    params = S.adjust_ring_params()
    fused, pairs = tab.fused, dr.pairs

    def refused(code, pr=pairs, f=fused, p=params, o=outs, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.adjust_ring_enqueue(context, pr, f, p, o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    # each argument
    assert "null" in refused(S.E_INVALID, context=None)
    assert "null" in refused(S.E_INVALID, f=None)
    assert "null" in refused(S.E_INVALID, o=None)
    assert "null params" in refused(S.E_INVALID, p=None)
    for i in range(9):
        assert "required" in refused(S.E_INVALID, f=fused[:i] + (None,) + fused[i + 1:])
    for i in (0, 1, 2, 4):
        assert "required" in refused(S.E_INVALID, o=outs[:i] + (None,) + outs[i + 1:])
    assert "3..4096" in refused(S.E_INVALID, pr=pairs[:2])                     # k = 2
    assert "max_track_views" in refused(S.E_INVALID, p=S.adjust_ring_params(max_track_views=1))
    assert "max_track_views" in refused(S.E_INVALID, p=S.adjust_ring_params(max_track_views=17))
    refused(S.E_INVALID, p=S.adjust_ring_params(max_iterations=51))
    assert "reserved" in refused(S.E_INVALID, p=S.adjust_ring_params(reserved=[0, 0, 1, 0]))
    assert "pairs[3]: null pair" in refused(S.E_INVALID, pr=pairs[:3] + [None] + pairs[4:])
    assert "pairs[3]: the pair is listed twice" in refused(S.E_INVALID, pr=pairs[:3] + [pairs[1]] + pairs[4:])
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, rg["K"], rg["Kinv"], 2, 257)
    foreign.fillXU(to_dev(torch, dev, rg["pairs"][2]["sift"]))
    assert "pairs[2]: the pair belongs to another context" in refused(S.E_INVALID, pr=pairs[:2] + [foreign] + pairs[3:])
    bare = S.ImagePair(ctx, rg["K"], rg["Kinv"], 2, 257)                       # the points stage is missing
    assert "pairs[2]" in refused(S.E_STATE, pr=pairs[:2] + [bare] + pairs[3:])
    # overlaps: an output on an input, on another output, on the ring report; the ring report on an output
    assert "out.d_cams overlaps in.d_cams" in refused(S.E_INVALID, o=(fused[1],) + outs[1:])
    assert "out.d_points overlaps in.d_points" in refused(S.E_INVALID, o=outs[:1] + (fused[5].data_ptr() + 16,) + outs[2:])
    assert "out.d_used overlaps in.d_flags" in refused(S.E_INVALID, o=outs[:2] + (fused[6],) + outs[3:])
    big = torch.full((8 * N,), -3.0, dtype=torch.float32, device=dev)
    text = refused(S.E_INVALID, o=outs[:1] + (big, outs[2], big.data_ptr() + 16 * N - 4) + outs[4:])
    assert "out.d_err" in text and "out.d_points" in text and "overlaps" in text
    assert "out.d_report overlaps in.d_ring_report" in refused(S.E_INVALID, o=outs[:4] + (tab.rep,))
    assert "out.d_report overlaps in.d_ring_report" in refused(S.E_INVALID, f=fused[:8] + (outs[4].data_ptr() + 8,))
    assert "out.d_cams overlaps in.d_ring_report" in refused(S.E_INVALID, f=fused[:8] + (outs[0].data_ptr() + 64,))
    assert untouched(outs) and bool((big == -3.0).all())
    S.adjust_ring_enqueue(ctx, pairs, fused, params, outs)                     # ... and the same buffers serve the valid call
    ctx.synchronize()
    assert not untouched(outs)
    assert outs[4].cpu().numpy()[:ADJ_BYTES].tobytes() == first["report"].tobytes()
    for p in (bare, foreign):
        p.close()
    other.close()
    dr.close()


def test_full_ring_on_the_device(gpu, HL):
    """6j's six-view cone ring, n = 1024, 4096 hypotheses: fillXU -> estimateE -> refine_pairs -> ONE align_pairs over all six links
    -> close_ring -> fuse_ring over the corrected links -> adjust_ring, no overrides.  The device equals the host build on the
    read-back state; the rms falls; the twin on the same state is printed and held to the noisy-ring bars; the seam features'
    median distance to the truth is printed next to 6k's 0.007314 and asserted (1.25 x the twin) only where the twin shows a gain;
    sfm_adjust_chain on the same table is printed next to it."""
    import ring_adjust_reference as RR
    from test_gpu_align import chain as refined_chain
    from test_gpu_fuse import read_back_chain
    import chain_adjust_scene as CS
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
    N = k * n
    fouts = S._fuse_buffers(torch, dev, k, N)
    for t in fouts:
        t.zero_()
    frep = torch.zeros(REPORT_BYTES, dtype=torch.uint8, device=dev)
    S.fuse_ring_enqueue(ctx, made, [(idx[i], routs[0][13 * i:13 * i + 13], a[1], a[2], a[4]) for i, a in enumerate(aouts)], S.fuse_ring_params(), fouts, frep)
    got = S.adjust_ring(made, fouts, frep)
    frames, root, cams, track, off, ocam, orec, pts, flags, err, counts = fouts
    table = (root, cams, off, ocam, orec, pts, flags, counts)
    T = int(counts[0].item())
    couts = S.adjust_chain_buffers(dev, k, N)
    S.adjust_chain_enqueue(ctx, made, table, S.adjust_chain_params(), couts)
    ctx.synchronize()
    chain = S.adjust_chain_results(couts, k, N, T)
    rep = got["report"]
    assert rep["ring_status"] == S.RING_CLOSED and rep["status"] != S.REFINE_DEGENERATE and rep["num_seam_tracks"] > 100, rep
    state = read_back_chain(torch, made, idx, aouts, sc["K"], sc["Kinv"])
    arrays = [t.cpu().numpy().copy() for t in table] + [frep.cpu().numpy().copy()]
    host = RAS.run_host(HL, S, state, arrays)
    d = differences(got, host)
    print(f"full ring: {rep}\n  device - host build {d}\n  sfm_adjust_chain on the same table: {chain['reports'][0]}")
    assert host["band"] and np.array_equal(got["used"], host["used"]) and got["report"].tobytes() == host["report"].tobytes()
    assert max(d.values()) == 0.0, d
    assert rep["final_rms_px"] < rep["initial_rms_px"]
    res = S._fuse_results(fouts, k, N)
    twin = RR.adjust_ring(state["pairs"], state["K"], res)
    rt = twin["report"]
    cm = got["cams"].astype(np.float64)
    drot = max(CS.rotation_angle(cm[p, 1, :9], twin["cams"][p, 1, :9]) for p in range(k - 1))
    dt = max(float(np.abs(cm[p, 1, 9:] - twin["cams"][p, 1, 9:]).max() / max(1.0, np.linalg.norm(twin["cams"][p, 1, 9:]))) for p in range(k - 1))
    drms = abs(float(rep["final_rms_px"]) - rt["final_rms_px"])
    print(f"  twin {rt}\n  device - twin: rot {drot:.3g} rad, t / |t| {dt:.3g}, rms {drms:.3g} px")
    assert np.array_equal(got["used"] != 0, twin["used"]) and rep["num_tracks"] == rt["num_tracks"] and rep["num_seam_tracks"] == rt["num_seam_tracks"]
    assert drot <= 1e-4 and dt <= 1e-3 and drms <= 1e-4
    # the seam features against the truth (pair 0's frame), before and after, next to 6k's 0.007314
    seam = np.flatnonzero((got["used"] != 0) & (res["flags"] == S.FUSE_SEAM_REFINED))
    feats, clean = [], []
    for t in seam:
        o = np.arange(res["track_offset"][t], res["track_offset"][t + 1] - 1)
        ids = {RS.feature(sc, int(res["obs_cam"][q]) >> 1, int(res["obs_record"][q])) for q in o}
        feats.append(RS.feature(sc, int(res["obs_cam"][o[0]]) >> 1, int(res["obs_record"][o[0]])))
        clean.append(len(ids) == 1 and all(sc["pairs"][int(res["obs_cam"][q]) >> 1]["good"][int(res["obs_record"][q])] for q in o))
    clean = np.array(clean, bool)
    truth = RS.truth_in_pair0(sc, feats)
    dist = lambda p: float(np.median(np.linalg.norm(np.asarray(p, np.float64)[:3, seam].T - truth, axis=1)[clean]))
    before, after_d, after_t, after_c = dist(res["points"]), dist(got["points"]), dist(twin["points"]), dist(chain["points"])
    print(f"  {int(clean.sum())} clean seam features: median distance to the truth {before:.4g} (6k: 0.007314) -> device {after_d:.4g}, twin {after_t:.4g}; "
          f"after sfm_adjust_chain (which leaves them alone) {after_c:.4g}" + ("" if after_t < before else "   (the twin shows no gain: nothing asserted)"))
    if clean.sum() >= 8 and after_t < before:
        assert after_d <= 1.25 * after_t
    for p in made:
        p.close()
