"""GPU: sfm_close_ring (csrc/ring.hip) through the C ABI -- every output against the host build of the same arithmetic
(tests/hostcheck/libringcheck.so) on the override path (a last pair that only has fillXU): rings of 3 .. 257 links, last pairs of
1 .. 1025 records, CLOSED / OPEN / REJECTED, default and supplied weights; determinism, nothing in the pair changed, every refusal
with nothing written; the full ring of six views on the device against the host build and the fp64 twins, its corrected links
fused by sfm_fuse_chain."""
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import fuse_reference as FR
import fuse_scene as FS
import ring_reference as RF
import ring_scene as RS
from test_gpu_align import chain as refined_chain, read_buffers
from test_gpu_fuse import read_back_chain
from test_ring_host import RECOMPOSED_MEASURED, bars, sim_diff, worst_of

pytestmark = pytest.mark.gpu
LINKS = [3, 4, 5, 63, 64, 65, 257]                     # 257: two rounds of the walk, the seam of the walk inside the ring
RECORDS = [1, 63, 64, 65, 257, 1025]                   # of the last pair: 257 is two blocks of the seam kernel, 1025 five
# Kernels against the host build: the same header functions per link and per record, the seam's sums in the same order.  What can
# differ is fp64 sin, cos, exp, log and atan2 of the two builds, before the one rounding to fp32.
# MEASURED: the largest absolute difference over every case below on the MI355X in the links, the frames, the seam errors and the
# report's floats.  Every one is 0, so the bars, 4 x the measured maximum, are equality.
MEASURED = dict(links=0.0, frames=0.0, seam=0.0, report=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}
INTEGERS = ("status", "num_links", "first_invalid", "seam_count", "seam_lost_open", "seam_lost_closed")
FLOATS = ("drift_log_scale", "drift_rotation_rad", "drift_t", "seam_rms_link_px", "seam_rms_open_px", "seam_rms_closed_px")
PATTERN = 0xA5


@pytest.fixture(scope="module")
def HL():
    return RS.host_lib()


@functools.lru_cache(maxsize=None)
def ring(k, n, seed=21):
    """The scene and one call's input: the true links, each with a tenth of the host tests' drift (a seam with members)."""
    sc = RS.build(k, n, seed)
    sims = RS.perturbed(sc["sims"], RS.small_similarities(k, seed + 1, rot=2e-4, scale=1e-3, trans=1e-3))
    return sc, RS.ring_input(sc, sims=sims)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


class DeviceRing:
    """One call's input on the device on the override path: the last pair only has fillXU; its points and flags and the links'
    similarities and reports are uploaded.  `host` is the same input over the device's OWN normalised observations."""

    def __init__(self, gpu, sc, inp):
        torch, dev, ctx = gpu
        d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
        L = inp["last"]
        self.ctx, self.k, self.n = ctx, inp["k"], L["n"]
        self.pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, L["n"])
        self.pair.fillXU(to_dev(torch, dev, L["sift"]))
        self.over = (d(L["points"]), d(L["valid"]))
        self.sims = d(inp["sims"].ravel())
        reps = np.zeros((self.k, S.C.sizeof(S.AlignReport)), np.uint8)
        for i in range(self.k):
            r = S.AlignReport(); r.status = int(inp["status"][i]); r.num_inliers = int(inp["inliers"][i])
            reps[i] = np.frombuffer(bytes(r), np.uint8)
        self.reports = d(reps.ravel())
        self.links = [(self.sims[13 * i:13 * i + 13], self.reports[reps.shape[1] * i:reps.shape[1] * (i + 1)]) for i in range(self.k)]
        self.host = dict(inp, last=dict(L, X1=self.pair.get_XU(S.BUF_X1), ld=L["n"]))

    def run(self, **kw):
        return S.close_ring(self.pair, self.links, override=self.over, **kw)

    def close(self):
        self.pair.close()


def differences(got, want):
    f = lambda a: np.asarray(a, np.float64)
    d = {}
    for q, a, b in (("links", got[0], want[0]), ("frames", got[1], want[1])):  # an OPEN ring returns its links, a NaN included
        fin = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(u8(a[~fin]), u8(b[~fin])), q
        d[q] = float(np.abs(f(a)[fin] - f(b)[fin]).max())
    fin = np.isfinite(want[2]) & np.isfinite(got[2])
    d["seam"] = float(np.abs(f(got[2])[fin] - f(want[2])[fin]).max()) if fin.any() else 0.0
    d["report"] = max(abs(float(got[3][q]) - float(want[3][q])) for q in FLOATS)
    return d


def check_against_host(HL, dr, what, worst=None, **kw):
    """Integers byte for byte, the floats within BARS (the same bytes where the bars are 0).  Returns the device's result."""
    got = dr.run(**kw)
    want = RS.run_host(HL, S, dr.host, **kw)
    for q in INTEGERS:
        assert got[3][q] == want[3][q], (what, q, got[3], want[3])
    assert np.array_equal(np.isinf(got[2]), np.isinf(want[2])) and not np.isnan(got[2]).any(), what
    d = differences(got, want)
    print(f"ring {what}: {got[3]}; differences {d}")
    for q, bar in BARS.items():
        assert d[q] <= bar, (what, q, d[q], bar)
    if max(BARS.values()) == 0.0:
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(u8(a), u8(b)), what
    if worst is not None:
        worst.update({q: max(worst.get(q, 0.0), d[q]) for q in d})
    return got


@pytest.mark.parametrize("k", LINKS)
def test_rings_of_every_length_against_the_host_build(gpu, HL, k):
    sc, inp = ring(k, 65)
    dr = DeviceRing(gpu, sc, inp)
    got = check_against_host(HL, dr, f"k={k} n=65")
    assert got[3]["status"] == S.RING_CLOSED and got[3]["num_links"] == k and got[3]["seam_count"] > 0
    w = np.random.default_rng(k).uniform(0.0, 1.0, k).astype(np.float32)
    w[::3] = 0.0; w[1] = 1.0
    given = check_against_host(HL, dr, f"k={k} n=65, supplied weights", weights=w)
    assert given[3]["status"] == S.RING_CLOSED and not np.array_equal(u8(given[0]), u8(got[0]))
    assert np.array_equal(u8(given[1][0]), u8(got[1][0]))                      # F'_0 = I whatever the weights
    dr.close()


@pytest.mark.parametrize("n", RECORDS)
def test_last_pairs_of_every_size_against_the_host_build(gpu, HL, n):
    sc, inp = ring(5, n)
    dr = DeviceRing(gpu, sc, inp)
    got = check_against_host(HL, dr, f"k=5 n={n}")
    assert got[3]["status"] == S.RING_CLOSED and got[2].shape == (3, n)
    usable = RF.pixel_errors(sc["K"], RF.IDENTITY, dr.host["last"]["points"], dr.host["last"]["valid"], dr.host["last"]["X1"], n, 4.0)[0]
    assert not np.isfinite(got[2][:, ~usable]).any()                           # +inf where the record is not usable
    loose = check_against_host(HL, dr, f"k=5 n={n}, 40 px", threshold_px=40.0)
    assert loose[3]["seam_count"] >= got[3]["seam_count"]
    dr.close()


@pytest.mark.parametrize("k", [3, 65, 257])
def test_open_and_rejected_rings_return_their_links(gpu, HL, k):
    sc, inp = ring(k, 65)
    nan_t = inp["sims"].copy(); nan_t[k - 2, 11] = np.nan
    zero_s = inp["sims"].copy(); zero_s[0, 0] = 0.0
    degenerate = np.where(np.arange(k) == k - 1, S.REFINE_DEGENERATE, 0).astype(np.int32)
    for what, change, first in (("NaN in t", dict(sims=nan_t), k - 2), ("s = 0", dict(sims=zero_s), 0), ("degenerate", dict(status=degenerate), k - 1)):
        bad = dict(inp, **change)
        dr = DeviceRing(gpu, sc, bad)
        got = check_against_host(HL, dr, f"k={k} open ({what})")
        assert got[3]["status"] == S.RING_OPEN and got[3]["first_invalid"] == first
        assert np.array_equal(u8(got[0]), u8(bad["sims"])) and np.array_equal(u8(got[2][1]), u8(got[2][2]))
        dr.close()
    turned = RS.perturbed(inp["sims"], [None, (1.0, RS.rodrigues([0.0, 0.4, 0.0]), np.zeros(3))] + [None] * (k - 2))
    scaled = RS.perturbed(inp["sims"], [None] * (k - 1) + [(0.45, np.eye(3), np.zeros(3))])
    for what, sims in (("rotation", turned), ("scale", scaled)):
        dr = DeviceRing(gpu, sc, dict(inp, sims=sims))
        got = check_against_host(HL, dr, f"k={k} rejected ({what})")
        assert got[3]["status"] == S.RING_REJECTED and got[3]["first_invalid"] == -1
        assert np.array_equal(u8(got[0]), u8(sims)) and np.array_equal(u8(got[2][1]), u8(got[2][2]))
        wide = check_against_host(HL, dr, f"k={k} wider gates ({what})", max_rotation_rad=0.5, max_log_scale=1.0)
        assert wide[3]["status"] == S.RING_CLOSED
        dr.close()


def filled(torch, dev, k, n):
    f = lambda m, dt, v: torch.full((int(m),), v, dtype=dt, device=dev)
    return (f(13 * k, torch.float32, -3.0), f(13 * k, torch.float32, -3.0), f(3 * n, torch.float32, -3.0),
            f(S.C.sizeof(S.RingReport), torch.uint8, PATTERN))


def untouched(outs):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, -3.0, -3.0, PATTERN)))


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    k, n = 65, 257
    sc, inp = ring(k, n)
    dr = DeviceRing(gpu, sc, inp)
    before = read_buffers(dr.pair, ctx)
    first, second = dr.run(), dr.run()
    assert first[3] == second[3] and first[3]["status"] == S.RING_CLOSED and first[3]["seam_count"] > 100
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(u8(a), u8(b))
    for which, (a, b) in enumerate(zip(before, read_buffers(dr.pair, ctx))):   # every SFM_BUF_* of the pair
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    outs = filled(torch, dev, k, n)
    params = S.ring_params()
    last = (dr.pair,) + dr.over

    def refused(code, lk=dr.links, pair=last, p=params, o=outs, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.close_ring_enqueue(context, lk, pair, p, o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    assert "num_links 2 outside 3..4096" in refused(S.E_INVALID, lk=dr.links[:2])
    assert "links[7]: d_sim and d_report are required" in refused(S.E_INVALID, lk=dr.links[:7] + [(dr.links[7][0], None)] + dr.links[8:])
    assert "last_pair: null pair" in refused(S.E_INVALID, pair=(None, None, None))
    assert "last_pair: d_valid needs d_points" in refused(S.E_INVALID, pair=(dr.pair, None, dr.over[1]))
    assert "every buffer of sfm_ring_out but d_seam_err is required" in refused(S.E_INVALID, o=(outs[0], None, outs[2], outs[3]))
    assert "reserved" in refused(S.E_INVALID, p=S.ring_params(reserved=[1, 0, 0, 0]))
    assert "max_rotation_rad" in refused(S.E_INVALID, p=S.ring_params(max_rotation_rad=1.6))
    assert "max_log_scale" in refused(S.E_INVALID, p=S.ring_params(max_log_scale=0.0))
    assert "threshold_px" in refused(S.E_INVALID, p=S.ring_params(threshold_px=-1.0))
    assert "links[4]: its weight" in refused(S.E_INVALID, p=S.ring_params(weights=[1.0] * 4 + [-1.0] + [1.0] * (k - 5)))
    assert "positive sum" in refused(S.E_INVALID, p=S.ring_params(weights=[0.0] * k))
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, sc["K"], sc["Kinv"], 2, n)
    foreign.fillXU(to_dev(torch, dev, inp["last"]["sift"]))
    assert "last_pair: the pair belongs to another context" in refused(S.E_INVALID, pair=(foreign,) + dr.over)
    assert "another context" in refused(S.E_INVALID, context=other)
    # aliasing: an output on a link's input, on the pair's input, on another output
    assert "out.d_links overlaps links[2].d_sim" in refused(S.E_INVALID, o=(dr.links[2][0].data_ptr() + 48,) + outs[1:])
    assert "out.d_frames overlaps links[64].d_report" in refused(S.E_INVALID, o=(outs[0], dr.links[64][1]) + outs[2:])
    assert "out.d_seam_err overlaps last_pair.d_points" in refused(S.E_INVALID, o=outs[:2] + (dr.over[0].data_ptr() + 16 * n - 4, outs[3]))
    assert "out.d_report overlaps last_pair.d_valid" in refused(S.E_INVALID, o=outs[:3] + (dr.over[1].data_ptr() + n - 1,))
    big = torch.full((26 * k,), -3.0, dtype=torch.float32, device=dev)
    assert "out.d_frames overlaps out.d_links" in refused(S.E_INVALID, o=(big, big.data_ptr() + 52 * k - 4) + outs[2:])
    # a missing refinement without d_points; no points at all
    assert "last_pair: " in refused(S.E_STATE, pair=(dr.pair, None, None))
    bare = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    assert "last_pair: no points yet" in refused(S.E_STATE, pair=(bare,) + dr.over)
    assert untouched(outs) and bool((big == -3.0).all())
    S.close_ring_enqueue(ctx, dr.links, last, params, outs)                    # ... and the same buffers serve the valid call
    ctx.synchronize()
    assert not untouched(outs)
    got = S._ring_results(outs, k, n)
    assert got[3] == first[3] and all(np.array_equal(u8(a), u8(b)) for a, b in zip(got[:3], first[:3]))
    S.close_ring_enqueue(ctx, dr.links, last, params, outs[:2] + (None, outs[3]))     # d_seam_err is optional
    ctx.synchronize()
    for p in (bare, foreign):
        p.close()
    other.close()
    dr.close()


def seam_gap(res, pairs, link, k):
    """Per feature seen across the seam (an inlier of the closing link whose two records both carry a track): the distance between
    the track fused at the chain's end (record j of pair k - 1) and the one fused at its start (record index[j] of pair 0), relative
    to the depth in pair 0's frame."""
    off = np.concatenate([[0], np.cumsum([P["n"] for P in pairs])]).astype(int)
    out = []
    for j in np.flatnonzero(link["inlier"] != 0):
        m = int(link["index"][j])
        a, b = res["track"][off[k - 1] + j], res["track"][off[0] + m]
        if a >= 0 and b >= 0 and a != b:
            Xa, Xb = res["points"][:3, a].astype(np.float64), res["points"][:3, b].astype(np.float64)
            out.append(np.linalg.norm(Xa - Xb) / Xb[2])
    return np.array(out)


def test_full_ring_on_the_device(gpu, HL):
    """6 views, n = 1024: fillXU -> estimateE -> refine_pairs -> ONE align_pairs over all six links -> close_ring, then fuse_chain
    with the measured and with the corrected first five links.  The device equals the host build; what the closure gains is held
    to the twins on the read-back state, never to the truth (6g's gauge argument)."""
    torch, dev, ctx = gpu
    k, n = 6, 1024
    sc = RS.build(k, n, 61, pairs="all", cone_deg=10.0)                        # neighbours 10 degrees and one baseline apart, as in 6g's and 6h's chains
    # 4096 hypotheses: at 1024 estimateE leaves two of this ring's six links degenerate and the ring OPEN (seeds 61 .. 66 tried: 6j)
    made, _ = refined_chain(gpu, dict(sc, pairs=[sc["pairs"][v] for v in range(k)]), hyps=4096)
    idx = [to_dev(torch, dev, sc["index"][v]) for v in range(k)]
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, params.num_hypotheses) for p in made]
    S.align_pairs_enqueue(made, made[1:] + made[:1], idx, params, aouts)
    outs = S._ring_buffers(dev, k, n)
    S.close_ring_enqueue(ctx, [(a[0], a[4]) for a in aouts], made[k - 1], S.ring_params(), outs)
    ctx.synchronize()
    got = S._ring_results(outs, k, n)
    # the read-back state: what the call read
    state = read_back_chain(torch, made, idx, aouts, sc["K"], sc["Kinv"])
    inliers = [S.AlignReport.from_buffer_copy(a[4].cpu().numpy().tobytes()).num_inliers for a in aouts]
    inp = dict(k=k, K=sc["K"], sims=np.stack([L["sim"] for L in state["links"]]), status=np.array([L["status"] for L in state["links"]], np.int32),
               inliers=np.array(inliers, np.int32), last=state["pairs"][k - 1])
    host, twin = RS.run_host(HL, S, inp), RF.close_ring(inp)
    print(f"full ring: {got[3]}\n  twin {twin['report']}\n  links " + ", ".join(f"status {L['status']} s {L['sim'][0]:.4f} {c} inliers" for L, c in zip(state["links"], inliers)))
    assert got[3]["status"] == S.RING_CLOSED
    for q in INTEGERS:
        assert got[3][q] == host[3][q], q
    d = differences(got, host)
    print(f"  device against the host build {d}")
    for q, bar in BARS.items():
        assert d[q] <= bar, (q, d[q], bar)
    if twin["report"]["seam_rms_closed_px"] < twin["report"]["seam_rms_open_px"]:
        assert got[3]["seam_rms_closed_px"] < got[3]["seam_rms_open_px"]
    # sfm_fuse_chain over the first five links: measured, then corrected
    corrected = [(outs[0][13 * i:13 * i + 13], a[1], a[2], a[3], a[4]) for i, a in enumerate(aouts[:k - 1])]
    fused_open, fused = S.fuse_chain(made, idx[:k - 1], aouts[:k - 1]), S.fuse_chain(made, idx[:k - 1], corrected)
    re = worst_of(zip(fused["frames"], got[1]))
    print(f"  fuse_chain's frames from the corrected links against the closed frames {re}")
    for q, bar in bars(RECOMPOSED_MEASURED).items():
        assert re[q] <= bar, (q, re[q], bar)
    assert np.array_equal(u8(fused_open["frames"]), u8(FS.run_host(FS.host_lib(), S, dict(state, links=state["links"][:k - 1]))["frames"]))
    # the features seen across the seam: the two copies, against the twins (close_ring's, then fuse's, on the read-back state)
    closing = state["links"][k - 1]
    twin_links = [dict(L, sim=twin["links"][i].astype(np.float32)) for i, L in enumerate(state["links"][:k - 1])]
    twin_fused = FR.fuse(dict(state, links=twin_links))
    g_dev, g_twin, g_open = seam_gap(fused, state["pairs"], closing, k), seam_gap(twin_fused, state["pairs"], closing, k), seam_gap(fused_open, state["pairs"], closing, k)
    print(f"  {len(g_dev)} features across the seam: gap / depth median corrected {np.median(g_dev):.4g} (twin {np.median(g_twin):.4g}), measured links {np.median(g_open):.4g}")
    assert len(g_dev) >= 10 and len(g_twin) >= 10
    assert np.median(g_dev) <= 1.25 * np.median(g_twin) + 1e-7
    for p in made:
        p.close()
