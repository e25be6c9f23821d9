"""GPU: sfm_fuse_chain (csrc/fuse.hip) through the C ABI -- every output against the host build of the same arithmetic
(tests/hostcheck/libfusecheck.so) on the override path (pairs that only have fillXU); cuts, conflicts, one pair, a ragged chain
and a chain whose block counts need more than one round of the scan; determinism, nothing in any pair changed, every refusal with
nothing written; the full chain on the device against the fp64 twin (tests/fuse_reference.py); the dino frames 0 .. 3."""
import functools

import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import DINO_K, DINO_KINV, to_dev
import fuse_reference as FR
import fuse_scene as FS
import view_points_scene as VS
from test_gpu_align import chain as refined_chain, read_buffers

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
PAIRS = [1, 2, 3, 5]
RECORDS = [1, 63, 64, 65, 257, 1025]                     # per pair: one node block is 256 records
# Kernels against the host build at 5 iterations: the same header functions per lane and per track, no sum whose order differs.
# MEASURED: the largest absolute difference over the 24 cases below, the ragged chain and the tiled chain on the MI355X, in the
# frames, the cameras, the points and the errors.  Every one is 0, so the bars, 4 x the measured maximum, are equality.
MEASURED = dict(frames=0.0, cams=0.0, points=0.0, err=0.0)
BARS = {k: 4.0 * v for k, v in MEASURED.items()}
INTEGERS = ("root", "track", "track_offset", "obs_cam", "obs_record", "flags")


@pytest.fixture(scope="module")
def HL():
    return FS.host_lib()


@functools.lru_cache(maxsize=None)
def scene(n, seed=17):
    return FS.build(n, seed)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


class DeviceChain:
    """A chain on the device on the override path: every pair only has fillXU; points, valid, pose and the links' arrays are
    uploaded.  `host` is the same chain over the device's OWN normalised observations, for the host build and the twin."""

    def __init__(self, gpu, chain):
        torch, dev, ctx = gpu
        d = lambda a: to_dev(torch, dev, np.ascontiguousarray(a))
        self.ctx, self.pairs, self.over, host_pairs = ctx, [], [], []
        for P in chain["pairs"]:
            pair = S.ImagePair(ctx, chain["K"], chain["Kinv"], 2, P["n"])
            pair.fillXU(to_dev(torch, dev, P["sift"]))
            self.pairs.append(pair)
            self.over.append((d(P["points"]), d(P["valid"]), d(P["pose"])))
            host_pairs.append(dict(P, X0=pair.get_XU(S.BUF_X0), X1=pair.get_XU(S.BUF_X1), ld=P["n"]))
        self.indices, self.links = [], []
        for L in chain["links"]:
            rep = S.AlignReport(); rep.status = int(L["status"])
            self.indices.append(d(L["index"]))
            self.links.append((d(L["sim"]), d(L["inlier"]), d(L["err"]), None, d(np.frombuffer(bytes(rep), np.uint8).copy())))
        self.host = dict(chain, pairs=host_pairs)

    def run(self, **kw):
        return S.fuse_chain(self.pairs, self.indices, self.links, overrides=self.over, **kw)

    def close(self):
        for p in self.pairs:
            p.close()


def differences(got, want):
    f = lambda a: np.asarray(a, np.float64)
    d = {k: float(np.abs(f(got[k]) - f(want[k])).max()) if got[k].size else 0.0 for k in ("frames", "cams", "points")}
    fin = np.isfinite(want["err"]) & np.isfinite(got["err"])
    d["err"] = float(np.abs(f(got["err"])[fin] - f(want["err"])[fin]).max()) if fin.any() else 0.0
    return d


def check_against_host(HL, dc, what, iterations=(0, 5)):
    """Integers byte for byte; at 0 iterations everything byte for byte; at 5 the differences within BARS.  Returns the last result."""
    worst = dict.fromkeys(MEASURED, 0.0)
    for iters in iterations:
        got = dc.run(max_iterations=iters)
        want = FS.run_host(HL, S, dc.host, max_iterations=iters)
        assert got["counts"] == want["counts"], (what, iters, got["counts"], want["counts"])
        for k in INTEGERS:
            assert np.array_equal(got[k], want[k]), (what, iters, k)
        assert np.array_equal(np.isinf(got["err"]), np.isinf(want["err"])), (what, iters)
        if iters == 0:
            for k in ("frames", "cams", "points", "err"):
                assert np.array_equal(u8(got[k]), u8(want[k])), (what, k)
        else:
            d = differences(got, want)
            worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"fuse {what}: {got['counts']}, differences at {iterations[-1]} iterations {worst}")
    for k, bar in BARS.items():
        assert worst[k] <= bar, (what, k, worst[k], bar)
    if max(worst.values()) == 0.0:                                             # the same bytes, then
        for k in ("frames", "cams", "points", "err"):
            assert np.array_equal(u8(got[k]), u8(want[k])), (what, k)
    return got


@pytest.mark.parametrize("n", RECORDS)
@pytest.mark.parametrize("k", PAIRS)
def test_override_path_against_the_host_build(gpu, HL, k, n):
    sc, ch = scene(n)
    dc = DeviceChain(gpu, FS.head(ch, k))
    got = check_against_host(HL, dc, f"k={k} n={n}")
    live = sum(int(FR.live_nodes(P).sum()) for P in dc.host["pairs"])
    assert got["counts"]["observations"] == live + got["counts"]["tracks"] and got["counts"]["segments"] == 1
    if k == 1:
        assert got["counts"]["tracks"] == live and got["counts"]["longest_track"] == (2 if live else 0)
    if k == 5 and n >= 63:
        assert got["counts"]["longest_track"] == 6
    dc.close()


def test_ragged_chain_and_more_blocks_than_one_scan_round(gpu, HL):
    sc, ch = scene(257, 7)
    dc = DeviceChain(gpu, FS.truncated(ch, [65, 257, 64, 257, 1]))
    check_against_host(HL, dc, "ragged 65/257/64/257/1")
    dc.close()
    # 11 copies of the 1025-record chain: 55 pairs of 5 node blocks each, 275 block counts against 256 per round of the scan
    sc, ch = scene(1025)
    dc = DeviceChain(gpu, FS.tiled(ch, 11))
    got = check_against_host(HL, dc, "tiled 11 x 5 x 1025", iterations=(5,))
    assert got["counts"]["segments"] == 11 and got["root"].tolist() == [5 * (i // 5) for i in range(55)]
    one = FS.run_host(HL, S, dict(dc.host, pairs=dc.host["pairs"][:5], links=dc.host["links"][:4]))
    assert got["counts"]["tracks"] == 11 * one["counts"]["tracks"] and got["counts"]["observations"] == 11 * one["counts"]["observations"]
    dc.close()
    # 60 copies of the 65-record chain: 300 pairs against 256 links per round of the frames kernel, a segment across the seam
    sc, ch = scene(65)
    dc = DeviceChain(gpu, FS.tiled(ch, 60))
    got = check_against_host(HL, dc, "tiled 60 x 5 x 65", iterations=(5,))
    assert got["counts"]["segments"] == 60 and got["root"].tolist() == [5 * (i // 5) for i in range(300)]
    assert np.array_equal(u8(got["frames"][255:260]), u8(got["frames"][0:5])) and got["counts"]["longest_track"] == 6
    dc.close()


def test_cut_conflict_and_one_pair_on_the_device(gpu, HL):
    sc, ch = scene(257, 7)
    nan_t = ch["links"][2]["sim"].copy(); nan_t[11] = np.nan
    zero_s = ch["links"][2]["sim"].copy(); zero_s[0] = 0.0
    for name, change in (("degenerate", dict(status=S.REFINE_DEGENERATE)), ("s = 0", dict(sim=zero_s)), ("NaN in t", dict(sim=nan_t))):
        dc = DeviceChain(gpu, dict(ch, links=[dict(L, **change) if i == 2 else L for i, L in enumerate(ch["links"])]))
        got = check_against_host(HL, dc, f"cut ({name})")
        assert got["root"].tolist() == [0, 0, 0, 3, 3] and got["counts"]["segments"] == 2 and got["counts"]["longest_track"] == 4
        assert np.array_equal(got["frames"][3], FS.sim13(1.0, np.eye(3), np.zeros(3)))
        for t in range(got["counts"]["tracks"]):
            pairs = got["obs_cam"][got["track_offset"][t]:got["track_offset"][t + 1]] >> 1
            assert pairs.max() <= 2 or pairs.min() >= 3, (name, t)
        dc.close()
    # three records of pair 0 name one record of pair 1: the smallest error wins, then the lowest record
    base = FS.head(ch, 2)
    L = base["links"][0]
    prop = np.flatnonzero(L["inlier"] != 0)
    first, m = int(prop[5]), int(L["index"][prop[5]])
    others = [int(j) for j in np.flatnonzero(FR.live_nodes(base["pairs"][0]) & (L["inlier"] == 0))[:2]]
    recs = sorted([first] + others)
    for name, errs, winner in (("the middle one best", [0.5, 0.125, 0.25], recs[1]), ("all alike", [0.25, 0.25, 0.25], recs[0])):
        link = dict(L, index=L["index"].copy(), inlier=L["inlier"].copy(), err=L["err"].copy())
        for j, e in zip(recs, errs):
            link["index"][j] = m; link["inlier"][j] = 1; link["err"][j] = e
        dc = DeviceChain(gpu, dict(base, links=[link]))
        got = check_against_host(HL, dc, f"conflict ({name})")
        t = got["track"][257 + m]
        assert t >= 0 and got["track"][winner] == t
        for j in recs:
            if j != winner:
                tj = got["track"][j]
                assert tj >= 0 and tj != t and got["track_offset"][tj + 1] - got["track_offset"][tj] == 2, (name, j)
        dc.close()
    dc = DeviceChain(gpu, FS.head(ch, 1))
    got = check_against_host(HL, dc, "one pair")
    live = FR.live_nodes(dc.host["pairs"][0])
    assert got["counts"]["tracks"] == live.sum() and np.array_equal(got["obs_cam"], np.tile([0, 1], live.sum()))
    dc.close()


def filled(torch, dev, k, N):
    f = lambda n, dt, v: torch.full((int(n),), v, dtype=dt, device=dev)
    i32, f32 = torch.int32, torch.float32
    return (f(13 * k, f32, -3.0), f(k, i32, -9), f(24 * k, f32, -3.0), f(N, i32, -9), f(N + 1, i32, -9), f(2 * N, i32, -9), f(2 * N, i32, -9),
            f(4 * N, f32, -3.0), f(N, torch.uint8, PATTERN), f(N, f32, -3.0), f(8, i32, -9))


def untouched(outs):
    return all(bool((t == v).all()) for t, v in zip(outs, (-3.0, -9, -3.0, -9, -9, -9, -9, -3.0, PATTERN, -3.0, -9)))


def test_second_call_repeats_nothing_changes_and_refusals_write_nothing(gpu, HL):
    torch, dev, ctx = gpu
    sc, ch = scene(257, 7)
    dc = DeviceChain(gpu, ch)
    before = [read_buffers(p, ctx) for p in dc.pairs]
    first, second = dc.run(), dc.run()
    assert first["counts"] == second["counts"] and first["counts"]["tracks"] == 391
    for key in first:
        if key != "counts":
            assert np.array_equal(u8(first[key]), u8(second[key])), key
    for p, bufs in zip(dc.pairs, before):                                      # every SFM_BUF_* of every pair
        for which, (a, b) in enumerate(zip(bufs, read_buffers(p, ctx))):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), which
    k, N = 5, 5 * 257
    outs = filled(torch, dev, k, N)
    params = S.fuse_params()
    links = [(dc.indices[i], a[0], a[1], a[2], a[4]) for i, a in enumerate(dc.links)]
    pin = [(p,) + o for p, o in zip(dc.pairs, dc.over)]

    def refused(code, pairs=pin, lk=links, p=params, o=outs, context=ctx):
        with pytest.raises(S.SfmError) as e:
            S.fuse_chain_enqueue(context, pairs, lk, p, o)
        ctx.synchronize()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    assert "pairs[3]: the pair is listed twice" in refused(S.E_INVALID, pairs=pin[:3] + [pin[1]] + pin[4:])
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = S.ImagePair(other, ch["K"], ch["Kinv"], 2, 257)
    foreign.fillXU(to_dev(torch, dev, ch["pairs"][2]["sift"]))
    assert "pairs[2]: the pair belongs to another context" in refused(S.E_INVALID, pairs=pin[:2] + [(foreign,) + dc.over[2]] + pin[3:])
    assert "another context" in refused(S.E_INVALID, context=other)
    # aliasing: an output on an input of a pair, of a link, on another output
    assert "out.d_track overlaps links[1].d_index" in refused(S.E_INVALID, o=outs[:3] + (dc.indices[1],) + outs[4:])
    assert "out.d_flags overlaps pairs[4].d_valid" in refused(S.E_INVALID, o=outs[:8] + (dc.over[4][1].data_ptr() + 256,) + outs[9:])
    assert "out.d_cams overlaps links[0].d_sim" in refused(S.E_INVALID, o=outs[:2] + (dc.links[0][0].data_ptr() + 48,) + outs[3:])
    big = torch.full((8 * N,), -9, dtype=torch.int32, device=dev)
    assert "out.d_obs_record overlaps out.d_obs_cam" in refused(S.E_INVALID, o=outs[:5] + (big, big.data_ptr() + 8 * N - 4) + outs[7:])
    assert "out.d_counts overlaps out.d_err" in refused(S.E_INVALID, o=outs[:9] + (big, big.data_ptr() + 4 * N - 4))
    assert "reserved" in refused(S.E_INVALID, p=S.fuse_params(reserved=[0, 0, 0, 1]))
    refused(S.E_INVALID, p=S.fuse_params(max_iterations=51))
    # a missing refinement without both overrides
    assert "pairs[1]" in refused(S.E_STATE, pairs=pin[:1] + [dc.pairs[1]] + pin[2:])
    assert "pairs[4]" in refused(S.E_STATE, pairs=pin[:4] + [(dc.pairs[4], dc.over[4][0], dc.over[4][1], None)])
    assert "pairs[0]" in refused(S.E_STATE, pairs=[(dc.pairs[0], None, None, dc.over[0][2])] + pin[1:])
    bare = S.ImagePair(ctx, ch["K"], ch["Kinv"], 2, 257)                       # no points at all
    assert "pairs[2]" in refused(S.E_STATE, pairs=pin[:2] + [(bare,) + dc.over[2]] + pin[3:])
    assert untouched(outs) and bool((big == -9).all())
    S.fuse_chain_enqueue(ctx, pin, links, params, outs)                        # ... and the same buffers serve the valid call
    ctx.synchronize()
    assert not untouched(outs) and int(outs[10][0]) == 391
    for p in (bare, foreign):
        p.close()
    other.close()
    dc.close()


def read_back_chain(torch, made, idx, aouts, K, Kinv):
    """The device state a fuse_chain call without overrides reads, as the chain dict of the host build and the twin."""
    pairs = []
    for p in made:
        _, used = p.get_reprojection_errors()
        P4 = p.get_refined_pose()[0]
        pairs.append(dict(n=p.num_points, ld=p.num_points, points=p.get_refined_points(), valid=used, X0=p.get_XU(S.BUF_X0), X1=p.get_XU(S.BUF_X1),
                          pose=np.concatenate([P4[:3, :3].ravel(), P4[:3, 3]]).astype(np.float32)))
    links = []
    for d_index, a in zip(idx, aouts):
        rep = S.AlignReport.from_buffer_copy(a[4].cpu().numpy().tobytes())
        links.append(dict(index=d_index.cpu().numpy(), sim=a[0].cpu().numpy()[:13].copy(), inlier=a[1].cpu().numpy(), err=a[2].cpu().numpy(),
                          status=rep.status))
    return dict(K=K, Kinv=Kinv, pairs=pairs, links=links)


def aligned(gpu, made, idx):
    """sfm_align_pairs over the chain with its outputs left on the device."""
    torch, dev, ctx = gpu
    params = S.align_params()
    aouts = [S._align_buffers(torch, dev, p.num_points, params.num_hypotheses) for p in made[:-1]]
    S.align_pairs_enqueue(made[:-1], made[1:], idx, params, aouts)
    return aouts


def test_full_chain_on_the_device(gpu, HL):
    """5 views, n = 1024: fillXU -> estimateE -> refine_pairs -> align_pairs -> fuse_chain, no overrides.  The structure equals the
    twin's on the read-back state; the points are held to 1.25 x the twin's error against the truth, not to the truth (6g's rule:
    what is off is the two-view reconstructions the chain connects)."""
    torch, dev, ctx = gpu
    sc, _ = FS.build(1024, 61, views=5)
    made, reports = refined_chain(gpu, sc)
    idx = [to_dev(torch, dev, L["index"]) for L in sc["links"]]
    aouts = aligned(gpu, made, idx)
    got = S.fuse_chain(made, idx, aouts)
    state = read_back_chain(torch, made, idx, aouts, sc["K"], sc["Kinv"])
    host, twin = FS.run_host(HL, S, state), FR.fuse(state)
    print(f"full chain: {got['counts']}; links " + ", ".join(f"status {L['status']} s {L['sim'][0]:.4f} {int(L['inlier'].sum())} inliers" for L in state["links"]))
    assert got["counts"] == host["counts"]
    for k in INTEGERS:
        assert np.array_equal(got[k], host[k]), k
    d = differences(got, host)
    for k, bar in BARS.items():
        assert d[k] <= bar, (k, d[k], bar)
    for k in ("track", "track_offset", "obs_cam", "obs_record", "root"):
        assert np.array_equal(got[k], twin[k]), k
    for k in ("tracks", "observations", "segments", "longest_track"):
        assert got["counts"][k] == twin["counts"][k], k
    assert got["counts"]["tracks"] > 0 and got["counts"]["longest_track"] >= 3
    band = np.abs(twin["err"] - 4.0) <= 0.4
    assert np.array_equal(got["flags"][~band], twin["flags"][~band])
    # against the truth in pair 0's frame, on the refined tracks of the first segment whose records are one true feature
    truth = FS.truth_in_pair0(sc, state, got)
    pure = np.zeros(len(got["flags"]), bool)
    for t in range(len(pure)):
        o = np.arange(got["track_offset"][t], got["track_offset"][t + 1] - 1)
        ids = [sc["perm"][got["obs_cam"][q] >> 1][got["obs_record"][q]] for q in o]
        pure[t] = len(set(ids)) == 1 and all(sc["pairs"][got["obs_cam"][q] >> 1]["good"][got["obs_record"][q]] for q in o)
    pure &= np.isfinite(truth).all(1) & (got["flags"] == S.FUSE_REFINED) & (twin["flags"] == FR.REFINED)
    e_dev = np.linalg.norm(got["points"][:3].T[pure].astype(np.float64) - truth[pure], axis=1) / truth[pure, 2]
    e_twin = np.linalg.norm(twin["points"][:3].T[pure] - truth[pure], axis=1) / truth[pure, 2]
    print(f"  {pure.sum()} clean refined tracks of segment 0: |X - truth| / depth median device {np.median(e_dev):.4g} twin {np.median(e_twin):.4g}, "
          f"largest device {e_dev.max():.4g} twin {e_twin.max():.4g}")
    assert pure.sum() >= 50
    assert np.median(e_dev) <= 1.25 * np.median(e_twin) + 1e-7 and e_dev.max() <= 1.25 * e_twin.max() + 1e-7
    for p in made:
        p.close()


def test_dino_frames_0_to_3(gpu, HL):
    """Real frames: pairs (0, 1), (1, 2), (2, 3).  No bar on scale: the counts are printed and compared with the twin's on the
    read-back state."""
    torch, dev, ctx = gpu
    views = [VS.dino_extract(gpu, k) for k in range(4)]
    made, idx = [], []
    for (da, na), (db, nb) in zip(views[:-1], views[1:]):
        ctx.match(da, na, db, nb)
        pair = S.ImagePair(ctx, DINO_K, DINO_KINV, 2, na)
        pair.fillXU(da)
        pair.estimateE(S.default_params(na))
        made.append(pair)
    S.refine_pairs(made, max_iterations=20)
    for (da, na), _ in zip(views[:-2], made[:-1]):
        d_index = torch.empty(na, dtype=torch.int32, device=dev)
        S.align_index_from_matches(ctx, da, na, d_index)
        idx.append(d_index)
    aouts = aligned(gpu, made, idx)
    got = S.fuse_chain(made, idx, aouts)
    state = read_back_chain(torch, made, idx, aouts, DINO_K, DINO_KINV)
    host, twin = FS.run_host(HL, S, state), FR.fuse(state)
    print(f"dino 0..3: device {got['counts']}\n  twin {twin['counts']}; links " +
          ", ".join(f"status {L['status']} s {L['sim'][0]:.4f} {int(L['inlier'].sum())} inliers" for L in state["links"]))
    assert got["counts"] == host["counts"]
    for k in INTEGERS:
        assert np.array_equal(got[k], host[k]), k
    d = differences(got, host)
    for k, bar in BARS.items():
        assert d[k] <= bar, (k, d[k], bar)
    for k in ("track", "track_offset", "obs_cam", "obs_record", "root"):
        assert np.array_equal(got[k], twin[k]), k
    for k in ("tracks", "observations", "segments", "longest_track"):
        assert got["counts"][k] == twin["counts"][k], k
    band = np.abs(twin["err"] - 4.0) <= 0.4
    assert np.array_equal(got["flags"][~band], twin["flags"][~band])
    assert got["counts"]["tracks"] > 0 and np.isfinite(got["points"]).all()
    for p in made:
        p.close()
