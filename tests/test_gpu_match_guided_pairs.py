"""GPU: sfm_match_guided_pairs against the host build (tests/hostcheck/libmatchguidedcheck.so) and the single call
(sfm_match_guided): a ragged list over both configurations in one call, split counts from the shared budget, a job search several
levels deep, degenerate gates among good jobs, repeatability next to the single call, the contract with the records compared
before and after every refusal, the whole chain plain match -> estimateE -> sfm_refine_pairs -> sfm_pair_fundamentals -> one
sfm_match_guided_pairs on the device, and the facade through host/guided_pairs_demo.  Every comparison is over the five match
fields bit for bit, with all other fields and the whole of d_sift2 byte-equal to before."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
import match_guided_scene as MS
from helpers import to_dev as _to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canary_record():
    c = np.zeros(1, S.SIFT_DTYPE)
    c["match"] = 123456; c["score"] = -7.0; c["ambiguity"] = -8.0; c["match_xpos"] = -9.0; c["match_ypos"] = -10.0
    c["xpos"] = 3.0; c["ypos"] = 5.0; c["data"] = 0.25
    return c


def upload(gpu, rec):
    """the records with a canary record behind them -> device tensor (len(rec) + 1 rows of 576 bytes)"""
    torch, dev, _ = gpu
    return _to_dev(torch, dev, np.concatenate([np.array(rec, copy=True), canary_record()]))


def records(t, n):
    return t.cpu().numpy().view(S.SIFT_DTYPE).reshape(-1)[:n]


def dev_F(gpu, F):
    torch, dev, _ = gpu
    return torch.from_numpy(np.ascontiguousarray(np.asarray(F, np.float32).reshape(9))).to(dev)


@functools.lru_cache(maxsize=None)
def host(n1, n2, seed, band=4.0):
    sc = MS.scene(n1, n2, seed)
    return MS.host_run(sc["sift1"], sc["sift2"], sc["F"], band)


class Job:
    """one job's device buffers, from (sift1, sift2, F) on the host"""
    def __init__(self, gpu, s1, s2, F):
        self.s1, self.s2, self.n1, self.n2 = s1, s2, len(s1), len(s2)
        self.d1, self.d2, self.dF = upload(gpu, s1), upload(gpu, s2), dev_F(gpu, F)

    def tuple(self):
        return (self.d1, self.n1, self.d2, self.n2, self.dF)

    def check(self, want):
        """the five fields are `want`'s, everything else is as uploaded, the canaries stand"""
        got = records(self.d1, self.n1 + 1)
        assert MS.fields_equal(got[:self.n1], want)
        for f in self.s1.dtype.names:
            if f not in MS.FIELDS:
                assert np.array_equal(got[f][:self.n1].view(np.uint32), self.s1[f].view(np.uint32)), f
        assert got[self.n1:].tobytes() == canary_record().tobytes()
        db = records(self.d2, self.n2 + 1)
        assert db[:self.n2].tobytes() == np.ascontiguousarray(self.s2).tobytes() and db[self.n2:].tobytes() == canary_record().tobytes()


def scene_job(gpu, n1, n2, seed):
    sc = MS.scene(n1, n2, seed)
    return Job(gpu, sc["sift1"], sc["sift2"], sc["F"])


def single(gpu, job, band=4.0):
    """the single call on copies of the job's records -> sift1 afterwards"""
    torch, dev, ctx = gpu
    d1, d2 = upload(gpu, job.s1), upload(gpu, job.s2)
    S.match_guided(ctx, d1, job.n1, d2, job.n2, job.dF, band_px=band)
    torch.cuda.synchronize()
    return records(d1, job.n1)


# 1 ---- a ragged list in one call ---------------------------------------------------------------------------------------------------
RAGGED = [(1, 1), (31, 33), (33, 31), (255, 64), (257, 65), (1024, 1025), (0, 64), (64, 0), (4600, 97)]     # the last: launch two, (1,8)


def test_ragged_list_in_one_call(gpu):
    torch, dev, ctx = gpu
    jobs = []
    for k, (n1, n2) in enumerate(RAGGED):
        sc = MS.scene(n1, n2, 7 + k)
        s1 = np.array(sc["sift1"], copy=True)
        if n1 == 0 or n2 == 0:                       # the empty jobs' records carry canaries in the match fields
            for f, v in (("match", 4242), ("score", -1.0), ("ambiguity", -2.0), ("match_xpos", -3.0), ("match_ypos", -4.0)):
                s1[f] = v
        jobs.append(Job(gpu, s1, sc["sift2"], sc["F"]))
    ctx.set_match_kernel(S.MATCH_AUTO)
    last = ctx.last_match_kernel()
    S.match_guided_pairs(ctx, [j.tuple() for j in jobs], band_px=4.0)
    torch.cuda.synchronize()
    assert ctx.last_match_kernel() == last
    for k, (j, (n1, n2)) in enumerate(zip(jobs, RAGGED)):
        if n1 == 0 or n2 == 0:
            j.check(j.s1)                            # untouched
            continue
        want = host(n1, n2, 7 + k)
        assert (want["match"] >= 0).sum() >= min(n1, n2) // 2 or min(n1, n2) < 4
        j.check(want)
        assert MS.fields_equal(single(gpu, j), want)


# 2 ---- split counts from the shared budget -------------------------------------------------------------------------------------------
def test_split_counts_from_the_shared_budget(gpu):
    """alone the job takes many splits, among forty small jobs few (tests/test_match_guided_pairs_host.py: 23 against 4 on 256
    CUs): the same bytes"""
    torch, dev, ctx = gpu
    want = host(2155, 2170, 7)
    alone = scene_job(gpu, 2155, 2170, 7)
    S.match_guided_pairs(ctx, [alone.tuple()], band_px=4.0)
    small = [scene_job(gpu, 257, 65, 8) for _ in range(40)]
    among = scene_job(gpu, 2155, 2170, 7)
    S.match_guided_pairs(ctx, [j.tuple() for j in small[:20]] + [among.tuple()] + [j.tuple() for j in small[20:]], band_px=4.0)
    torch.cuda.synchronize()
    alone.check(want)
    among.check(want)
    for j in small:
        j.check(host(257, 65, 8))


# 3 ---- seventy jobs -------------------------------------------------------------------------------------------------------------------
def test_seventy_jobs(gpu):
    """the job search several levels deep, query blocks partly filled"""
    torch, dev, ctx = gpu
    sizes = [(33 + (k * 41) % 98, 40 + (k * 13) % 90) for k in range(70)]
    assert min(s[0] for s in sizes) == 33 and max(s[0] for s in sizes) == 130
    jobs = [scene_job(gpu, n1, n2, 100 + k) for k, (n1, n2) in enumerate(sizes)]
    S.match_guided_pairs(ctx, [j.tuple() for j in jobs], band_px=4.0)
    torch.cuda.synchronize()
    for k, (j, (n1, n2)) in enumerate(zip(jobs, sizes)):
        j.check(host(n1, n2, 100 + k))


# 4 ---- degenerate gates -----------------------------------------------------------------------------------------------------------------
def test_degenerate_gates_among_good_jobs(gpu):
    torch, dev, ctx = gpu
    sc = MS.scene(257, 65, 7)
    s1 = np.array(sc["sift1"], copy=True)
    s1["match"] = 5; s1["score"] = 0.5; s1["ambiguity"] = 0.5; s1["match_xpos"] = 1.0; s1["match_ypos"] = 2.0
    Fnan = np.array(sc["F"], np.float64); Fnan[1, 1] = np.nan
    jobs = [scene_job(gpu, 255, 64, 9), Job(gpu, s1, sc["sift2"], np.zeros((3, 3))), scene_job(gpu, 257, 65, 7),
            Job(gpu, s1, sc["sift2"], Fnan), scene_job(gpu, 31, 33, 11)]
    S.match_guided_pairs(ctx, [j.tuple() for j in jobs], band_px=4.0)
    torch.cuda.synchronize()
    for k in (1, 3):
        got = records(jobs[k].d1, 257)
        assert np.all(got["match"] == -1)
        for f in ("score", "match_xpos", "match_ypos", "ambiguity"):
            assert np.all(got[f].view(np.uint32) == 0), f
        jobs[k].check(MS.host_run(s1, sc["sift2"], np.zeros((3, 3)) if k == 1 else Fnan, 4.0))
    jobs[0].check(host(255, 64, 9))
    jobs[2].check(host(257, 65, 7))
    jobs[4].check(host(31, 33, 11))
    assert (host(257, 65, 7)["match"] >= 0).sum() > 30


# 5 ---- repeatability ----------------------------------------------------------------------------------------------------------------------
def test_repeatability_beside_the_single_call(gpu):
    torch, dev, ctx = gpu
    shapes = [(1024, 1025, 12), (257, 65, 7), (4600, 97, 15)]
    jobs = [scene_job(gpu, *s) for s in shapes]
    S.match_guided_pairs(ctx, [j.tuple() for j in jobs], band_px=4.0)
    first = [j.d1.clone() for j in jobs]
    S.match_guided_pairs(ctx, [j.tuple() for j in jobs], band_px=4.0)
    torch.cuda.synchronize()
    for j, f, s in zip(jobs, first, shapes):
        assert torch.equal(f, j.d1)
        j.check(host(*s))
    # a plain single call, then the batched call on fresh records, then a single call again: each is right
    one = scene_job(gpu, 2155, 2170, 7)
    S.match_guided(ctx, one.d1, one.n1, one.d2, one.n2, one.dF, band_px=4.0)
    again = [scene_job(gpu, *s) for s in shapes]
    S.match_guided_pairs(ctx, [j.tuple() for j in again], band_px=4.0)
    after = scene_job(gpu, 2155, 2170, 7)
    S.match_guided(ctx, after.d1, after.n1, after.d2, after.n2, after.dF, band_px=4.0)
    torch.cuda.synchronize()
    one.check(host(2155, 2170, 7))
    after.check(host(2155, 2170, 7))
    for j, s in zip(again, shapes):
        j.check(host(*s))


# 6 ---- the contract, at sizes <= 255 only ------------------------------------------------------------------------------------------------
def test_contract(gpu):
    torch, dev, ctx = gpu
    L = S.lib()
    sc = [MS.scene(255, 64, 7), MS.scene(200, 100, 8)]
    canary = []
    for s in sc:
        c = np.array(s["sift1"], copy=True)
        c["match"] = 123456; c["score"] = -7.0; c["ambiguity"] = -8.0; c["match_xpos"] = -9.0; c["match_ypos"] = -10.0
        canary.append(c)
    jobs = [Job(gpu, canary[0], sc[0]["sift2"], sc[0]["F"]), Job(gpu, canary[1], sc[1]["sift2"], sc[1]["F"])]
    # a table of two F matrices: job 1's d_sift1 can be laid over "another job's d_F" only by address, so the F of job 0 lives
    # inside a spare record array here
    spare = upload(gpu, canary[0])
    before = [t.clone() for j in jobs for t in (j.d1, j.d2)] + [spare.clone()]

    def unchanged():
        torch.cuda.synchronize()
        now = [t for j in jobs for t in (j.d1, j.d2)] + [spare]
        return all(torch.equal(a, b) for a, b in zip(before, now))

    ok = S.match_guided_params()
    P = lambda t: t.data_ptr() if t is not None else None
    J = lambda *tuples: S.match_guided_jobs(list(tuples))
    a, b = jobs
    good = [a.tuple(), b.tuple()]
    call = lambda ctx_h, arr, n, p: L.sfm_match_guided_pairs(ctx_h, arr, n, C.byref(p) if p is not None else None)
    refusals = [
        (None, J(*good), 2, ok), (ctx._h, None, 2, ok), (ctx._h, J(*good), 2, None), (ctx._h, J(*good), -1, ok),
        (ctx._h, J(a.tuple(), (P(b.d1), -1, P(b.d2), 100, P(b.dF))), 2, ok),                     # negative sizes
        (ctx._h, J(a.tuple(), (P(b.d1), 200, P(b.d2), -1, P(b.dF))), 2, ok),
        (ctx._h, J(a.tuple(), (None, 200, P(b.d2), 100, P(b.dF))), 2, ok),                       # null pointers in a job that runs
        (ctx._h, J(a.tuple(), (P(b.d1), 200, None, 100, P(b.dF))), 2, ok),
        (ctx._h, J(a.tuple(), (P(b.d1), 200, P(b.d2), 100, None)), 2, ok),
        # job 0's d_sift1 inside job 1's d_sift2; two jobs with one d_sift1; job 1's d_sift1 over job 0's F
        (ctx._h, J(a.tuple(), (P(b.d1), 200, P(a.d1) + 576 * 10, 100, P(b.dF))), 2, ok),
        (ctx._h, J(a.tuple(), (P(a.d1), 255, P(b.d2), 100, P(b.dF))), 2, ok),
        (ctx._h, J(a.tuple(), (P(a.d1) + 576 * 254, 1, P(b.d2), 100, P(b.dF))), 2, ok),          # ... by one record
        (ctx._h, J((P(a.d1), 255, P(a.d2), 64, P(spare) + 576 * 3 + 32), (P(spare), 200, P(b.d2), 100, P(b.dF))), 2, ok),
    ]
    for band in (0.0, -1.0, float("nan"), float("inf")):
        refusals.append((ctx._h, J(*good), 2, S.match_guided_params(band_px=band)))
    for k in range(4):
        r = [0, 0, 0, 0]; r[k] = 1
        refusals.append((ctx._h, J(*good), 2, S.match_guided_params(reserved=r)))
    for i, args in enumerate(refusals):
        assert call(*args) == S.E_INVALID, i
        assert unchanged(), i
    with pytest.raises(S.SfmError) as e:
        S.match_guided_pairs(ctx, good, band_px=-2.0)
    assert e.value.code == S.E_INVALID
    # no job, and jobs that are empty (null pointers allowed there), write nothing
    assert call(ctx._h, J(*good), 0, ok) == S.OK
    assert call(ctx._h, J((P(a.d1), 0, P(a.d2), 64, P(a.dF)), (None, 0, None, 0, None), (P(b.d1), 200, None, 0, None)), 3, ok) == S.OK
    assert unchanged()
    # what may be shared: one second view and one F for two jobs
    c = Job(gpu, canary[0], sc[0]["sift2"], sc[0]["F"])
    assert call(ctx._h, J(a.tuple(), (P(c.d1), 255, P(a.d2), 64, P(a.dF))), 2, ok) == S.OK
    torch.cuda.synchronize()
    want = MS.host_run(canary[0], sc[0]["sift2"], sc[0]["F"], 4.0)
    a.check(want)
    assert MS.fields_equal(records(c.d1, 255), want)
    assert torch.equal(before[2], b.d1)                                                          # job b never ran


# 7 ---- the chain on the device -----------------------------------------------------------------------------------------------------------
def test_chain_of_four_pairs(gpu):
    torch, dev, ctx = gpu
    n = 256
    scs = [MS.scene(n, n, 300 + k) for k in range(4)]
    jobs, pairs, plain = [], [], []
    for sc in scs:
        j = Job(gpu, sc["sift1"], sc["sift2"], sc["F"])
        ctx.match(j.d1, n, j.d2, n)
        torch.cuda.synchronize()
        plain.append(np.array(records(j.d1, n), copy=True))
        pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
        pair.fillXU(j.d1)
        pair.estimateE(S.default_params(n, num_hypotheses=2048))
        jobs.append(j); pairs.append(pair)
    S.refine_pairs(pairs, max_iterations=20)
    table = S.pair_fundamentals(pairs, refined=True)
    S.match_guided_pairs(ctx, [(j.d1, n, j.d2, n, table[k]) for k, j in enumerate(jobs)], band_px=4.0)
    torch.cuda.synchronize()
    F = table.cpu().numpy()
    for k, (j, sc) in enumerate(zip(jobs, scs)):
        got = records(j.d1, n)
        want = MS.host_run(plain[k], sc["sift2"], F[k], 4.0)
        assert MS.fields_equal(got, want), k
        pc, pw = MS.accepted(plain[k], sc["truth"])
        gc, gw = MS.accepted(got, sc["truth"])
        print(f"pair {k}: plain accepted {pc} correct / {pw} wrong, guided at 4 px {gc} correct / {gw} wrong")
    assert len({F[k].tobytes() for k in range(4)}) == 4
    for p in pairs:
        p.close()


# 8 ---- the facade --------------------------------------------------------------------------------------------------------------------------
def test_guided_pairs_demo_prints_guided_match_demos_lines(gpu, tmp_path):
    from view_points_scene import dino_extract
    host_dir = os.path.join(ROOT, "cuda-sfm_amd", "host")
    demo, one = os.path.join(host_dir, "guided_pairs_demo"), os.path.join(host_dir, "guided_match_demo")
    assert os.path.exists(demo) and os.path.exists(one), "guided_pairs_demo / guided_match_demo not built (make)"
    files = []
    for k in (0, 1, 2):
        d, n = dino_extract(gpu, k)
        files.append(str(tmp_path / f"f{k}.bin"))
        d[:n].cpu().numpy().tofile(files[-1])
    lines = lambda out, what: re.findall(r"^%s: .*$" % what, out, flags=re.M)
    want_plain, want_guided = [], []
    for a, b in ((0, 1), (1, 2)):
        r = subprocess.run([one, files[a], files[b]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        want_plain += lines(r.stdout, "plain"); want_guided += lines(r.stdout, "guided")
    r = subprocess.run([demo, "2", files[0], files[1], files[1], files[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(f"guided_pairs_demo: {lines(r.stdout, 'plain')} {lines(r.stdout, 'guided')}; guided_match_demo pair by pair: {want_plain} {want_guided}")
    assert len(want_guided) == 2 and lines(r.stdout, "guided") == want_guided and lines(r.stdout, "plain") == want_plain
    r = subprocess.run([demo, "2", files[0]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
