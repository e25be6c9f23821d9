"""CPU: sfm_align_pair / sfm_align_pairs without a device -- the header's Jacobians against central differences, the triad solver
against Umeyama's SVD solution on exact triples, the host build (tests/hostcheck/libaligncheck.so: the header's functions,
serial fp64 sums) against ground truth and against the fp64 twin (tests/align_reference.py) on the checked scenes, degenerate
inputs, chain_links, struct layouts, header / exports / Python mirror, the argument checks that precede the device, and the
compiler's resource report of align.hip."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import align_reference as AR
import align_scene as AS
import refine_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "build", "align.usage.txt")
NAMES = ["sfm_align_default_params", "sfm_align_index_from_matches", "sfm_align_pair", "sfm_align_pairs"]
f32p = C.POINTER(C.c_float)
# Triad solver (fp32) against Umeyama by SVD (fp64) on 4096 exact, well-conditioned triples (points in [-1, 1]^2 x [4, 8], sin of
# the angle at the first sample >= 0.2, s in [0.5, 2]): MEASURED largest relative difference in s, rotation angle (rad), largest
# |dt| / max(1, |t|).  The bars are 4 x these.
SOLVER_MEASURED = dict(s=1.8e-7, rot=3.0e-6, t=2.0e-5)
SOLVER_BARS = {k: 4.0 * v for k, v in SOLVER_MEASURED.items()}
# host build against the twin from the same inlier set and the same start, DESIGN 6b's bars for rotation and t; for s the MEASURED
# largest relative difference over the three scenes, bar 4 x that.
ROT_BAR, T_BAR = 2e-5, 2e-5
S_MEASURED = 1.6e-6
S_BAR = 4.0 * S_MEASURED
# exact points: 6c's bars
EXACT_BAR = 1e-4


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def HL():
    h = AS.host_lib()
    h.aln_solve3.argtypes = [f32p, f32p, f32p]
    h.aln_jacobian.argtypes = [f32p, f32p, f32p, f32p, C.c_float, f32p]
    h.aln_jacobian.restype = None
    h.aln_layout.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    return h


@pytest.fixture(scope="module")
def runs(S, HL):
    """Per checked scene: the scene, the host build's result on its first link, and the twin's, computed once."""
    out = []
    for n, seed in AS.SCENES:
        sc = AS.build(n, seed)
        A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
        out.append((sc, AS.run_host(HL, S, A, B, L["index"], K=sc["K"]), AR.run(A, B, L["index"], sc["K"], sc["K"])))
    return out


def fp(a):
    return a.ctypes.data_as(f32p)


def lib_jac(HL, cam, sim, cand, thr=4.0):
    out = np.zeros(34, np.float32)
    HL.aln_jacobian(fp(cam), fp(cam), fp(np.ascontiguousarray(sim, np.float32)), fp(np.ascontiguousarray(cand, np.float32)), thr, fp(out))
    return out[:4].astype(np.float64), out[4:32].reshape(4, 7).astype(np.float64), bool(out[32]), float(out[33])


def test_jacobians_match_central_differences(HL):
    """Steps and bar of tests/test_refine_host.py's camera block (6b): 1e-4, 1e-3 of the block's largest entry; the step in sigma
    is 1e-3 (a relative change of the scale, whose residuals are as smooth as the translation's)."""
    sc = AS.build(64, 3, wrong_match=0.0, wrong_index=0.0)
    A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
    K = sc["K"].astype(np.float64)
    cam = np.array([K[0, 0], K[0, 1], K[1, 1]], np.float32)
    j, Xa, Xb, oa, ob = AR.gather(A, B, L["index"])
    R = RR.expso3(np.array([1e-3, -2e-3, 5e-4])) @ L["R"]
    t = L["t"] + np.array([0.01, -0.02, 0.005])
    s = L["s"] * 1.01
    pack = lambda s_, R_, t_: np.concatenate([[s_], R_.ravel(), t_]).astype(np.float32)
    for k in range(0, len(j), 7):
        cand = np.concatenate([Xa[k], Xb[k], oa[k], ob[k]])
        r, J, _, _ = lib_jac(HL, cam, pack(s, R, t), cand)
        want = AR.residuals(AR.cams(K), AR.cams(K), (s, R, t), Xa[k:k + 1], Xb[k:k + 1], oa[k:k + 1], ob[k:k + 1])[0][0]
        assert np.abs(r - want).max() <= 1e-3 * max(1.0, np.abs(want).max()), (k, r, want)
        assert not J[2:, 6].any()                                              # the backward residual does not see the scale
        for c in range(7):
            h = 1e-3 if c == 6 else 1e-4

            def at(sgn):
                d = np.zeros(7); d[c] = sgn * h
                return lib_jac(HL, cam, pack(s * np.exp(d[6]), RR.expso3(d[:3]) @ R, t + d[3:6]), cand)[0]
            fd = (at(1) - at(-1)) / (2 * h)
            for rows in (slice(0, 2), slice(2, 4)):
                assert np.abs(fd[rows] - J[rows, c]).max() <= 1e-3 * max(np.abs(J[rows]).max(), 1e-30), (k, c, fd, J[:, c])


def exact_triples(count, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        a = np.stack([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(4, 8, 3)], 1)
        u, v = a[1] - a[0], a[2] - a[0]
        if np.linalg.norm(np.cross(u, v)) < 0.2 * np.linalg.norm(u) * np.linalg.norm(v):
            continue
        w = rng.standard_normal(3)
        R = RR.expso3(w / np.linalg.norm(w) * rng.uniform(0, 0.5))
        s, t = rng.uniform(0.5, 2.0), rng.uniform(-1, 1, 3)
        out.append((a, s * a @ R.T + t))
    return out


def test_triad_solver_equals_umeyama_on_exact_triples(HL):
    worst = dict(s=0.0, rot=0.0, t=0.0)
    for a, b in exact_triples(4096):
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        sim = np.zeros(13, np.float32)
        assert HL.aln_solve3(fp(np.ascontiguousarray(a32)), fp(np.ascontiguousarray(b32)), fp(sim)) == 1
        s, R, t = AR.umeyama(a32.astype(np.float64), b32.astype(np.float64))
        worst["s"] = max(worst["s"], abs(sim[0] - s) / s)
        worst["rot"] = max(worst["rot"], RR.rotation_angle(sim[1:10].reshape(3, 3).astype(np.float64), R))
        worst["t"] = max(worst["t"], np.abs(sim[10:] - t).max() / max(1.0, np.linalg.norm(t)))
    print(f"triad solver against Umeyama: {worst}")
    for k, bar in SOLVER_BARS.items():
        assert worst[k] <= bar, (k, worst[k], bar)


def test_degenerate_samples_store_the_zero_link(HL):
    sim = np.ones(13, np.float32)
    a = np.array([[0, 0, 5], [1, 0, 5], [2, 0, 5]], np.float32)                 # collinear in A
    b = np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5]], np.float32)
    assert HL.aln_solve3(fp(a), fp(b), fp(sim)) == 0 and not sim.any()
    sim[:] = 1
    assert HL.aln_solve3(fp(b), fp(a), fp(sim)) == 0 and not sim.any()          # collinear in B
    sim[:] = 1
    c = b.copy(); c[1] = c[0]                                                   # coincident samples
    assert HL.aln_solve3(fp(c), fp(b), fp(sim)) == 0 and not sim.any()
    sim[:] = 1
    d = b.copy(); d[2, 1] = np.nan
    assert HL.aln_solve3(fp(b), fp(d), fp(sim)) == 0 and not sim.any()
    # no candidate passes the zero link
    cam = np.array([2360.0, 0.0, 2360.0], np.float32)
    _, _, inl, err = lib_jac(HL, cam, np.zeros(13, np.float32), np.array([0, 0, 5, 0, 0, 5, 0, 0, 0, 0], np.float32))
    assert not inl and err == np.inf


def test_exact_points_recover_the_link(S, HL):
    """n = 512, no noise, no wrong matches or indices: 6c's exact-point bars."""
    sc = AS.build(512, 11, noise_px=0.0, wrong_match=0.0, wrong_index=0.0)
    A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
    sim, inl, err, counts, rep, order = AS.run_host(HL, S, A, B, L["index"], K=sc["K"])
    es, er, et = AS.sim_errors(sim[:13], L)
    print(f"exact points: {rep}, errors s {es:.3g} rot {er:.3g} t {et:.3g}")
    assert rep["status"] != S.REFINE_DEGENERATE and rep["num_candidates"] == 512 and rep["num_inliers"] == 512
    assert es <= EXACT_BAR and er < EXACT_BAR and et <= EXACT_BAR
    assert np.array_equal(order[:512], np.arange(512)) and inl.all() and err.max() < 0.1


@pytest.mark.parametrize("which", range(len(AS.SCENES)))
def test_noisy_scenes_against_truth_and_twin(S, HL, runs, which):
    """15 % wrong view-2 matches on each side, 5 % wrong indices.  Bars of 6c for the mask, of 6b for the refined link."""
    sc, host, twin = runs[which]
    A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
    sim, inl, err, counts, rep, order = host
    cand = AS.candidates(A, B, L["index"])
    m = int(cand.sum())
    assert rep["num_candidates"] == m and np.array_equal(order[:m], np.flatnonzero(cand)) and (order[m:] == -1).all()
    assert np.array_equal(twin["records"], np.flatnonzero(cand))
    good, bad = cand & L["good"], cand & ~L["good"]
    for name, flags in (("host", inl.astype(bool)), ("twin", twin["inlier"])):
        print(f"{AS.SCENES[which]} {name}: {m} candidates, {good.sum()} good ({flags[good].mean():.4f} kept), {bad.sum()} bad ({flags[bad].mean():.4f} kept)")
        assert flags[good].mean() >= 0.95 and flags[bad].mean() <= 0.01, name
        assert not flags[~cand].any()
    assert np.isposinf(err[~cand]).all() and rep["num_inliers"] == int(inl.sum())
    # the twin from the host's winner and the host's RANSAC inliers: the two LM chains start alike
    h0 = AS.run_host(HL, S, A, B, L["index"], K=sc["K"], max_iterations=0)
    assert np.array_equal(h0[0][:13], h0[0][13:]) and np.array_equal(h0[0][13:], sim[13:]) and h0[4]["num_inliers"] == rep["ransac_inliers"]
    win = (float(sim[13]), sim[14:23].reshape(3, 3).astype(np.float64), sim[23:26].astype(np.float64))
    tw = AR.run(A, B, L["index"], sc["K"], sc["K"], start=win, inliers=h0[1][cand].astype(bool))
    ts, tR, tt = tw["sim"]
    ds = abs(sim[0] - ts) / ts
    dr = RR.rotation_angle(sim[1:10].reshape(3, 3).astype(np.float64), tR)
    dt = np.linalg.norm(sim[10:13] - tt) / np.linalg.norm(tt)
    print(f"  refined against the twin: s {ds:.3g} rot {dr:.3g} t {dt:.3g}; rms {rep['final_rms_px']:.6f} / {tw['lm']['final_rms']:.6f}")
    assert dr <= ROT_BAR and dt <= T_BAR and ds <= S_BAR
    assert abs(rep["final_rms_px"] - tw["lm"]["final_rms"]) <= 1e-4 and abs(rep["initial_rms_px"] - tw["lm"]["initial_rms"]) <= 1e-4
    # flags against the twin's outside a 10 % band around the threshold, at most 1 % of the candidates inside it
    band = np.abs(tw["margin"] - 1.0) < 0.1
    assert band.mean() <= 0.01, band.mean()
    assert np.array_equal(inl[cand].astype(bool)[~band], tw["inlier"][cand][~band])
    both = cand & np.isfinite(err) & np.isfinite(tw["err"])
    assert (np.abs(err[both] - tw["err"][both]) <= 1e-3 * np.maximum(1.0, tw["err"][both])).all()
    # Refined beats the RANSAC winner in the rms over the winner's inliers and in the robust cost (the LM minimises them: it
    # holds for the twin on every scene).  It is NOT asserted for s, R or t against the truth: a minimal sample can land closer
    # to the truth in one of them than the least-squares link (the twin's winner has the smaller error in s on scenes (1024, 61)
    # and (4096, 3)), so only the rotation, where the twin improves on all three scenes, is held to it.
    assert rep["final_rms_px"] < rep["initial_rms_px"] and tw["lm"]["final_rms"] < tw["lm"]["initial_rms"]
    assert AS.sim_errors(sim[:13], L)[1] < AS.sim_errors(sim[13:], L)[1]
    assert AS.sim_errors(AR.pack(tw["sim"]), L)[1] < AS.sim_errors(AR.pack(tw["ransac"]), L)[1]


def small_pairs(sc, keep):
    """The first link of sc with only the records `keep` of A left as candidates (the others' index set to -1)."""
    A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
    index = np.full(A["n"], -1, np.int32)
    index[keep] = L["index"][keep]
    return A, B, index


def test_degenerate_inputs(S, HL):
    sc = AS.build(257, 7, wrong_match=0.0, wrong_index=0.0)
    A, B, L = sc["pairs"][0], sc["pairs"][1], sc["links"][0]
    cand = np.flatnonzero(AS.candidates(A, B, L["index"]))
    ident = np.array([1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)

    def check_degenerate(res, m, winner_is_identity):
        sim, inl, err, counts, rep, order = res
        assert rep["status"] == S.REFINE_DEGENERATE and rep["num_candidates"] == m and rep["iterations"] == 0
        assert rep["num_inliers"] == 0 and rep["ransac_inliers"] == 0 and not inl.any()
        assert np.array_equal(sim[:13], sim[13:]) and np.array_equal(sim[:13], ident) == winner_is_identity
    # 2 candidates: no sample
    A2, B2, idx = small_pairs(sc, cand[:2])
    check_degenerate(AS.run_host(HL, S, A2, B2, idx, K=sc["K"]), 2, True)
    # every sample collinear: A's points on one line
    keep = cand[:40]
    Ac = dict(A, points=A["points"].copy())
    Ac["points"][:3, keep] = np.outer([0.1, 0.2, 1.0], np.linspace(4, 8, len(keep)))
    _, _, idx = small_pairs(sc, keep)
    res = AS.run_host(HL, S, Ac, B, idx, K=sc["K"])
    check_degenerate(res, 40, True)
    assert not res[3].any()                                                    # no hypothesis counted anything
    # a winner with 5 inliers: 5 consistent records, 30 whose point of B is moved away
    keep = cand[:35]
    Bw = dict(B, points=B["points"].copy())
    Bw["points"][:3, L["index"][keep[5:]]] *= np.linspace(1.3, 2.5, 30)[None]
    _, _, idx = small_pairs(sc, keep)
    res = AS.run_host(HL, S, A, Bw, idx, K=sc["K"])
    assert res[3].max() == 5
    check_degenerate(res, 35, False)
    res6 = AS.run_host(HL, S, A, dict(B, points=np.where(np.arange(B["n"]) == L["index"][keep[5]], B["points"], Bw["points"])), idx, K=sc["K"])
    assert res6[3].max() == 6 and res6[4]["status"] != S.REFINE_DEGENERATE and res6[4]["ransac_inliers"] == 6
    # W = 0 and a NaN column on either side, an index >= n_B, an index of -1: not candidates, nothing else changes
    full = AS.run_host(HL, S, A, B, L["index"], K=sc["K"])
    Aq, Bq, idx = dict(A, points=A["points"].copy()), dict(B, points=B["points"].copy()), L["index"].copy()
    a, b, c, d, e, f = cand[:6]
    Aq["points"][3, a] = 0.0; Aq["points"][1, b] = np.nan
    Bq["points"][3, idx[c]] = 0.0; Bq["points"][0, idx[d]] = np.nan
    idx[e] = B["n"]; idx[f] = -1
    res = AS.run_host(HL, S, Aq, Bq, idx, K=sc["K"])
    assert res[4]["num_candidates"] == full[4]["num_candidates"] - 6 and res[4]["status"] != S.REFINE_DEGENERATE
    assert not res[1][[a, b, c, d, e, f]].any() and np.isposinf(res[2][[a, b, c, d, e, f]]).all() and np.isfinite(res[0]).all()
    assert np.array_equal(res[5][:res[4]["num_candidates"]], cand[6:])
    tw = AR.run(Aq, Bq, idx, sc["K"], sc["K"])
    assert np.array_equal(tw["records"], cand[6:])


def test_chain_links_against_direct_composition(S):
    rng = np.random.default_rng(2)
    links = []
    for _ in range(5):
        w = rng.standard_normal(3)
        links.append((rng.uniform(0.5, 2.0), RR.expso3(0.3 * w), rng.uniform(-1, 1, 3)))
    chain = S.chain_links(links)
    assert len(chain) == 6 and chain[0][0] == 1.0 and np.array_equal(chain[0][1], np.eye(3)) and not chain[0][2].any()
    X0 = rng.uniform(-1, 1, (20, 3)) + [0, 0, 6]
    X = X0
    total = (1.0, np.eye(3), np.zeros(3))
    for i, l in enumerate(links):
        X = l[0] * X @ l[1].T + l[2]                                           # pair i + 1's coordinates of the same points
        total = AR.compose(l, total)
        s, R, t = chain[i + 1]
        assert np.abs(s * X @ R.T + t - X0).max() <= 1e-12
        # the chained transform is the inverse of the direct composition
        si, Ri, ti = AR.compose((s, R, t), total)
        assert abs(si - 1) <= 1e-12 and np.abs(Ri - np.eye(3)).max() <= 1e-12 and np.abs(ti).max() <= 1e-12
    # the packed 13 / 26 floats of an align_to result are accepted as they are
    packed = [np.concatenate([AR.pack(l), np.zeros(13)]).astype(np.float32) for l in links]
    for (s, R, t), (s2, R2, t2) in zip(chain, S.chain_links(packed)):
        assert abs(s - s2) <= 1e-5 and np.abs(R - R2).max() <= 1e-5 and np.abs(t - t2).max() <= 1e-5


def test_struct_layouts_match_the_header(S, HL):
    for which, T in enumerate((S.AlignParams, S.AlignReport, S.AlignOut)):
        out = (C.c_int64 * 16)()
        nf = HL.aln_layout(which, out)
        assert nf == len(T._fields_) and out[0] == C.sizeof(T), T
        assert [out[1 + i] for i in range(nf)] == [getattr(T, f).offset for f, _ in T._fields_], T


def test_ctypes_mirrors_equal_sizeof_and_offsetof_of_the_header(S, tmp_path):
    """A C program prints sizeof / offsetof of the three structs (tests/test_abi_load.py's check for the older ones)."""
    structs = {"sfm_align_params": S.AlignParams, "sfm_align_report": S.AlignReport, "sfm_align_out": S.AlignOut}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sfm_amd.h"', "int main(void) {"]
    for st, T in structs.items():
        lines.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        for f, _ in T._fields_:
            lines.append(f'  printf("{st}.{f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    seen = 0
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        tok = line.split()
        if "." in tok[0]:
            st, f = tok[0].split(".")
            d = getattr(structs[st], f)
            assert (d.offset, d.size) == (int(tok[1]), int(tok[2])), line
        else:
            assert C.sizeof(structs[tok[0]]) == int(tok[1]), line
        seen += 1
    assert seen == sum(len(T._fields_) + 1 for T in structs.values())


def test_declared_exported_wrapped_and_documented(S):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_amd.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "cuda-sfm_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = [g.strip() for g in re.search(r"global\s*:(.*?)local\s*:", script, flags=re.S).group(1).split(";") if g.strip()]
    for name in NAMES:
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
        assert name in exported and any(fnmatch.fnmatchcase(name, g) for g in globs), name
    assert re.search(r"#define\s+SFM_ABI_VERSION\s+3\b", hdr)
    for f in ("align_params", "align_pairs", "align_pairs_enqueue", "align_index_from_matches", "chain_links"):
        assert callable(getattr(S, f)), f
    assert callable(S.ImagePair.align_to) and callable(S.ImagePair.align_to_enqueue)
    p = S.align_params()
    assert (p.num_hypotheses, p.seed, p.threshold_px, p.max_iterations) == (4096, 0x5EED5F3D, 4.0, 10)
    assert (p.huber_px, p.initial_lambda) == (1.0, np.float32(1e-3)) and p.min_rel_decrease == np.float32(1e-6)
    assert not any((p.d_points_a, p.d_valid_a, p.d_points_b, p.d_valid_b)) and not any(p.reserved)
    with pytest.raises(TypeError):
        S.align_params(min_score=0.5)


def test_argument_checks_come_before_any_device_call(S):
    one, many, index = S.lib().sfm_align_pair, S.lib().sfm_align_pairs, S.lib().sfm_align_index_from_matches
    p, ref = S.align_params(), C.byref
    fake = (C.c_void_p * 1)(0x1000)                      # never dereferenced: the checks that reject the call come first
    null = (C.c_void_p * 1)(None)
    out = (S.AlignOut * 1)(S.AlignOut(0x2000, 0x3000, None, None, 0x4000))
    assert many(fake, fake, 1, fake, None, out) == S.E_INVALID                   # null p
    assert many(fake, fake, -1, fake, ref(p), out) == S.E_INVALID
    assert many(fake, fake, 65536, fake, ref(p), out) == S.E_INVALID
    for args in ((None, fake, fake, out), (fake, None, fake, out), (fake, fake, None, out), (fake, fake, fake, None),
                 (null, fake, fake, out), (fake, null, fake, out), (fake, fake, null, out)):            # null lists, null entries
        assert many(args[0], args[1], 1, args[2], ref(p), args[3]) == S.E_INVALID
    assert many(fake, fake, 1, fake, ref(p), out) == S.E_INVALID                 # a and b are the same pair
    b = (C.c_void_p * 1)(0x8000)
    for o in (S.AlignOut(None, 0x3000, None, None, 0x4000), S.AlignOut(0x2000, None, None, None, 0x4000), S.AlignOut(0x2000, 0x3000, None, None, None),
              S.AlignOut(0x2000, 0x2000, None, None, 0x4000), S.AlignOut(0x2000, 0x3000, 0x2010, None, 0x4000),
              S.AlignOut(0x2000, 0x3000, None, 0x4004, 0x4000), S.AlignOut(0x1000, 0x3000, None, None, 0x4000)):
        assert many(fake, b, 1, fake, ref(p), (S.AlignOut * 1)(o)) == S.E_INVALID, [getattr(o, f) for f, _ in o._fields_]
    assert b"links[0]" in S.lib().sfm_last_error()
    for kw in (dict(points_a=0x9000), dict(points_b=0x9000), dict(points_a=0x9000, valid_a=0x9100), dict(valid_a=0x9000), dict(valid_b=0x9000)):
        assert many(fake, b, 1, fake, ref(S.align_params(**kw)), out) == S.E_INVALID, kw
    for kw in (dict(num_hypotheses=0), dict(num_hypotheses=(1 << 20) + 1), dict(threshold_px=0.0), dict(threshold_px=float("nan")),
               dict(max_iterations=-1), dict(max_iterations=201), dict(huber_px=-1.0), dict(min_rel_decrease=float("inf")),
               dict(initial_lambda=-1.0), dict(reserved=[0, 1, 0, 0])):
        assert many(fake, b, 1, fake, ref(S.align_params(**kw)), out) == S.E_INVALID, kw
        assert many(None, None, 0, None, ref(S.align_params(**kw)), None) == S.E_INVALID, kw
    # the single call: null arguments, parameters, outputs and the same pair, all before either pair is looked at
    assert one(None, 0x8000, 0x1000, ref(p), out) == S.E_INVALID and one(0x7000, None, 0x1000, ref(p), out) == S.E_INVALID
    assert one(0x7000, 0x8000, None, ref(p), out) == S.E_INVALID and one(0x7000, 0x8000, 0x1000, None, out) == S.E_INVALID
    assert one(0x7000, 0x8000, 0x1000, ref(p), None) == S.E_INVALID
    assert one(0x7000, 0x8000, 0x1000, ref(S.align_params(reserved=[1, 0, 0, 0])), out) == S.E_INVALID
    assert one(0x7000, 0x8000, 0x1000, ref(S.align_params(valid_b=0x9000)), out) == S.E_INVALID
    assert one(0x7000, 0x8000, 0x1000, ref(p), (S.AlignOut * 1)(S.AlignOut(0x2000, 0x2000, None, None, 0x4000))) == S.E_INVALID
    assert one(0x7000, 0x7000, 0x1000, ref(p), out) == S.E_INVALID
    assert index(None, 0x1000, 4, 0.85, 0.95, 0x2000) == S.E_INVALID and index(0x7000, None, 4, 0.85, 0.95, 0x2000) == S.E_INVALID
    assert index(0x7000, 0x1000, 4, 0.85, 0.95, None) == S.E_INVALID and index(0x7000, 0x1000, -1, 0.85, 0.95, 0x2000) == S.E_INVALID
    assert index(0x7000, 0x1000, 4, float("nan"), 0.95, 0x2000) == S.E_INVALID and index(0x7000, 0x1000, 0, 0.85, 0.95, 0x2000) == S.OK


def test_an_empty_list_is_not_an_error(S):
    many = S.lib().sfm_align_pairs
    p = S.align_params()
    assert many(None, None, 0, None, C.byref(p), None) == S.OK
    assert many(None, None, 0, None, None, None) == S.E_INVALID                  # the parameters are checked whatever the count
    S.align_pairs_enqueue([], [], [], p, [])
    assert S.align_pairs([], [], []) == []


def kernel_usage():
    """{mangled kernel name: {field: value}} of build/align.usage.txt (-Rpass-analysis=kernel-resource-usage)."""
    assert os.path.exists(USAGE), "run `make`: the product build leaves the compiler's resource report next to the objects"
    out, cur = {}, None
    for line in open(USAGE):
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_resource_report():
    """No scratch in any kernel, the batched kernels within one VGPR of their twins, the score kernel's LDS is its tile: 1024
    candidates of 40 bytes."""
    usage = kernel_usage()
    assert len(usage) == 9, sorted(usage)

    def find(tail):
        hits = [v for k, v in usage.items() if k.endswith(tail)]
        assert len(hits) == 1, (tail, sorted(usage))
        return hits[0]
    for k, v in usage.items():
        assert v["ScratchSize"] == 0, (k, v)
    for stage in ("gate", "solve", "score", "refine"):
        b, s = find(f"align_{stage}_pairs_kernelEPKNS_9AlignArgsE"), find(f"align_{stage}_kernelENS_9AlignArgsE")
        print(f"align_{stage}: {s['VGPRs']} VGPRs, LDS {s['LDS Size']}; batched {b['VGPRs']} VGPRs, LDS {b['LDS Size']}")
        assert abs(b["VGPRs"] - s["VGPRs"]) <= 1 and b["LDS Size"] == s["LDS Size"], (stage, b, s)
    assert find("align_score_kernelENS_9AlignArgsE")["LDS Size"] == 1024 * 40
    assert find("align_refine_kernelENS_9AlignArgsE")["VGPRs"] <= 256
