"""CPU: the gate of sfm_match_guided and the arithmetic of sfm_pair_fundamental (cuda-sfm_amd/csrc/match_guided_math.hpp) in the
host build (tests/hostcheck/libmatchguidedcheck.so) against numpy and the fp64 twin (tests/match_guided_reference.py); what the
guided match buys over the plain one on scenes with repeated descriptors; struct layout, documents and the kernels' no-scratch
pin."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_sfm_amd as S
import match_guided_reference as MR
import match_guided_scene as MS

SCENES = ((1024, 61), (2155, 7))
BANDS = (2.0, 4.0)
f32 = np.float32


@functools.lru_cache(maxsize=None)
def lib():
    return MS.host_lib()


@functools.lru_cache(maxsize=None)
def twin(n, seed, band):
    sc = MS.scene(n, n, seed)
    return MR.match_guided(sc["sift1"], sc["sift2"], sc["F"], band)


@functools.lru_cache(maxsize=None)
def host(n, seed, band):
    sc = MS.scene(n, n, seed)
    return MS.host_run(sc["sift1"], sc["sift2"], sc["F"], band)


@functools.lru_cache(maxsize=None)
def twin_plain(n, seed):
    sc = MS.scene(n, n, seed)
    return MR.match_plain(sc["sift1"], sc["sift2"])


def gate(F, band, x1, y1, x2, y2):
    f = np.ascontiguousarray(np.asarray(F, f32).reshape(9))
    return lib().mg_gate(MS.vp(f), C.c_float(band), C.c_float(x1), C.c_float(y1), C.c_float(x2), C.c_float(y2))


# ---- the header's pieces -----------------------------------------------------------------------------------------------------
def test_line_and_residual_against_numpy():
    rng = np.random.default_rng(5)
    for _ in range(200):
        F = rng.standard_normal(9).astype(f32)
        x, y, x2, y2 = (rng.uniform(-300, 1000, 4)).astype(f32)
        l = np.empty(3, f32); lt = np.empty(3, f32)
        lib().mg_line(MS.vp(F), C.c_float(x), C.c_float(y), MS.vp(l))
        lib().mg_line_t(MS.vp(F), C.c_float(x), C.c_float(y), MS.vp(lt))
        F64 = F.astype(np.float64).reshape(3, 3)
        u = np.array([x, y, 1.0], np.float64)
        scale = np.abs(F64) @ np.abs(u)
        assert np.all(np.abs(l - F64 @ u) <= 4 * 2.0 ** -24 * scale)
        assert np.all(np.abs(lt - F64.T @ u) <= 4 * 2.0 ** -24 * (np.abs(F64).T @ np.abs(u)))
        # the fused chain itself, bit for bit: l_r = fma(F[3r], x, fma(F[3r+1], y, F[3r+2])), each fma one rounding of the exact value
        for r in range(3):
            inner = f32(np.float64(F[3 * r + 1]) * np.float64(y) + np.float64(F[3 * r + 2]))       # (exact in fp64 up to its own rounding: 24 + 24 bits)
            want = f32(np.float64(F[3 * r]) * np.float64(x) + np.float64(inner))
            assert abs(float(l[r]) - float(want)) <= abs(float(want)) * 2.0 ** -23
        d = lib().mg_residual(MS.vp(l), C.c_float(x2), C.c_float(y2))
        dd = float(l[0]) * float(x2) + float(l[1]) * float(y2) + float(l[2])
        assert abs(d - dd) <= 3 * 2.0 ** -24 * (abs(float(l[0]) * float(x2)) + abs(float(l[1]) * float(y2)) + abs(float(l[2])))
        lim = lib().mg_limit(MS.vp(l), C.c_float(3.0))
        assert abs(lim - 9.0 * (float(l[0]) ** 2 + float(l[1]) ** 2)) <= 4 * 2.0 ** -24 * lim


def test_gate_nan_zero_epipole_symmetry():
    sc = MS.scene(1024, 1024, 61)
    F = sc["F"]
    s1, s2, truth = sc["sift1"], sc["sift2"], sc["truth"]
    i = 3
    j = int(truth[i])
    x1, y1, x2, y2 = float(s1["xpos"][i]), float(s1["ypos"][i]), float(s2["xpos"][j]), float(s2["ypos"][j])
    assert gate(F, 4.0, x1, y1, x2, y2) == 1                              # a true pair (0.5 px of noise) is in a 4 px band
    assert gate(F, 4.0, x1, y1, x2 + 60.0, y2 + 60.0) == 0                # and a point 85 px away is not
    nan = float("nan")
    for bad in ((nan, y1, x2, y2), (x1, nan, x2, y2), (x1, y1, nan, y2), (x1, y1, x2, nan)):
        assert gate(F, 4.0, *bad) == 0
    assert gate(F, nan, x1, y1, x2, y2) == 0
    assert gate(np.zeros(9), 1e6, x1, y1, x2, y2) == 0                    # a zero F passes nothing, whatever the band
    for k in range(9):
        for v in (nan, float("inf"), -float("inf")):
            Fb = np.array(F, np.float64).reshape(9); Fb[k] = v
            assert gate(Fb, 1e6, x1, y1, x2, y2) == 0, (k, v)
    assert lib().mg_pass(C.c_float(0.0), C.c_float(0.0), C.c_float(1.0)) == 0 and lib().mg_pass(C.c_float(0.0), C.c_float(1.0), C.c_float(0.0)) == 0
    assert lib().mg_pass(C.c_float(1.0), C.c_float(1.0), C.c_float(1.0)) == 1 and lib().mg_pass(C.c_float(-1.0), C.c_float(1.0), C.c_float(2.0)) == 1
    assert lib().mg_pass(C.c_float(1.5), C.c_float(4.0), C.c_float(2.0)) == 0
    # a feature ON the epipole has no line: an F whose right null vector is (100, 50, 1) in fp32 exactly
    e1 = np.array([100.0, 50.0, 1.0])
    A = np.array([[0.0, -1.0, 50.0], [1.0, 0.0, -100.0], [-50.0, 100.0, 0.0]])        # [e1]x: A e1 = 0, small integers
    assert np.all(A @ e1 == 0)
    assert gate(A, 1e6, 100.0, 50.0, 7.0, 9.0) == 0
    assert gate(A, 1e6, 101.0, 50.0, 7.0, 9.0) == 1
    assert gate(A.T, 1e6, 7.0, 9.0, 100.0, 50.0) == 0                                  # the other view's epipole
    # symmetry: the gate of (u1, u2) under F is the gate of (u2, u1) under F^T
    rng = np.random.default_rng(9)
    F32 = np.asarray(F, f32).reshape(3, 3)
    seen = set()
    for _ in range(4000):
        a = int(rng.integers(0, 1024)); b = int(truth[a]) if rng.random() < 0.5 else int(rng.integers(0, 1024))
        p = (float(s1["xpos"][a]), float(s1["ypos"][a]), float(s2["xpos"][b]), float(s2["ypos"][b]))
        g = gate(F32, 2.0, *p)
        assert g == gate(F32.T.copy(), 2.0, p[2], p[3], p[0], p[1])
        seen.add(g)
    assert seen == {0, 1}


def test_params_layout_against_the_ctypes_mirror(tmp_path):
    fields = ["band_px", "reserved"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sfm_amd.h"', 'int main(void) {',
             '  sfm_match_guided_params p; sfm_match_guided_default_params(&p);',
             '  printf("size %zu\\n", sizeof(sfm_match_guided_params));']
    for f in fields:
        lines.append(f'  printf("{f} %zu %zu\\n", offsetof(sfm_match_guided_params, {f}), sizeof(p.{f}));')
    lines += ['  printf("band %g %d %d %d %d\\n", p.band_px, p.reserved[0], p.reserved[1], p.reserved[2], p.reserved[3]);', '  return 0;', '}']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    libdir = os.path.join(MS.ROOT, "cuda-sfm_amd", "lib")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(MS.ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsfm_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict((l.split()[0], l.split()[1:]) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"][0]) == C.sizeof(S.MatchGuidedParams) == 20
    assert [f for f, _ in S.MatchGuidedParams._fields_] == fields
    for f in fields:
        d = getattr(S.MatchGuidedParams, f)
        assert tuple(int(x) for x in out[f]) == (d.offset, d.size)
    assert out["band"] == ["4", "0", "0", "0", "0"]
    p = S.match_guided_params()
    assert p.band_px == 4.0 and list(p.reserved) == [0, 0, 0, 0]
    assert S.match_guided_params(band_px=2.5, reserved=(0, 1, 0, 0)).reserved[1] == 1
    assert C.sizeof(S.MatchGuidedParams) == lib().mg_sizeof_params()


def test_documents():
    read = lambda *p: open(os.path.join(MS.ROOT, *p)).read()
    design = read("DESIGN.md")
    m = re.search(r"^##+ *6n\b.*?(?=^##+ *(?:6o|7)\b|\Z)", design, re.S | re.M)
    assert m, "DESIGN.md has no section 6n"
    sec = m.group(0)
    for word in ("sfm_match_guided", "sfm_pair_fundamental", "band", "ticket", "scratch", "Out of scope", "tiles", "pre-filter", "_soa", "batched",
                 "chain stages", "16384"):
        assert word in sec, word
    assert "sfm_pair_fundamental" in re.search(r"^##+ *6d\b.*?(?=^##+ *6e\b)", design, re.S | re.M).group(0)
    readme = read("README.md")
    assert "sfm_match_guided" in readme and "guided_match_demo" in readme
    integ = read("INTEGRATION.md")
    for name in ("sfm_match_guided_default_params", "sfm_match_guided", "sfm_pair_fundamental"):
        assert name in integ and name in S.EXPORTS


def test_kernels_use_no_scratch():
    """build/match_guided.usage.txt (written next to the object): no scratch in any kernel of match_guided.hip, the two matcher
    configurations present, their LDS the descriptor buffers plus 2 KiB of row positions."""
    path = os.path.join(MS.ROOT, "build", "match_guided.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make builds it with the library"
    text = open(path).read()
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", text, re.S):
        found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    kernels = {k: v for k, v in found.items() if "match_guided_kernel" in k}
    print("match_guided.hip (VGPRs, scratch, LDS):", found)
    assert len(kernels) == 2 and len(found) == 3, found
    for name, (vgprs, scratch, lds) in found.items():
        assert scratch == 0, (name, scratch)
    for name, (vgprs, scratch, lds) in kernels.items():
        assert vgprs <= 256 and 2 * 64 * 132 * 4 + 2048 <= lds <= 2 * 64 * 132 * 4 + 2048 + 64, (name, vgprs, lds)


# ---- the host build against the twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("n,seed", SCENES)
def test_host_build_equals_the_twin(n, seed, band):
    sc = MS.scene(n, n, seed)
    wide, narrow, undecided = twin(n, seed, band)
    got = host(n, seed, band)
    tied = wide["tied"] | narrow["tied"]
    print(f"scene ({n}, {seed}) band {band}: undecided {int(undecided.sum())}, tied {int(tied.sum())} of {n} queries; "
          f"matched {int((got['match'] >= 0).sum())}")
    # the twin alone stays inside both caps: the scenes are fit for the comparison
    assert undecided.sum() <= 0.01 * n and tied.sum() <= 0.01 * n
    m = got["match"].astype(np.int64)
    sure = ~undecided & ~tied
    assert np.array_equal(m[sure], wide["match"][sure])
    assert np.all((m[undecided] == wide["match"][undecided]) | (m[undecided] == narrow["match"][undecided]))
    t = tied & ~undecided
    assert np.all((m[t] == wide["match"][t]) | (m[t] == wide["runner_up"][t]))
    # scores and ambiguity at 2e-5 relative, positions exactly, wherever the match is the twin's
    for ref in (wide, narrow):
        same = (m == ref["match"]) & ~tied
        assert np.all(np.abs(got["score"][same] - ref["score"][same]) <= 2e-5 * ref["score"][same])
        assert np.array_equal(got["match_xpos"][same].astype(np.float64), ref["match_xpos"][same])
        assert np.array_equal(got["match_ypos"][same].astype(np.float64), ref["match_ypos"][same])
    # ambiguity = second / (best + 1e-6): where the twin's runner-up does not hang on a row at the band's edge either
    stable = sure & (wide["runner_up"] == narrow["runner_up"])
    print(f"  ambiguity compared on {int(stable.sum())} queries")
    assert stable.sum() >= 0.97 * n
    assert np.all(np.abs(got["ambiguity"][stable] - wide["ambiguity"][stable]) <= 2e-5 * wide["ambiguity"][stable])
    none = m < 0
    assert np.all(got["score"][none] == 0) and np.all(got["ambiguity"][none] == 0) and np.all(got["match_xpos"][none] == 0)
    # nothing but the five match fields moves
    for f in ("xpos", "ypos", "scale", "data", "match_error", "subsampling"):
        assert np.array_equal(got[f], sc["sift1"][f])


def test_host_build_plain_equals_the_twins_plain_match():
    """gated = 0 is sfm_match: the comparison of the counts below is between like and like"""
    n, seed = SCENES[0]
    sc = MS.scene(n, n, seed)
    got = MS.host_run(sc["sift1"], sc["sift2"], sc["F"], 4.0, gated=False)
    ref = twin_plain(n, seed)
    ok = ~ref["tied"]
    assert np.array_equal(got["match"][ok].astype(np.int64), ref["match"][ok])
    assert np.all(np.abs(got["score"] - ref["score"]) <= 2e-5 * ref["score"])
    huge = MS.host_run(sc["sift1"], sc["sift2"], sc["F"], 1e6)
    assert MS.fields_equal(huge, got)                                      # a band of 1e6 px gates nothing out


# ---- what it buys --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", SCENES)
def test_guided_accepts_more_correct_matches_and_no_more_wrong_ones(n, seed):
    sc = MS.scene(n, n, seed)
    ref = twin_plain(n, seed)
    plain = np.zeros(n, S.SIFT_DTYPE)
    plain["match"] = ref["match"]; plain["score"] = ref["score"]; plain["ambiguity"] = ref["ambiguity"]
    pc, pw = MS.accepted(plain, sc["truth"])
    for band in BANDS:
        gc, gw = MS.accepted(host(n, seed, band), sc["truth"])
        print(f"scene ({n}, {seed}): plain accepted {pc + pw} ({pc} correct / {pw} wrong); guided at {band} px accepted {gc + gw} ({gc} / {gw})")
        assert gc > pc and gw <= pw


# ---- sfm_pair_fundamental's host form ---------------------------------------------------------------------------------------------
def test_fundamental_against_numpy():
    rng = np.random.default_rng(11)
    for trial in range(100):
        E = rng.standard_normal((3, 3)).astype(f32)
        K = np.array([[rng.uniform(500, 3000), rng.uniform(-2, 2), rng.uniform(200, 900)], [0, rng.uniform(500, 3000), rng.uniform(200, 900)], [0, 0, 1]])
        Kinv = np.linalg.inv(K).astype(f32)
        Ki = Kinv.astype(np.float64)
        for refined in (0, 1):
            M = E.astype(np.float64) if refined else E.astype(np.float64).T
            G = Ki.T @ M @ Ki
            want = G / np.linalg.norm(G)
            got = MS.host_fundamental(E, Kinv, refined).astype(np.float64).reshape(3, 3)
            assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 1e-12 * np.abs(want).max())
            assert abs(np.linalg.norm(got) - 1.0) < 1e-6
    Kinv = np.linalg.inv(np.array([[2360.0, 0, 360], [0, 2360.0, 288], [0, 0, 1]])).astype(f32)
    assert np.all(MS.host_fundamental(np.zeros(9, f32), Kinv, 1) == 0)
    for v in (np.nan, np.inf):
        E = np.eye(3, dtype=f32); E[1, 2] = v
        assert np.all(MS.host_fundamental(E, Kinv, 0) == 0) and np.all(MS.host_fundamental(E, Kinv, 1) == 0)


def test_fundamental_convention_on_a_pairs_own_records():
    """fill_xu reads view 1 from (xpos, ypos) and view 2 from (match_xpos, match_ypos); the oracle's E has X0^T E X1 = 0.  The host
    form with refined = 0 must turn such an E into an F with u2^T F u1 = 0, and with refined = 1 an E = [t]x R (X2 = R X1 + t)."""
    import sys
    sys.path.insert(0, os.path.join(MS.ROOT, "oracle"))
    import oracle as O
    from cuda_sfm_amd import synth
    sc = synth.two_view_scene(512, noise_px=0.0, outlier_frac=0.0)
    t, R = sc["t"], sc["R"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E_textbook = (tx @ R).astype(f32)                                      # X1^T E X0 = 0
    _, _, X0, X1 = O.fill_xu(sc["sift"], sc["Kinv"])
    # the oracle's residual is small under the TRANSPOSE of the textbook E: its convention is X0^T E X1 = 0
    r_t = [O.residual(E_textbook.T.copy(), X0[:, j], X1[:, j]) for j in range(8)]
    r_n = [O.residual(E_textbook, X0[:, j], X1[:, j]) for j in range(8)]
    assert max(r_t) < 1e-9 < min(r_n)
    u1 = np.stack([sc["sift"]["xpos"], sc["sift"]["ypos"], np.ones(512, f32)]).astype(np.float64)
    u2 = np.stack([sc["sift"]["match_xpos"], sc["sift"]["match_ypos"], np.ones(512, f32)]).astype(np.float64)
    for E, refined in ((E_textbook.T.copy(), 0), (E_textbook, 1)):
        F = MS.host_fundamental(E, sc["Kinv"], refined).astype(np.float64).reshape(3, 3)
        l = F @ u1
        dist = np.abs(np.sum(u2 * l, 0)) / np.hypot(l[0], l[1])
        assert dist.max() < 0.05, (refined, dist.max())                   # pixels; the wrong transposition gives tens of pixels
        Fw = MS.host_fundamental(E, sc["Kinv"], 1 - refined).astype(np.float64).reshape(3, 3)
        lw = Fw @ u1
        assert np.median(np.abs(np.sum(u2 * lw, 0)) / np.hypot(lw[0], lw[1])) > 5.0
