"""CPU: sfm_triangulate_view / sfm_triangulate_views without a device -- header, exports, Python mirror and INTEGRATION.md agree,
the argument checks answer before any device call, the host build of the arithmetic (tests/hostcheck/libviewpointscheck.so)
against the fp64 twin (tests/view_points_reference.py) on the checked scenes with exact cameras, low parallax, monotone cost,
and the compiler's resource report of view_points.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import register_scene as RS
import view_points_reference as VR
import view_points_scene as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sfm_view_points_default_params", "sfm_triangulate_view", "sfm_triangulate_views"]
# |X32 - X64| / |X64| over the accepted points of the three scenes: measured maximum 1.91e-5 (scene (4096, 3); median 1.3e-7 --
# the depth of a point seen under a few degrees is what moves), the bar 4 x that.  The factor covers the host build's fp32 sums
# taken in another order than numpy's and nothing else.
REL_MEASURED, REL_BAR = 1.91e-5, 7.64e-5
# monotone cost: the largest excess of the output's fp64 Huber cost over the start point's that the host build shows on the three
# scenes is negative (every class-2 point's cost went down or stayed: largest difference -1.4e-4 px^2), so the slack, 4 x the
# largest excess, is 0
COST_SLACK = 0.0


@pytest.fixture(scope="module")
def S():
    import cuda_sfm_amd as S
    return S


@pytest.fixture(scope="module")
def HL():
    return VS.host_lib()


@pytest.fixture(scope="module")
def runs(S, HL):
    """Per checked scene: the scene, the fp64 twin's result and the host build's, computed once."""
    out = []
    for n, seed in VS.SCENES:
        s = VS.build(n, seed)
        ref = VR.view_points(s["sc"]["K"], s["sc"]["Kinv"], s["rec"], s["X0"], s["X1"], s["points"], s["valid"], s["P2"], s["P3"])
        out.append((s, ref, VS.run_host(HL, S, s)))
    return out


def band(ref, threshold_px=4.0, min_parallax_deg=1.0):
    """Points whose fp64 error lies within 10 % of the threshold or whose parallax lies within 10 % of the smallest accepted."""
    with np.errstate(invalid="ignore"):
        return ref["seen"] & ((np.abs(ref["err"] - threshold_px) <= 0.1 * threshold_px) |
                              (np.abs(ref["parallax"] - min_parallax_deg) <= 0.1 * min_parallax_deg))


def test_header_exports_wrapper_and_integration_md_agree(S):
    hdr = open(os.path.join(ROOT, "include", "sfm_amd.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in S.EXPORTS and hasattr(S.lib(), name) and re.search(rf"\b{name}\s*\(", hdr) and name in doc, name
    assert S.lib().sfm_abi_version() == 3 and S.ABI_VERSION == 3
    for k, name in enumerate(("UNSEEN", "NEW", "REFINED", "NEW_REJECTED", "KEPT")):
        assert getattr(S, "VP_" + name) == k == getattr(VR, name)
        assert re.search(rf"^#define\s+SFM_VP_{name}\s+{k}\b", hdr, flags=re.M), name
    for fn in ("view_points_params", "triangulate_views_enqueue", "triangulate_views"):
        assert callable(getattr(S, fn))
    for fn in ("triangulate_view_enqueue", "triangulate_view"):
        assert callable(getattr(S.ImagePair, fn))
    p = S.view_points_params()
    got = (p.threshold_px, p.min_score, p.max_ambiguity, p.min_parallax_deg, p.max_iterations, p.huber_px, p.min_rel_decrease, p.initial_lambda)
    want = (4.0, 0.85, 0.95, 1.0, 5, 1.0, 1e-6, 1e-3)
    assert np.allclose(got, want, rtol=1e-6) and not p.d_points and not p.d_valid and not p.d_poses and list(p.reserved) == [0] * 4


def test_ctypes_mirrors_equal_sizeof_and_offsetof_of_the_header(S, HL, tmp_path):
    fields = {"sfm_view_points_params": [f for f, _ in S.ViewPointsParams._fields_], "sfm_view_points_out": [f for f, _ in S.ViewPointsOut._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sfm_amd.h"', 'int main(void) {']
    for st, fs in fields.items():
        lines.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        for f in fs:
            lines.append(f'  printf("{st}.{f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st} *)0)->{f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = tuple(int(x) for x in v)
    for which, (st, cls) in enumerate((("sfm_view_points_params", S.ViewPointsParams), ("sfm_view_points_out", S.ViewPointsOut))):
        assert got[st] == (C.sizeof(cls),), (st, got[st], C.sizeof(cls))
        for f in fields[st]:
            d = getattr(cls, f)
            assert got[f"{st}.{f}"] == (d.offset, d.size), (st, f, got[f"{st}.{f}"], d.offset, d.size)
        lay = (C.c_int64 * 16)()                       # the host build of the same header (HIP host compiler)
        k = HL.vp_layout(which, lay)
        assert k == len(fields[st]) and lay[0] == C.sizeof(cls)
        assert [lay[1 + i] for i in range(k)] == [getattr(cls, f).offset for f in fields[st]]


def test_argument_checks_answer_before_any_device_call(S):
    """Every pointer below is a made-up address: a check that came after a dereference or a device call would not return."""
    L = S.lib()
    fake_pair, fake_sift, fake_buf = C.c_void_p(0x1000), C.c_void_p(0x2000), 0x3000
    out = S.ViewPointsOut(fake_buf, fake_buf + 0x100000, None, None)
    ok = S.view_points_params()
    single = lambda p, o=out, pair=fake_pair, sift=fake_sift: L.sfm_triangulate_view(pair, sift, C.byref(p) if p is not None else None,
                                                                                     C.byref(o) if o is not None else None)
    assert single(ok, pair=None) == S.E_INVALID and single(ok, sift=None) == S.E_INVALID
    assert single(None) == S.E_INVALID and single(ok, o=None) == S.E_INVALID
    nan, inf = float("nan"), float("inf")
    bad = (dict(reserved=[0, 0, 0, 1]), dict(reserved=[1, 0, 0, 0]), dict(max_iterations=-1), dict(max_iterations=51), dict(threshold_px=0.0),
           dict(threshold_px=nan), dict(threshold_px=inf), dict(min_score=nan), dict(max_ambiguity=inf), dict(min_parallax_deg=-0.5),
           dict(min_parallax_deg=90.5), dict(min_parallax_deg=nan), dict(huber_px=-1.0), dict(huber_px=inf), dict(min_rel_decrease=-1.0),
           dict(min_rel_decrease=nan), dict(initial_lambda=-1.0), dict(initial_lambda=inf))
    for kw in bad:
        assert single(S.view_points_params(**kw)) == S.E_INVALID, kw
        assert L.sfm_triangulate_views(None, 0, None, C.byref(S.view_points_params(**kw)), None) == S.E_INVALID, kw
    assert single(ok, o=S.ViewPointsOut(None, fake_buf, None, None)) == S.E_INVALID          # required outputs
    assert single(ok, o=S.ViewPointsOut(fake_buf, None, None, None)) == S.E_INVALID
    assert single(S.view_points_params(valid=fake_buf)) == S.E_INVALID                          # d_valid without d_points
    assert single(S.view_points_params(points=fake_buf)) == S.E_INVALID                         # out->d_points == p->d_points
    assert b"input points" in L.sfm_last_error()
    assert single(ok, sift=C.c_void_p(0x2008)) == S.E_INVALID and b"16-byte aligned" in L.sfm_last_error()
    with pytest.raises(TypeError):
        S.view_points_params(max_iteration=0)                                                    # a misspelt field is not ignored
    # the batched call
    vp = C.c_void_p
    many = lambda pairs, n, sifts, p, outs: L.sfm_triangulate_views(pairs, n, sifts, C.byref(p) if p is not None else None, outs)
    pairs2 = (vp * 2)(0x1000, None)
    sifts2 = (vp * 2)(0x2000, 0x2000)
    outs2 = (S.ViewPointsOut * 2)(out, S.ViewPointsOut(fake_buf + 0x200000, fake_buf + 0x300000, None, None))
    assert many(None, 0, None, ok, None) == S.OK                                               # an empty list
    assert many(pairs2, 0, sifts2, ok, outs2) == S.OK
    assert many(pairs2, 2, sifts2, None, outs2) == S.E_INVALID
    assert many(pairs2, -1, sifts2, ok, outs2) == S.E_INVALID and many(pairs2, 65536, sifts2, ok, outs2) == S.E_INVALID
    assert many(None, 2, sifts2, ok, outs2) == S.E_INVALID and many(pairs2, 2, None, ok, outs2) == S.E_INVALID
    assert many(pairs2, 2, sifts2, ok, None) == S.E_INVALID
    assert many(pairs2, 2, sifts2, ok, outs2) == S.E_INVALID and b"pairs[1] is null" in L.sfm_last_error()
    assert many((vp * 2)(None, 0x1000), 2, sifts2, ok, outs2) == S.E_INVALID and b"pairs[0] is null" in L.sfm_last_error()
    assert many((vp * 1)(0x1000), 1, (vp * 1)(None), ok, outs2) == S.E_INVALID and b"d_sifts[0]" in L.sfm_last_error()
    assert many((vp * 1)(0x1000), 1, (vp * 1)(0x2004), ok, outs2) == S.E_INVALID and b"d_sifts[0] must be 16-byte aligned" in L.sfm_last_error()
    assert many((vp * 1)(0x1000), 1, sifts2, ok, (S.ViewPointsOut * 1)(S.ViewPointsOut(fake_buf, None, None, None))) == S.E_INVALID
    for kw in (dict(points=fake_buf + 0x400000), dict(poses=fake_buf), dict(points=fake_buf + 0x400000, valid=fake_buf)):
        assert many((vp * 1)(0x1000), 1, sifts2, S.view_points_params(**kw), outs2) == S.E_INVALID, kw
        assert many(None, 0, None, S.view_points_params(**kw), None) == S.E_INVALID, kw


def test_checked_inputs_in_fp64(runs):
    """What the issue states about the three scenes, with the true cameras in fp64."""
    wrong_new = []
    seen_total = near_threshold = 0
    for s, ref, _ in runs:
        f, out3 = ref["flags"], s["truth"]["outlier"]
        accepted = (f == VR.NEW) | (f == VR.REFINED)
        assert accepted[ref["seen"] & ~out3].all()                       # every truly good seen record is accepted
        fresh = ref["seen"] & ~ref["usable"]
        wrong_new.append(int((fresh & out3).sum()))
        assert not (accepted & out3).any()                               # no record with a wrong view-3 match, new or refined
        P = s["sc"]["points3d"]
        m = f == VR.REFINED
        d3 = np.linalg.norm(ref["points"][:3, m].T - P[m], axis=1)
        d2 = np.linalg.norm(s["points"][:3, m].T.astype(np.float64) - P[m], axis=1)
        ratio = np.sqrt((d3 ** 2).mean() / (d2 ** 2).mean())
        assert 0.535 <= ratio < 0.585, ratio                              # 0.54-0.58 to two digits (measured 0.583, 0.544, 0.553)
        seen_total += int(ref["seen"].sum())
        near_threshold += int((ref["seen"] & (np.abs(ref["err"] - 4.0) <= 0.4)).sum())
        par = ref["parallax"][ref["seen"] & np.isfinite(ref["parallax"])]        # every seen record that has one, accepted or not
        assert len(par) and not (np.abs(par - 1.0) <= 0.1).any()
        assert ref["parallax"][f == VR.NEW].min() >= 9.7                   # measured 10.09, 10.46, 9.88 degrees
    assert wrong_new == [89, 26, 337]
    assert near_threshold <= 4, (near_threshold, seen_total)


def test_host_build_agrees_with_the_fp64_twin(runs):
    worst, excluded, seen = 0.0, 0, 0
    for s, ref, (pts, flags, err, counts) in runs:
        ex = band(ref)
        excluded += int(ex.sum()); seen += int(ref["seen"].sum())
        assert np.array_equal(flags[~ex], ref["flags"][~ex])
        assert np.array_equal(counts[:5], np.bincount(flags, minlength=5)) and not counts[5:].any()
        acc = ~ex & ((flags == VR.NEW) | (flags == VR.REFINED))
        X64, X32 = ref["points"][:3, acc].T, pts[:3, acc].T.astype(np.float64)
        rel = np.linalg.norm(X32 - X64, axis=1) / np.linalg.norm(X64, axis=1)
        worst = max(worst, float(rel.max()))
        assert (pts[3, acc] == 1.0).all()
        keep = ~acc
        assert np.array_equal(pts[:, keep].view(np.uint32), s["points"][:, keep].view(np.uint32))      # the input column, byte for byte
        assert np.isposinf(err[flags == VR.UNSEEN]).all()
        fin = ref["seen"] & np.isfinite(ref["err"])
        assert np.abs(err[fin] - ref["err"][fin]).max() < 0.05         # px: the error that is reported
    print(f"largest |X32 - X64| / |X64| over accepted points {worst:.3e} (measured {REL_MEASURED:.2e}, bar {REL_BAR:.2e}); "
          f"{excluded} of {seen} seen records inside a band")
    assert worst <= REL_BAR
    assert excluded <= 0.01 * seen


def test_low_parallax_points_are_rejected_unless_asked_for(S, HL):
    t3 = 0.05 * RS.T3_DEFAULT / np.linalg.norm(RS.T3_DEFAULT)
    s = VS.build(1024, 61, noise3=0.0, outlier3=0.0, gated3=0.0, R3=np.eye(3), t3=t3)
    ref = VR.view_points(s["sc"]["K"], s["sc"]["Kinv"], s["rec"], s["X0"], s["X1"], s["points"], s["valid"], s["P2"], s["P3"])
    fresh = ref["seen"] & ~ref["usable"]
    ang = ref["parallax"][fresh]
    print(f"{int(fresh.sum())} seen records without a usable point, parallax {ang.min():.2f} .. {ang.max():.2f} deg")
    assert fresh.sum() > 200 and 0.3 < ang.min() and ang.max() < 0.75
    _, flags, _, counts = VS.run_host(HL, S, s)
    assert (flags[fresh] == VR.NEW_REJECTED).all() and counts[VR.NEW] == 0
    pts0, flags0, _, counts0 = VS.run_host(HL, S, s, min_parallax_deg=0.0)
    assert (flags0[fresh] == VR.NEW).all() and counts0[VR.NEW_REJECTED] == 0 and np.isfinite(pts0[:, fresh]).all()
    assert np.array_equal(flags[~fresh], flags0[~fresh])


def test_refined_points_never_cost_more_than_their_start(runs):
    for s, ref, (pts, flags, _, _) in runs:
        m = flags == VR.REFINED
        K = s["sc"]["K"].astype(np.float64)
        start = (s["points"][:3, m].astype(np.float64) / s["points"][3, m].astype(np.float64)).T
        c0 = VR.huber_cost(K, s["P2"], s["P3"], True, ref["obs"][m], start, 1.0)
        c1 = VR.huber_cost(K, s["P2"], s["P3"], True, ref["obs"][m], pts[:3, m].T.astype(np.float64), 1.0)
        print(f"n = {s['n']}: largest cost(output) - cost(start) {np.max(c1 - c0):.3e} px^2 over {int(m.sum())} points")
        assert (c1 <= c0 + COST_SLACK).all()


def usage_of(path):
    """kernel name -> {field: int} from the compiler's resource-usage remarks."""
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_kernels_use_no_scratch_and_the_batched_one_has_its_twins_registers():
    path = os.path.join(ROOT, "build", "view_points.usage.txt")
    assert os.path.exists(path), f"{path} is missing: make writes it"
    u = usage_of(path)
    assert len(u) == 2, sorted(u)
    for name, f in u.items():
        assert f["ScratchSize"] == 0, (name, f)
    single = next(f for k, f in u.items() if "view_points_kernel" in k)
    batched = next(f for k, f in u.items() if "view_points_views_kernel" in k)
    print(f"view_points_kernel {single['VGPRs']} VGPRs, view_points_views_kernel {batched['VGPRs']} VGPRs")
    assert batched["VGPRs"] == single["VGPRs"] <= 128


def test_record_is_read_with_one_8_byte_and_one_16_byte_load():
    """The instruction text of the product's build (build/view_points.s): in each kernel the record is ONE global_load_dwordx2 at +24
    and ONE global_load_dwordx4 at +32, both behind nothing but the j < n guard and issued before the first wait for memory; no
    other wide vector load exists in the kernels."""
    path = os.path.join(ROOT, "build", "view_points.s")
    assert os.path.exists(path), f"{path} is missing: make writes it"
    text = open(path).read()
    bodies = re.findall(r"^_ZN3sfm\d+(view_points(?:_views)?_kernel)E\w*:[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M)
    assert sorted(k for k, _ in bodies) == ["view_points_kernel", "view_points_views_kernel"]
    for name, body in bodies:
        lines = [ln.strip() for ln in body.splitlines()]
        wide = [(i, ln) for i, ln in enumerate(lines) if re.match(r"(global|flat|buffer)_load_dwordx[234]\b", ln)]
        assert len(wide) == 2, (name, wide)
        (i2, l2), (i4, l4) = wide
        assert l2.startswith("global_load_dwordx2") and l2.endswith("offset:24"), (name, l2)
        assert l4.startswith("global_load_dwordx4") and l4.endswith("offset:32"), (name, l4)
        assert not [ln for ln in lines if ln.startswith("flat_load")], name
        before = lines[:i4]
        assert sum("saveexec" in ln for ln in before) == 1, name               # the j < n guard, nothing else
        assert not [ln for ln in before if "vmcnt" in ln], name                # no wait for memory in front of either load
