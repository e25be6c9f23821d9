"""Inputs of the sfm_adjust_chain tests (helper, not a test): sfm_fuse_chain's results of a fuse_scene chain as the arrays the call
reads, the wrapper around the host build (tests/hostcheck/libchainadjustcheck.so), and the camera errors against the truth."""
import ctypes as C
import os

import numpy as np

import fuse_scene as FS

ROOT = FS.ROOT


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libchainadjustcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.chain_adjust_run.restype = None
    h.chain_adjust_run.argtypes = [C.c_int] + [C.c_void_p] * 9
    h.chain_adjust_jacobian.restype = None
    h.chain_adjust_jacobian.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    h.chain_adjust_residual.restype = None
    h.chain_adjust_residual.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    h.chain_adjust_start_state.restype = None
    h.chain_adjust_start_state.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    h.chain_adjust_camera_step.restype = None
    h.chain_adjust_camera_step.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    h.chain_adjust_track_terms.restype = None
    h.chain_adjust_track_terms.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
    h.chain_adjust_band_at.restype = C.c_int64
    h.chain_adjust_band_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    h.chain_adjust_layout.argtypes = [C.c_int, C.c_void_p]
    return h


def fused_arrays(res, k, N):
    """fuse_scene.results' dict -> host arrays in the order of sfm_adjust_chain_in behind `pairs` (root, cams, track_offset, obs_cam,
    obs_record, points, flags, counts), padded to the lengths sfm_fuse_out has."""
    T, M = len(res["flags"]), len(res["obs_cam"])
    pad = lambda a, n, dt: np.concatenate([np.asarray(a, dt).ravel(), np.zeros(n - np.asarray(a).size, dt)])
    pts = np.zeros((4, N), np.float32); pts[:, :T] = res["points"]
    counts = np.zeros(8, np.int32)
    counts[:6] = [res["counts"][c] for c in ("tracks", "observations", "refined", "kept", "segments", "longest_track")]
    return [np.ascontiguousarray(res["root"], np.int32), np.ascontiguousarray(res["cams"], np.float32).ravel(), pad(res["track_offset"], N + 1, np.int32),
            pad(res["obs_cam"], 2 * N, np.int32), pad(res["obs_record"], 2 * N, np.int32), pts.ravel(), pad(res["flags"], N, np.uint8), counts]


def empty_outputs(S, k, N, fill=0):
    return [np.full(24 * k, fill, np.float32), np.full(4 * N, fill, np.float32), np.full(N, fill, np.uint8), np.full(N, fill, np.float32),
            np.full(k * S.ADJUST_CHAIN_REPORT_DTYPE.itemsize, fill, np.uint8)]


def results(S, outs, k, N, T):
    cams, pts, used, err, rep = outs
    return dict(cams=cams.reshape(k, 2, 12), points=pts.reshape(4, N)[:, :T].copy(), used=used[:T].copy(), err=err[:T].copy(),
                reports=rep.view(S.ADJUST_CHAIN_REPORT_DTYPE).copy())


def run_host(HL, S, chain, fused, **kw):
    """The host build over a chain's pairs and the arrays of fused_arrays, AdjustChainParams fields kw: results' dict + `accepts`
    (k x 64: per root and iteration 1 accepted, 2 rejected, 3 failed solve)."""
    p = S.adjust_chain_params(**kw)
    pairs = chain["pairs"]
    k = len(pairs)
    N = sum(P["n"] for P in pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = dict(X0=[f32(P["X0"]) for P in pairs], X1=[f32(P["X1"]) for P in pairs], K=[f32(P.get("K", chain["K"])) for P in pairs])
    tables = {name: (C.c_void_p * k)(*[a.ctypes.data for a in arrs]) for name, arrs in keep.items()}
    n = np.array([P["n"] for P in pairs], np.int32); ld = np.array([P["ld"] for P in pairs], np.int32)
    outs = empty_outputs(S, k, N)
    accepts = np.zeros((k, 64), np.uint8)
    i = S.AdjustChainIn(None, *[a.ctypes.data for a in fused])
    o = S.AdjustChainOut(*[a.ctypes.data for a in outs])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    HL.chain_adjust_run(k, vp(n), vp(ld), C.cast(tables["X0"], C.c_void_p), C.cast(tables["X1"], C.c_void_p), C.cast(tables["K"], C.c_void_p),
                        C.cast(C.byref(i), C.c_void_p), C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(o), C.c_void_p), vp(accepts))
    return dict(results(S, outs, k, N, int(fused[7][0])), accepts=accepts)


def rotation_angle(Ra, Rb):
    """Angle between two rotations given as 9 or 3 x 3 (refine_reference's: accurate near 0, unlike arccos of the trace)."""
    import refine_reference as RR
    return RR.rotation_angle(np.asarray(Ra, np.float64).reshape(3, 3), np.asarray(Rb, np.float64).reshape(3, 3))


def true_cameras(sc):
    """Camera 2 of every pair of the (uncut) chain, (R, t), in the root pair's gauge: view 0's frame with the baseline of pair 0 as
    the unit.  The scene keeps every pair's own (R, t, baseline) and the links; the pairs' true frames compose along the chain."""
    out = []
    Rw, tw = np.eye(3), np.zeros(3)                              # view i <- view 0, in units of pair 0's baseline
    b0 = sc["pairs"][0]["baseline"]
    for P in sc["pairs"]:
        R, t = np.asarray(P["R"], np.float64).reshape(3, 3), np.asarray(P["t"], np.float64) * P["baseline"] / b0
        Rw, tw = R @ Rw, R @ tw + t
        out.append((Rw.copy(), tw.copy()))
    return out


def strip(k=70, n=65, W=8, seed=3, noise_px=0.5, turn=1e-3, shift=5e-3):
    """ONE segment of k cameras (fuse_scene's six views give five at the most): k + 1 views stepping along a strip of points, one
    unit per view (pair 0's baseline, the gauge), every point seen in 2 .. W consecutive views, n records in every pair.  Built
    directly, not through sfm_fuse_chain, which sfm_adjust_chain does not need: returns (chain, fused, truth) -- chain as
    fuse_scene's (pairs with n, ld, sift, X0, X1 and the fields DeviceChain uploads), fused as fuse_scene.results' dict (root,
    cams, the track table, points, flags, counts), truth the cameras [(R, t)] of views 1 .. k.  The start cameras are the truth
    turned by `turn` rad and moved by `shift` of |t| (at least of one unit), the points the truth moved by 1e-3 of their depth;
    observations carry noise_px of pixel noise, one draw per (point, view)."""
    import cuda_sfm_amd as S
    import align_scene as AS
    import chain_adjust_reference as CR
    rng = np.random.default_rng(seed)
    K, Kinv = AS.camera()
    K64 = K.astype(np.float64)
    # tracks: (head pair, number of pairs); every pair is covered by exactly n of them
    tracks, cover = [], [[] for _ in range(k)]
    for p in range(k):
        while len(cover[p]) < n:
            L = int(min(rng.integers(1, W), k - p))                # pairs: 1 .. W - 1, so 2 .. W views
            tracks.append([p, L])
            for q in range(p, p + L):
                cover[q].append(len(tracks) - 1)
    rec = [dict() for _ in range(k)]                               # pair -> {track: record}
    for p in range(k):
        order = rng.permutation(len(cover[p]))
        for r, i in enumerate(order):
            rec[p][cover[p][i]] = r
    ids = sorted(range(len(tracks)), key=lambda i: (tracks[i][0], rec[tracks[i][0]][i]))       # numbered by head pair, then record
    T = len(ids)
    # cameras: view v at (v, 0, 0) with a small wobble; X_v = R_v (X - c_v)
    views = []
    for v in range(k + 1):
        R = AS.rot_y(np.deg2rad(2.0 * np.sin(0.7 * v))) @ AS.rot_x(np.deg2rad(1.5 * np.cos(0.4 * v))) if v else np.eye(3)
        c = np.array([float(v), 0.05 * np.sin(0.3 * v), 0.1 * np.sin(0.2 * v)]) if v > 1 else np.array([float(v), 0.0, 0.0])
        views.append((R, -R @ c))
    P = np.zeros((T, 3))
    pix = {}
    off, ocam, orec = [0], [], []
    for t, i in enumerate(ids):
        h, L = tracks[i]
        P[t] = [h + 0.5 * L + rng.uniform(-1.5, 1.5), rng.uniform(-2, 2), rng.uniform(20, 40)]
        for v in range(h, h + L + 1):
            Y = K64 @ (views[v][0] @ P[t] + views[v][1])
            pix[(t, v)] = Y[:2] / Y[2] + noise_px * rng.standard_normal(2)
        for q in range(h, h + L):
            ocam.append(2 * q); orec.append(rec[q][i])
        ocam.append(2 * (h + L - 1) + 1); orec.append(rec[h + L - 1][i])
        off.append(len(ocam))
    ld = (n + 127) // 128 * 128
    number = {i: t for t, i in enumerate(ids)}
    track_of = [{r: number[i] for i, r in rec[p].items()} for p in range(k)]
    pairs = []
    for p in range(k):
        sift = np.zeros(n, S.SIFT_DTYPE)
        for r in range(n):
            t = track_of[p][r]
            sift["xpos"][r], sift["ypos"][r] = pix[(t, p)]
            sift["match_xpos"][r], sift["match_ypos"][r] = pix[(t, p + 1)]
        sift["score"], sift["ambiguity"] = 0.95, 0.5
        X0 = AS.normalised(Kinv, sift["xpos"], sift["ypos"], ld)
        X1 = AS.normalised(Kinv, sift["match_xpos"], sift["match_ypos"], ld)
        pairs.append(dict(n=n, ld=ld, sift=sift, X0=X0, X1=X1, points=np.ones((4, n), np.float32), valid=np.ones(n, np.uint8),
                          pose=np.concatenate([np.eye(3).ravel(), [1.0, 0.0, 0.0]]).astype(np.float32)))
    cams = np.zeros((k, 2, 12), np.float32)
    start = []
    for v in range(k + 1):
        R, t = views[v]
        if v:
            w = rng.normal(0, 1, 3); w *= turn / np.linalg.norm(w)
            d = rng.normal(0, 1, 3); d *= shift * max(np.linalg.norm(t), 1.0) / np.linalg.norm(d)
            R, t = CR.expso3(w) @ R, t + d
        start.append(np.concatenate([R.ravel(), t]))
    for p in range(k):
        cams[p, 0], cams[p, 1] = start[p], start[p + 1]
    pts = np.ones((4, T), np.float32)
    pts[:3] = (P * (1.0 + 1e-3 * rng.standard_normal((T, 1)))).T
    longest = int(np.diff(off).max())
    fused = dict(root=np.zeros(k, np.int32), cams=cams, track_offset=np.array(off, np.int32), obs_cam=np.array(ocam, np.int32),
                 obs_record=np.array(orec, np.int32), points=pts, flags=np.ones(T, np.uint8), err=np.zeros(T, np.float32),
                 counts=dict(tracks=T, observations=len(ocam), refined=T, kept=0, segments=1, longest_track=longest))
    return dict(K=K, Kinv=Kinv, pairs=pairs, links=[]), fused, views[1:]
