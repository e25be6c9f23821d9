"""Inputs of the sfm_close_ring tests (helper, not a test): k views on a circle around a point cloud, all looking at its centre,
every pair (v, v + 1 mod k) reconstructed in its own gauge as align_scene does (camera 1 = [I|0], |t| = 1, points triangulated from
observations with pixel noise, wrong view-2 matches in a given share of the records), the k TRUE links of the ring -- link k - 1
carries pair k - 1 into pair 0 -- and the wrapper around the host build (tests/hostcheck/libringcheck.so).

Every view sees every point and keeps its records in an order of its own.  The views stand at uneven angles and radii, so the
baselines b_v, and with them the gauges, differ from pair to pair.  With X_{v+1} = Rrel_v X_v + trel_v and b_v = |trel_v|, pair v's
points are X_v / b_v and link v is s = b_v / b_{v+1}, R = Rrel_v, t = trel_v / b_{v+1} (align_scene's convention): the true links
compose to the identity.  Only the pairs asked for are built: the call itself reads the k links and pair k - 1."""
import ctypes as C
import os

import numpy as np

import align_scene as AS

ROOT = AS.ROOT
RADIUS = 8.0


def sim13(s, R, t):
    return np.concatenate([[s], np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()]).astype(np.float32)


def unpack(v):
    v = np.asarray(v, np.float64).ravel()
    return v[0], v[1:10].reshape(3, 3), v[10:13]


def compose(A, B):
    """A o B of two similarities (s, R, t): B first."""
    return A[0] * B[0], A[1] @ B[1], A[0] * (A[1] @ B[2]) + A[2]


def invert(A):
    return 1.0 / A[0], A[1].T, -(A[1].T @ A[2]) / A[0]


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th ** 2 * (W @ W)


def look_at(Cw):
    """World-to-camera rotation of a camera at Cw that looks at the origin, y down."""
    z = -Cw / np.linalg.norm(Cw)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])


def build(k, n, seed, pairs="last", noise_px=0.5, wrong_match=0.15, wrong_index=0.05, cone_deg=None):
    """The ring of k views / k pairs / k links over n points.  pairs: "last" (pair k - 1 only), "all", or a list of pair numbers.
    Returns a dict: K, Kinv, k, n, P (the points, world frame), R / C (the views), baseline (k), true (k links as (s, R, t)), sims
    (k x 13 float32: the true links), inliers (k, what the links' reports say), perm / inv (the views' record orders), index (per
    link, int32 n), and pairs: {v: align_scene's pair dict + pose}.  cone_deg: the views stand on a circle IN FRONT of the cloud
    instead, on a cone of that half-angle about the z axis, 6 away: neighbours a few degrees and one baseline apart, the two-view
    geometry of align_scene, which estimateE and the refinement are tested on."""
    import cuda_sfm_amd as S
    rng = np.random.default_rng(seed)
    K, Kinv = AS.camera()
    K64 = K.astype(np.float64)
    P = rng.uniform(-0.8, 0.8, (n, 3))
    phi = 2.0 * np.pi * (np.arange(k) + rng.uniform(-0.2, 0.2, k)) / k
    rad = RADIUS * (1.0 + rng.uniform(-0.1, 0.1, k))
    Cw = np.stack([rad * np.sin(phi), rng.uniform(-0.5, 0.5, k), -rad * np.cos(phi)], 1)
    if cone_deg is not None:
        c = np.deg2rad(cone_deg)
        Cw = 0.75 * np.stack([rad * np.sin(c) * np.cos(phi), rad * np.sin(c) * np.sin(phi), -rad * np.cos(c) * np.ones(k)], 1)
        P = P * np.array([1.25, 1.25, 2.5])                                    # align_scene's cloud: +-1 across, depths 4 .. 8
    Rw = [look_at(c) for c in Cw]
    rel, base = [], np.empty(k)
    for v in range(k):
        w = (v + 1) % k
        R = Rw[w] @ Rw[v].T
        t = Rw[w] @ (Cw[v] - Cw[w])
        rel.append((R, t)); base[v] = np.linalg.norm(t)
    true = [(base[v] / base[(v + 1) % k], rel[v][0], rel[v][1] / base[(v + 1) % k]) for v in range(k)]
    perm = {}
    which = [k - 1] if pairs == "last" else (list(range(k)) if pairs == "all" else list(pairs))
    need = sorted({v for p in which for v in (p, (p + 1) % k)})
    uv = {}
    for v in need:
        prng = np.random.default_rng([seed, v])
        perm[v] = np.arange(n) if v == 0 else prng.permutation(n)
        q = (P - Cw[v]) @ Rw[v].T @ K64.T
        uv[v] = q[:, :2] / q[:, 2:] + noise_px * prng.standard_normal((n, 2))
    inv = {v: np.argsort(p) for v, p in perm.items()}
    ld = (n + 127) // 128 * 128
    built, index = {}, {}
    for v in which:
        w = (v + 1) % k
        prng = np.random.default_rng([seed, v, 1])
        R, t = rel[v]
        u1, u2 = uv[v][perm[v]], uv[w][perm[v]]
        bad = prng.random(n) < wrong_match
        u2 = np.where(bad[:, None], prng.random((n, 2)) * [AS.WIDTH, AS.HEIGHT], u2)
        sift = np.zeros(n, S.SIFT_DTYPE)
        sift["xpos"], sift["ypos"] = u1[:, 0].astype(np.float32), u1[:, 1].astype(np.float32)
        sift["match_xpos"], sift["match_ypos"] = u2[:, 0].astype(np.float32), u2[:, 1].astype(np.float32)
        sift["match"] = inv[w][perm[v]].astype(np.int32)
        sift["score"], sift["ambiguity"] = 0.95, 0.5
        X0 = AS.normalised(Kinv, sift["xpos"], sift["ypos"], ld)
        X1 = AS.normalised(Kinv, sift["match_xpos"], sift["match_ypos"], ld)
        X, front = AS.triangulate(X0[:2, :n].T.astype(np.float64), X1[:2, :n].T.astype(np.float64), R, t / base[v])
        pts = np.ascontiguousarray(np.vstack([X.T, np.ones(n)]).astype(np.float32))
        built[v] = dict(n=n, ld=ld, sift=sift, X0=X0, X1=X1, points=pts, valid=front.astype(np.uint8), good=~bad, R=R, t=t / base[v],
                        baseline=base[v], pose=np.concatenate([R.ravel(), t / base[v]]).astype(np.float32))
        idx = inv[w][perm[v]].astype(np.int32)
        wrong = prng.random(n) < wrong_index
        index[v] = np.where(wrong, prng.integers(0, n, n), idx).astype(np.int32)
    return dict(K=K, Kinv=Kinv, k=k, n=n, P=P, R=Rw, C=Cw, baseline=base, true=true, sims=np.stack([sim13(*L) for L in true]),
                inliers=rng.integers(max(n // 2, 1), n + 1, k).astype(np.int32), perm=perm, inv=inv, index=index, pairs=built)


def small_similarities(k, seed, rot=2e-3, scale=0.01, trans=0.01):
    """k small similarities (s, R, t): rotations of `rot` rad about random axes, ln s uniform in +-scale, |t| = trans."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        a = rng.standard_normal(3); a *= rot / np.linalg.norm(a)
        t = rng.standard_normal(3); t *= trans / np.linalg.norm(t)
        out.append((float(np.exp(rng.uniform(-scale, scale))), rodrigues(a), t))
    return out


def perturbed(sims, deltas):
    """The links (k x 13) with link i replaced by deltas[i] o link i (None: unchanged), as float32."""
    out = np.array(sims, np.float32, copy=True)
    for i, d in enumerate(deltas):
        if d is not None:
            out[i] = sim13(*compose(d, unpack(sims[i])))
    return out


def true_centres(sc):
    """The views' centres in pair 0's gauge (k x 3): view 0's frame divided by pair 0's baseline."""
    return (sc["C"] - sc["C"][0]) @ sc["R"][0].T / sc["baseline"][0]


def host_lib():
    path = os.path.join(ROOT, "tests", "hostcheck", "libringcheck.so")
    assert os.path.exists(path), f"{path} is missing: make hostcheck builds it"
    h = C.CDLL(path)
    h.ring_run.restype = None
    h.ring_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9
    h.ring_log.restype = C.c_double
    h.ring_log.argtypes = [C.c_void_p, C.c_void_p]
    h.ring_exp.restype = None
    h.ring_exp.argtypes = [C.c_void_p, C.c_void_p]
    h.ring_blocks.argtypes = [C.c_int]
    h.ring_layout.argtypes = [C.c_int, C.c_void_p]
    return h


def ring_input(sc, sims=None, status=None, inliers=None, last=None):
    """What one call reads: sims (k x 13 float32), status, inliers (k), last (pair k - 1: n, ld, points, valid, X1), K."""
    k = sc["k"]
    return dict(k=k, K=sc["K"], sims=np.ascontiguousarray(sc["sims"] if sims is None else sims, np.float32).reshape(k, 13),
                status=np.zeros(k, np.int32) if status is None else np.ascontiguousarray(status, np.int32),
                inliers=np.ascontiguousarray(sc["inliers"] if inliers is None else inliers, np.int32),
                last=sc["pairs"][k - 1] if last is None else last)


def run_host(HL, S, inp, **kw):
    """The host build over ring_input's dict with RingParams fields kw: (links (k, 13), frames (k, 13), seam errors (3, n),
    report dict), as cuda_sfm_amd.close_ring returns them."""
    p = S.ring_params(**kw)
    k, L = inp["k"], inp["last"]
    n = L["n"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    keep = [f32(inp["sims"]), inp["status"], inp["inliers"], f32(L["points"]),
            None if L.get("valid") is None else np.ascontiguousarray(L["valid"], np.uint8), f32(L["X1"]), f32(inp["K"])]
    links, frames, seam = np.zeros((k, 13), np.float32), np.zeros((k, 13), np.float32), np.zeros((3, n), np.float32)
    rep = S.RingReport()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    HL.ring_run(k, vp(keep[0]), vp(keep[1]), vp(keep[2]), n, L["ld"], vp(keep[3]), vp(keep[4]), vp(keep[5]), vp(keep[6]),
                C.cast(C.byref(p), C.c_void_p), vp(links), vp(frames), vp(seam), C.cast(C.byref(rep), C.c_void_p))
    return links, frames, seam, {f: getattr(rep, f) for f, _ in S.RingReport._fields_}
