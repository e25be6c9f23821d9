"""The fp64 twin of sfm_close_ring (helper, not a test): numpy float64 throughout, nothing rounded to float32 but the inputs it is
given.  It follows the call's model and not its code: matrices and vectors, numpy's own order of every sum."""
import numpy as np

CLOSED, OPEN, REJECTED = 0, 1, 2
DEGENERATE = 2                                        # SFM_REFINE_DEGENERATE


def unpack(v):
    v = np.asarray(v, np.float64).ravel()
    return v[0], v[1:10].reshape(3, 3), v[10:13]


def pack(S):
    return np.concatenate([[S[0]], np.asarray(S[1]).ravel(), np.asarray(S[2]).ravel()])


def compose(A, B):
    return A[0] * B[0], A[1] @ B[1], A[0] * (A[1] @ B[2]) + A[2]


def invert(A):
    return 1.0 / A[0], A[1].T, -(A[1].T @ A[2]) / A[0]


IDENTITY = (1.0, np.eye(3), np.zeros(3))


def link_valid(status, sim):
    sim = np.asarray(sim)
    return bool(status != DEGENERATE and np.isfinite(sim).all() and sim[0] > 0)


def rot_log(R):
    """Axis-angle from the antisymmetric part: atan2(|v|, (tr - 1) / 2)."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    nv = np.linalg.norm(v)
    angle = np.arctan2(nv, 0.5 * (np.trace(R) - 1.0))
    return (v * (angle / nv) if nv > 0 else v), float(angle)


def rot_exp(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0.0:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + 2.0 * np.sin(0.5 * th) ** 2 / th ** 2 * (W @ W)


def walk(sims, status):
    """F_0 .. F_k (an invalid link restarts at the identity) and the first invalid link (-1: none)."""
    F, first = [IDENTITY], -1
    for i, sim in enumerate(sims):
        if link_valid(status[i], sim):
            F.append(compose(F[-1], invert(unpack(sim))))
        else:
            F.append(IDENTITY)
            first = i if first < 0 else first
    return F, first


def alphas(weights):
    w = np.asarray(weights, np.float64)
    a = np.concatenate([[0.0], np.cumsum(w / w.sum())])
    a[-1] = 1.0
    return a


def pixel_errors(K, F, points, valid, X1, n, thr):
    """Per record of the last pair: usable, the pixel error of its point carried by F against its X1 observation under [I|0]
    (inf: not usable or behind the camera), and the inlier test."""
    K = np.asarray(K, np.float64)
    Pt = np.asarray(points, np.float64)[:, :n]
    with np.errstate(all="ignore"):
        usable = (np.ones(n, bool) if valid is None else np.asarray(valid)[:n] != 0) & np.isfinite(Pt).all(0) & (Pt[3] != 0) & (Pt[2] / Pt[3] > 0)
        X = Pt[:3] / Pt[3]
        Y = F[0] * (F[1] @ X) + F[2][:, None]
        x1 = np.asarray(X1, np.float64)[:, :n]
        ex, ey = Y[0] / Y[2] - x1[0] / x1[2], Y[1] / Y[2] - x1[1] / x1[2]
        e = np.hypot(K[0, 0] * ex + K[0, 1] * ey, K[1, 1] * ey)
        ok = usable & (Y[2] > 0) & np.isfinite(e)
        err = np.where(ok, e, np.inf)
    return usable, err, ok & (err < thr)


def close_ring(inp, threshold_px=4.0, max_rotation_rad=0.35, max_log_scale=float(np.log(2.0)), weights=None):
    """ring_scene.ring_input's dict -> dict(links (k, 13), frames (k, 13), open (k, 13: the open frames), seam (3, n), report)."""
    k, sims, status = inp["k"], np.asarray(inp["sims"], np.float64), inp["status"]
    F, first = walk(sims, status)
    rep = dict(status=OPEN, num_links=k, first_invalid=first, drift_log_scale=0.0, drift_rotation_rad=0.0, drift_t=0.0)
    closed, links = F[:k], [unpack(s) for s in sims]
    if first < 0:
        D = F[k]
        Dinv = invert(D)
        sigma = np.log(Dinv[0])
        w, angle = rot_log(Dinv[1])
        rep.update(drift_log_scale=float(-sigma), drift_rotation_rad=angle, drift_t=float(np.linalg.norm(D[2])))
        ok = angle <= np.float32(max_rotation_rad) and abs(sigma) <= np.float32(max_log_scale)
        rep["status"] = CLOSED if ok else REJECTED
        if ok:
            a = alphas([1.0 / max(int(c), 1) for c in inp["inliers"]] if weights is None else np.asarray(weights, np.float32))
            B = [(np.exp(x * sigma), rot_exp(x * w), x * Dinv[2]) for x in a[:k]] + [Dinv]
            G = [compose(B[i], F[i]) for i in range(k + 1)]
            closed = G[:k]
            links = [compose(invert(G[i + 1]), G[i]) for i in range(k)]
    L = inp["last"]
    n = L["n"]
    three = [unpack(sims[k - 1]), F[k - 1], closed[k - 1]]
    res = [pixel_errors(inp["K"], f, L["points"], L.get("valid"), L["X1"], n, threshold_px) for f in three]
    S = res[0][2]
    seam = np.stack([r[1] for r in res])
    rms = []
    for r in res:
        e = r[1][S & np.isfinite(r[1])]
        rms.append(float(np.sqrt(np.mean(e ** 2))) if len(e) else 0.0)
    rep.update(seam_count=int(S.sum()), seam_lost_open=int((S & ~np.isfinite(res[1][1])).sum()), seam_lost_closed=int((S & ~np.isfinite(res[2][1])).sum()),
               seam_rms_link_px=rms[0], seam_rms_open_px=rms[1], seam_rms_closed_px=rms[2])
    return dict(links=np.stack([pack(x) for x in links]), frames=np.stack([pack(x) for x in closed]), open=np.stack([pack(x) for x in F[:k]]),
                seam=seam, report=rep)
