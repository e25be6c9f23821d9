"""fp64 numpy twin of sfm_triangulate_view (cuda-sfm_amd/csrc/view_points_math.hpp), written independently of it: the DLT by
numpy's SVD, the point Levenberg-Marquardt with the same damping / accept / stop rules (LmControl), the same acceptance test
stated on the pixel error.  Vectorised over the points; every point keeps its own LM state."""
import numpy as np

UNSEEN, NEW, REFINED, NEW_REJECTED, KEPT = range(5)
DEFAULTS = dict(threshold_px=4.0, min_score=0.85, max_ambiguity=0.95, min_parallax_deg=1.0, max_iterations=5, huber_px=1.0,
                min_rel_decrease=1e-6, initial_lambda=1e-3)


def _views(P2, P3, use2):
    """The cameras a point is refined over: (R, t, column of obs) -- camera 1, camera 2 where use2, camera 3."""
    I = (np.eye(3), np.zeros(3), 0)
    return [I] + ([(np.asarray(P2[0], np.float64), np.asarray(P2[1], np.float64), 2)] if use2 else []) + \
        [(np.asarray(P3[0], np.float64), np.asarray(P3[1], np.float64), 4)]


def _residual(K, R, t, X, xy):
    """Pixel residual (m x 2), its Jacobian by X (m x 2 x 3) and the depth of the points X (m x 3) in camera [R|t]."""
    Y = X @ R.T + t
    with np.errstate(all="ignore"):
        iz = 1.0 / Y[:, 2]
        px, py = Y[:, 0] * iz, Y[:, 1] * iz
        ex, ey = px - xy[:, 0], py - xy[:, 1]
        r = np.stack([K[0, 0] * ex + K[0, 1] * ey, K[1, 1] * ey], 1)
        Z = np.zeros_like(iz)
        dpi = np.stack([np.stack([iz, Z, -px * iz], 1), np.stack([Z, iz, -py * iz], 1)], 1)       # m x 2 x 3
        J = np.einsum("ab,mbc,cd->mad", K[:2, :2].astype(np.float64), dpi, R)
    return r, J, Y[:, 2]


def _huber(r, h):
    with np.errstate(all="ignore"):
        e2 = (r * r).sum(1)
        e = np.sqrt(e2)
        big = (h > 0) & (e2 > h * h)
        rho = np.where(big, 2 * h * e - h * h, e2)
        w = np.where(big, h / np.where(e > 0, e, 1.0), 1.0)
    return w, rho


def huber_cost(K, P2, P3, use2, obs, X, h):
    """Robust cost of the points X (m x 3) over their views; obs m x 6."""
    c = np.zeros(len(X))
    for R, t, col in _views(P2, P3, use2):
        r, _, _ = _residual(K, R, t, X, obs[:, col:col + 2])
        c = c + _huber(r, h)[1]
    return c


def point_lm(K, P2, P3, use2, obs, X0, max_iterations, huber_px, min_rel_decrease, initial_lambda):
    """The point LM on every row of X0 at once."""
    X = np.array(X0, np.float64)
    m = len(X)
    lam = np.full(m, float(initial_lambda))
    cost = huber_cost(K, P2, P3, use2, obs, X, huber_px)
    iters = np.zeros(m, int)
    run = np.ones(m, bool)
    for _ in range(int(max_iterations)):
        run &= iters < max_iterations
        if not run.any():
            break
        V = np.zeros((m, 3, 3)); g = np.zeros((m, 3))
        for R, t, col in _views(P2, P3, use2):
            r, J, _ = _residual(K, R, t, X, obs[:, col:col + 2])
            w, _ = _huber(r, huber_px)
            V += w[:, None, None] * np.einsum("mka,mkb->mab", J, J)
            g += w[:, None] * np.einsum("mka,mk->ma", J, r)
        D = V + lam[:, None, None] * V * np.eye(3)
        with np.errstate(all="ignore"):
            ok = np.isfinite(D).all((1, 2)) & np.isfinite(g).all(1)
            ok[ok] &= np.abs(np.linalg.det(D[ok])) > 0
            step = np.zeros((m, 3))
            step[ok] = -np.linalg.solve(D[ok], g[ok][:, :, None])[:, :, 0]
            Xt = X + step
            ok &= np.isfinite(Xt).all(1)
            nc = huber_cost(K, P2, P3, use2, obs, np.where(ok[:, None], Xt, X), huber_px)
        iters[run] += 1
        better = run & ok & (nc < cost)
        with np.errstate(all="ignore"):
            rel = np.where(better, (cost - nc) / np.where(cost > 0, cost, 1.0), 0.0)
        X[better] = Xt[better]
        cost[better] = nc[better]
        lam[better] /= 10.0
        worse = run & ~better
        lam[worse] *= 10.0
        run &= ~(better & ~(rel >= min_rel_decrease)) & ~(worse & (lam > 1e16))
    return X


def pixel_errors(K, P2, P3, use2, obs, X):
    """Per view: pixel error (inf behind the camera or where it is not finite); m x views."""
    out = []
    for R, t, col in _views(P2, P3, use2):
        r, _, z = _residual(K, R, t, X, obs[:, col:col + 2])
        with np.errstate(all="ignore"):
            e = np.sqrt((r * r).sum(1))
        out.append(np.where((z > 0) & np.isfinite(e), e, np.inf))
    return np.stack(out, 1)


def parallax_deg(X, P3):
    """Angle at X between the rays to the centres of cameras 1 and 3."""
    R3, t3 = np.asarray(P3[0], np.float64), np.asarray(P3[1], np.float64)
    b = X + R3.T @ t3
    with np.errstate(all="ignore"):
        c = (X * b).sum(1) / np.sqrt((X * X).sum(1) * (b * b).sum(1))
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def dlt13(obs, P3):
    """SVD DLT of views 1 and 3 for every row of obs: X (m x 3, nan where w == 0)."""
    R3, t3 = np.asarray(P3[0], np.float64), np.asarray(P3[1], np.float64)
    M1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    M3 = np.hstack([R3, t3[:, None]])
    A = np.stack([obs[:, 0, None] * M1[2] - M1[0], obs[:, 1, None] * M1[2] - M1[1],
                  obs[:, 4, None] * M3[2] - M3[0], obs[:, 5, None] * M3[2] - M3[1]], 1)
    v = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(all="ignore"):
        return v[:, :3] / v[:, 3:]


def view_points(K, Kinv, rec, X0, X1, points, valid, P2, P3, **kw):
    """rec: view 1's records re-matched against view 3; X0, X1: 3 x (>= n) normalised observations; points: 4 x n; valid: n or
    None; P2, P3: (R 3x3, t 3).  Returns a dict: flags, points (4 x n), err, and for the band tests seen, usable, X (the point
    that was attempted, n x 3, nan where none), start (n x 3), parallax (degrees, nan unless a new point), obs (n x 6)."""
    p = dict(DEFAULTS); p.update(kw)
    K = np.asarray(K, np.float64); Kinv = np.asarray(Kinv, np.float64)
    n = len(rec)
    pts = np.asarray(points, np.float64)
    seen = (rec["match"] >= 0) & (rec["score"] > np.float32(p["min_score"])) & (rec["ambiguity"] < np.float32(p["max_ambiguity"]))
    with np.errstate(all="ignore"):
        usable = np.isfinite(pts).all(0) & (pts[3] != 0) & (pts[2] / pts[3] > 0)
    if valid is not None:
        usable &= np.asarray(valid).astype(bool)
    X0 = np.asarray(X0, np.float64)[:, :n]; X1 = np.asarray(X1, np.float64)[:, :n]
    u3 = Kinv @ np.stack([rec["match_xpos"].astype(np.float64), rec["match_ypos"].astype(np.float64), np.ones(n)])
    with np.errstate(all="ignore"):
        obs = np.stack([X0[0] / X0[2], X0[1] / X0[2], X1[0] / X1[2], X1[1] / X1[2], u3[0] / u3[2], u3[1] / u3[2]], 1)
    flags = np.zeros(n, np.uint8)
    out = pts.copy()
    err = np.full(n, np.inf)
    Xall = np.full((n, 3), np.nan); start = np.full((n, 3), np.nan); par = np.full(n, np.nan)
    lm = (p["max_iterations"], p["huber_px"], p["min_rel_decrease"], p["initial_lambda"])
    for use2 in (False, True):
        idx = np.flatnonzero(seen & (usable == use2))
        if not len(idx):
            continue
        o = obs[idx]
        with np.errstate(all="ignore"):
            S = (pts[:3, idx] / pts[3, idx]).T if use2 else dlt13(o, P3)
        good = np.isfinite(S).all(1)
        X = np.full((len(idx), 3), np.nan)
        if good.any():
            X[good] = point_lm(K, P2, P3, use2, o[good], S[good], *lm)
        e = np.full(len(idx), np.inf)
        if good.any():
            e[good] = pixel_errors(K, P2, P3, use2, o[good], X[good]).max(1)
        acc = good & (e < p["threshold_px"])
        if not use2:
            a = np.full(len(idx), np.nan)
            a[good] = parallax_deg(X[good], P3)
            par[idx] = a
            with np.errstate(all="ignore"):
                acc &= a >= p["min_parallax_deg"]
        flags[idx] = np.where(acc, REFINED if use2 else NEW, KEPT if use2 else NEW_REJECTED)
        out[:3, idx[acc]] = X[acc].T
        out[3, idx[acc]] = 1.0
        err[idx] = e
        Xall[idx] = X; start[idx] = S
    return {"flags": flags, "points": out, "err": err, "seen": seen, "usable": usable, "X": Xall, "start": start, "parallax": par, "obs": obs}
