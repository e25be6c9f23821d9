"""numpy fp64 twin of sfm_adjust_view (cuda-sfm_amd/csrc/adjust.hip, adjust_math.hpp), written independently of the header (test
helper, not a test): the same used-set rule, the same parameterisation (camera 2: R <- exp([w]x) R, t on the unit sphere through
the tangent basis; camera 3: R3 <- exp([w]x) R3, t3 <- t3 + dt; camera 1 fixed), the same Huber rule per view and the same LM
control.  Every point's normal equations are formed densely -- H = J^T W J with J = [d r / d cameras (6 x 11) | d r / d X (6 x 3)]
-- and the reduced camera system is the Schur complement of the damped point blocks."""
import numpy as np

import refine_reference as RR

CONVERGED, MAX_ITER, DEGENERATE = RR.CONVERGED, RR.MAX_ITER, RR.DEGENERATE
UNSEEN, NEW, REFINED, NEW_REJECTED, KEPT = range(5)
DEFAULTS = dict(max_iterations=20, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3)
MIN_VIEW2, MIN_VIEW3 = 16, 6


def observations(Kinv, rec, X0, X1):
    """n x 6: views 1 and 2 from the pair's normalised X0 / X1 (3 x >= n), view 3 as K^-1 (match_xpos, match_ypos, 1)."""
    n = len(rec)
    X0 = np.asarray(X0, np.float64)[:, :n]; X1 = np.asarray(X1, np.float64)[:, :n]
    u3 = np.asarray(Kinv, np.float64) @ np.stack([rec["match_xpos"].astype(np.float64), rec["match_ypos"].astype(np.float64), np.ones(n)])
    with np.errstate(all="ignore"):
        return np.stack([X0[0] / X0[2], X0[1] / X0[2], X1[0] / X1[2], X1[1] / X1[2], u3[0] / u3[2], u3[1] / u3[2]], 1)


def view_bits(flags, used2, points, P2, P3):
    """uint8[n]: bit 0 / 1 / 2 = views 1 / 2 / 3, 0 = the record is not used.  points 4 x n; P2, P3: (R, t)."""
    flags = np.asarray(flags); pts = np.asarray(points, np.float64)
    see3 = (flags == NEW) | (flags == REFINED)
    see2 = np.asarray(used2).astype(bool) & ((flags == UNSEEN) | (flags == REFINED) | (flags == KEPT))
    with np.errstate(all="ignore"):
        ok = (see2 | see3) & np.isfinite(pts).all(0) & (pts[3] != 0) & (pts[2] / pts[3] > 0)
        X = (pts[:3] / pts[3]).T
        z2 = (X @ np.asarray(P2[0], np.float64).T + P2[1])[:, 2]
        z3 = (X @ np.asarray(P3[0], np.float64).T + P3[1])[:, 2]
        ok &= ~(see2 & ~(z2 > 0)) & ~(see3 & ~(z3 > 0))
    return np.where(ok, 1 + 2 * see2 + 4 * see3, 0).astype(np.uint8)


def _residuals(cam, R2, t2, R3, t3, X, obs, bits):
    """(m, 6) pixel residuals, zero for a view that does not see the point; the depths (m, 3)."""
    Y2 = X @ R2.T + t2; Y3 = X @ R3.T + t3
    with np.errstate(all="ignore"):
        r = np.concatenate([RR._view(cam, X, obs[:, 0:2])[0], RR._view(cam, Y2, obs[:, 2:4])[0], RR._view(cam, Y3, obs[:, 4:6])[0]], 1)
    see = np.repeat(np.stack([bits & 1, bits & 2, bits & 4], 1) != 0, 2, axis=1)
    return np.where(see, r, 0.0), np.stack([X[:, 2], Y2[:, 2], Y3[:, 2]], 1)


def _weights(r, bits, h):
    w = np.zeros((len(r), 3)); rho = np.zeros((len(r), 3))
    for v in range(3):
        wv, rv = RR.huber(r[:, 2 * v:2 * v + 2], h)
        see = (bits & (1 << v)) != 0
        w[:, v] = np.where(see, wv, 0.0); rho[:, v] = np.where(see, rv, 0.0)
    return w, rho


def cost_of(cam, R2, t2, R3, t3, X, obs, bits, h):
    r, _ = _residuals(cam, R2, t2, R3, t3, X, obs, bits)
    _, rho = _weights(r, bits, h)
    return float(rho.sum()), float((r ** 2).sum())


def jacobians(cam, R2, t2, R3, t3, X, obs, bits):
    """r (m, 6) and the dense Jacobian (m, 6, 14): columns 0..4 camera 2 (omega, dt in the tangent basis at t2), 5..10 camera 3
    (omega, dt), 11..13 the point.  Rows of a view that does not see the point are zero."""
    m = len(X)
    b1, b2 = RR.tangent_basis(t2)
    q2 = X @ R2.T; q3 = X @ R3.T
    r, _ = _residuals(cam, R2, t2, R3, t3, X, obs, bits)
    with np.errstate(all="ignore"):
        J1 = RR._view(cam, X, obs[:, 0:2])[1]
        J2 = RR._view(cam, q2 + t2, obs[:, 2:4])[1]
        J3 = RR._view(cam, q3 + t3, obs[:, 4:6])[1]
    J = np.zeros((m, 6, 14))
    J[:, 0:2, 11:14] = J1
    J[:, 2:4, 11:14] = J2 @ R2
    J[:, 4:6, 11:14] = J3 @ R3
    J[:, 2:4, 0:3] = np.cross(q2[:, None, :], J2)             # d Y / d omega = -[q]x: row j times it is q x j
    J[:, 2:4, 3] = J2 @ b1; J[:, 2:4, 4] = J2 @ b2
    J[:, 4:6, 5:8] = np.cross(q3[:, None, :], J3)
    J[:, 4:6, 8:11] = J3
    see = np.repeat(np.stack([bits & 1, bits & 2, bits & 4], 1) != 0, 2, axis=1)
    return r, np.where(see[:, :, None], J, 0.0)


def system(cam, R2, t2, R3, t3, X, obs, bits, h, lam):
    """Per-point dense normal equations and their Schur complement on the 11 camera parameters at damping lam."""
    r, J = jacobians(cam, R2, t2, R3, t3, X, obs, bits)
    w, _ = _weights(r, bits, h)
    W6 = np.repeat(w, 2, axis=1)
    H = np.einsum("mai,ma,maj->mij", J, W6, J)                # (m, 14, 14)
    g = np.einsum("mai,ma,ma->mi", J, W6, r)
    U, Wm, V = H[:, :11, :11], H[:, :11, 11:], H[:, 11:, 11:].copy()
    i3 = np.arange(3)
    V[:, i3, i3] *= 1.0 + lam
    Vi = np.linalg.inv(V)
    T = Wm @ Vi
    S = U - T @ Wm.transpose(0, 2, 1)
    b = g[:, :11] - np.einsum("mij,mj->mi", T, g[:, 11:])
    return dict(S=S.sum(0), b=b.sum(0), dU=np.einsum("mii->i", U), Vi=Vi, Wm=Wm, gp=g[:, 11:], S_pt=S, b_pt=b, U_pt=U, w=w)


def adjust(cam, R2, t2, R3, t3, X0, obs, bits, max_iterations=20, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3):
    """LM from the start over the used points X0 (m, 3), obs (m, 6), bits (m).  Returns a dict like the report plus R2, t2, R3, t3, X."""
    cam = tuple(float(c) for c in cam)
    R2, t2, R3, t3 = (np.asarray(a, np.float64).copy() for a in (R2, t2, R3, t3))
    X = np.asarray(X0, np.float64).copy(); obs = np.asarray(obs, np.float64); bits = np.asarray(bits).astype(int)
    m = len(X); n2 = int(((bits & 2) != 0).sum()); n3 = int(((bits & 4) != 0).sum())
    terms = 2.0 * (m + n2 + n3)
    h = float(huber_px)
    cost, sq = cost_of(cam, R2, t2, R3, t3, X, obs, bits, h) if m else (0.0, 0.0)
    rep = dict(num_points=m, num_view2=n2, num_view3=n3, initial_rms_px=np.sqrt(sq / terms) if m else 0.0)
    lam = float(np.float32(initial_lambda))
    iters = accepted = 0
    status = DEGENERATE if (n2 < MIN_VIEW2 or n3 < MIN_VIEW3) else MAX_ITER
    while status != DEGENERATE and iters < max_iterations:
        b1, b2 = RR.tangent_basis(t2)
        sy = system(cam, R2, t2, R3, t3, X, obs, bits, h, lam)
        S = sy["S"] + lam * np.diag(sy["dU"])
        iters += 1
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            lam *= 10.0
            if lam > 1e16:
                break
            continue
        dc = -np.linalg.solve(L.T, np.linalg.solve(L, sy["b"]))
        R2t = RR.expso3(dc[:3]) @ R2
        t2t = t2 + b1 * dc[3] + b2 * dc[4]; t2t /= np.linalg.norm(t2t)
        R3t = RR.expso3(dc[5:8]) @ R3
        t3t = t3 + dc[8:11]
        dp = -np.einsum("mij,mj->mi", sy["Vi"], sy["gp"] + np.einsum("mip,i->mp", sy["Wm"], dc))
        Xt = X + dp
        nc, nsq = cost_of(cam, R2t, t2t, R3t, t3t, Xt, obs, bits, h)
        if nc < cost:
            rel = (cost - nc) / cost
            cost, sq = nc, nsq
            R2, t2, R3, t3, X = R2t, t2t, R3t, t3t, Xt
            accepted += 1
            lam /= 10.0
            if not rel >= min_rel_decrease:
                status = CONVERGED
                break
        else:
            lam *= 10.0
            if lam > 1e16:
                break
    rep.update(status=status, iterations=iters, accepted=accepted, final_rms_px=np.sqrt(sq / terms) if m else 0.0, final_cost=cost,
               **{"lambda": lam}, R2=R2, t2=t2, R3=R3, t3=t3, X=X)
    return rep


def pixel_error(cam, R2, t2, R3, t3, X, obs, bits):
    """The largest pixel error over each point's views, +inf where a view that sees it has it behind the camera."""
    r, z = _residuals(cam, R2, t2, R3, t3, X, obs, bits)
    e = np.sqrt(np.stack([(r[:, 0:2] ** 2).sum(1), (r[:, 2:4] ** 2).sum(1), (r[:, 4:6] ** 2).sum(1)], 1)).max(1)
    see = np.stack([bits & 1, bits & 2, bits & 4], 1) != 0
    return np.where((~see | (z > 0)).all(1), e, np.inf)


def run(K, Kinv, rec, X0, X1, points, flags, used2, poses, **kw):
    """The whole call: poses float[24] ([R|t] of cameras 2 and 3).  Returns poses (24), points (4 x n), views, err, report dict
    (with the twin's R2, t2, R3, t3, X and the used indices idx)."""
    p = dict(DEFAULTS); p.update(kw)
    K = np.asarray(K, np.float64)
    cam = (K[0, 0], K[0, 1], K[1, 1])
    poses = np.asarray(poses, np.float64)
    R2, t2, R3, t3 = poses[:9].reshape(3, 3), poses[9:12], poses[12:21].reshape(3, 3), poses[21:24]
    pts = np.asarray(points, np.float64)
    n = pts.shape[1]
    views = view_bits(flags, used2, pts, (R2, t2), (R3, t3))
    obs = observations(Kinv, rec, X0, X1)
    idx = np.flatnonzero(views)
    with np.errstate(all="ignore"):
        Xs = (pts[:3, idx] / pts[3, idx]).T
    rep = adjust(cam, R2, t2, R3, t3, Xs, obs[idx], views[idx], **p)
    out = pts.copy()
    err = np.full(n, np.inf)
    if rep["status"] != DEGENERATE:
        out[:3, idx] = rep["X"].T; out[3, idx] = 1.0
    if len(idx):
        err[idx] = pixel_error(cam, rep["R2"], rep["t2"], rep["R3"], rep["t3"], rep["X"], obs[idx], views[idx].astype(int))
    rep["idx"] = idx
    return np.concatenate([rep["R2"].ravel(), rep["t2"], rep["R3"].ravel(), rep["t3"]]), out, views, err, rep
