"""The fp64 twin of sfm_adjust_chain (helper, not a test): the same Levenberg-Marquardt in numpy.

Per segment: the residuals and Jacobians of every used observation, H = J^T W J assembled block by block (cameras dense, points
block diagonal, the camera x point part dense), the damping lambda diag H on both, the Schur complement on the cameras as a dense
matrix and its solve by numpy.linalg (no band, no Cholesky of its own), the back substitution, and LmControl's rules: ten times
the damping after a failed solve or a rejected step, a tenth after an accepted one, accepted when the cost falls, ended after
max_iterations, below min_rel_decrease, or past 1e16.

Inputs are what the host build reads: the chain's pairs (X0, X1, K) and sfm_fuse_chain's results as the dict fuse_scene.results
gives.  The used test, the block indices and the degenerate decisions follow DESIGN 6i."""
import numpy as np

REFINED, MAX_ITER, CONVERGED, DEGENERATE = 1, 1, 0, 2          # SFM_FUSE_REFINED; SFM_REFINE_MAX_ITER / _CONVERGED / _DEGENERATE
MIN_ROOT, MIN_OTHER = 16, 6


def block_of(obs_cam, root):
    """The camera block of an observation: pair q's camera 2 is block q, its camera 1 block q - 1 or the fixed root (-1)."""
    q = obs_cam >> 1
    return q if obs_cam & 1 else (-1 if root[q] == q else q - 1)


def tangent_basis(t):
    k = int(np.argmin(np.abs(t)))                              # the first smallest |t_k|
    e = np.zeros(3); e[k] = 1.0
    b1 = np.cross(t, e); b1 /= np.linalg.norm(b1)
    b2 = np.cross(t, b1); b2 /= np.linalg.norm(b2)
    return b1, b2


def expso3(w):
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def observations(pairs, K, fused):
    """Per observation of the track table: track, pair, block, x, y (float32 columns: float32 division as fuse_view, then float64),
    fx, s, fy."""
    root, T = fused["root"], len(fused["flags"])
    rows = []
    for t in range(T):
        for o in range(fused["track_offset"][t], fused["track_offset"][t + 1]):
            c, rec = int(fused["obs_cam"][o]), int(fused["obs_record"][o])
            P = pairs[c >> 1]
            X = np.asarray(P["X1"] if c & 1 else P["X0"])          # (float64 columns, where a test gives exact ones, stay float64)
            Kp = np.asarray(P.get("K", K), np.float64).reshape(3, 3)
            rows.append((t, c >> 1, block_of(c, root), float(X[0, rec] / X[2, rec]), float(X[1, rec] / X[2, rec]), Kp[0, 0], Kp[0, 1], Kp[1, 1]))
    return np.array(rows, np.float64).reshape(-1, 8)


def start_cameras(fused):
    """R (k, 3, 3), t (k, 3) of every block from slot 2p + 1; a root's t normalised."""
    cams = np.asarray(fused["cams"], np.float64)
    R, t = cams[:, 1, :9].reshape(-1, 3, 3).copy(), cams[:, 1, 9:].copy()
    for p in range(len(R)):
        if fused["root"][p] == p:
            t[p] /= np.linalg.norm(t[p])
    return R, t


def used_tracks(fused, ob, R, t, W):
    """The used flag of every track under the unified start cameras, and the start points X / W."""
    T = len(fused["flags"])
    pts = np.asarray(fused["points"], np.float32)
    used, X = np.zeros(T, bool), np.zeros((T, 3))
    with np.errstate(all="ignore"):
        for tr in range(T):
            rows = ob[ob[:, 0] == tr]
            col = pts[:, tr]
            if fused["flags"][tr] != REFINED or len(rows) > W or not np.isfinite(col).all() or col[3] == 0:
                continue
            x = (col[:3] / col[3]).astype(np.float64)
            if not np.isfinite(x).all():
                continue
            ok = True
            for r in rows:
                b = int(r[2])
                z = x[2] if b < 0 else (R[b] @ x + t[b])[2]
                ok = ok and z > 0
            used[tr], X[tr] = ok, x
    return used, X


def terms(ob, X, R, t, basis, huber, p0):
    """Residuals (m, 2), d r / d X (m, 2, 3), d r / d camera (m, 2, 6), weights, rho of the observations ob at the state."""
    ti, bi = ob[:, 0].astype(int), ob[:, 2].astype(int)
    fixed = bi < 0
    Ro = np.where(fixed[:, None, None], np.eye(3)[None], R[np.maximum(bi, 0)])
    to = np.where(fixed[:, None], 0.0, t[np.maximum(bi, 0)])
    q = np.einsum("mij,mj->mi", Ro, X[ti])
    Y = q + to
    iz = 1.0 / Y[:, 2]
    px, py = Y[:, 0] * iz, Y[:, 1] * iz
    fx, s, fy = ob[:, 5], ob[:, 6], ob[:, 7]
    ex, ey = px - ob[:, 3], py - ob[:, 4]
    r = np.stack([fx * ex + s * ey, fy * ey], 1)
    Jy = np.zeros((len(ob), 2, 3))
    Jy[:, 0, 0] = fx * iz; Jy[:, 0, 1] = s * iz; Jy[:, 0, 2] = -(fx * px + s * py) * iz
    Jy[:, 1, 1] = fy * iz; Jy[:, 1, 2] = -fy * py * iz
    Jp = np.einsum("mri,mij->mrj", Jy, Ro)
    Jc = np.zeros((len(ob), 2, 6))
    Jc[:, :, :3] = np.cross(q[:, None, :], Jy)
    Jc[:, :, 3:] = Jy
    rootb = bi == p0
    Jc[rootb, :, 3:5] = np.einsum("mri,ij->mrj", Jy[rootb], np.stack(basis, 1))
    Jc[rootb, :, 5] = 0.0
    Jc[fixed] = 0.0
    e2 = (r * r).sum(1)
    w, rho = np.ones(len(ob)), e2.copy()
    if huber > 0:
        big = e2 > huber * huber
        e = np.sqrt(e2[big])
        w[big], rho[big] = huber / e, 2 * huber * e - huber * huber
    return r, Jp, Jc, w, rho, Y[:, 2]


def adjust_segment(ob, X, R, t, p0, p1, max_iterations, huber, min_rel, lambda0, degenerate):
    """LM over one segment.  ob: the used observations of the segment; X: (T, 3), the segment's used tracks are moved; R, t: all
    blocks, p0 .. p1 - 1 are moved.  Returns the report dict and the accept sequence."""
    nb = p1 - p0
    tracks = np.unique(ob[:, 0].astype(int))
    slot = {tr: i for i, tr in enumerate(tracks)}
    tl = np.array([slot[int(x)] for x in ob[:, 0]], int)
    bl = ob[:, 2].astype(int) - p0
    cam = bl >= 0
    X, R, t = X.copy(), R.copy(), t.copy()
    basis = tangent_basis(t[p0])

    def cost_of(Xs, Rs, ts, bs):
        r, _, _, _, rho, _ = terms(ob, Xs, Rs, ts, bs, huber, p0)
        return float(rho.sum()), float((r * r).sum())

    cost, sq = cost_of(X, R, t, basis) if len(ob) else (0.0, 0.0)
    rms = lambda v: float(np.sqrt(v / (2 * len(ob)))) if len(ob) else 0.0
    rep = dict(root=p0, status=DEGENERATE if degenerate else MAX_ITER, iterations=0, accepted=0, num_cameras=nb, num_tracks=len(tracks),
               num_observations=len(ob), initial_rms_px=rms(sq))
    lam, seq = float(lambda0), []
    while rep["status"] != DEGENERATE and rep["iterations"] < max_iterations:
        r, Jp, Jc, w, rho, _ = terms(ob, X, R, t, basis, huber, p0)
        U = np.zeros((6 * nb, 6 * nb)); gc = np.zeros(6 * nb)
        Wm = np.zeros((6 * nb, 3 * len(tracks)))
        V = np.zeros((len(tracks), 3, 3)); gp = np.zeros((len(tracks), 3))
        np.add.at(V, tl, w[:, None, None] * np.einsum("mri,mrj->mij", Jp, Jp))
        np.add.at(gp, tl, w[:, None] * np.einsum("mri,mr->mi", Jp, r))
        for m in np.flatnonzero(cam):
            b, c = 6 * bl[m], 3 * tl[m]
            U[b:b + 6, b:b + 6] += w[m] * Jc[m].T @ Jc[m]
            gc[b:b + 6] += w[m] * Jc[m].T @ r[m]
            Wm[b:b + 6, c:c + 3] += w[m] * Jc[m].T @ Jp[m]
        Ud = U + lam * np.diag(np.diag(U))
        Ud[5, 5] = 1.0                                            # the 5-dof block's unit row
        Vd = V + lam * np.einsum("tij,ij->tij", V, np.eye(3))
        rep["iterations"] += 1
        try:
            with np.errstate(all="raise"):
                Vi = np.linalg.inv(Vd)
                WV = np.einsum("ctk,tkj->ctj", Wm.reshape(6 * nb, len(tracks), 3), Vi).reshape(6 * nb, -1)
                S = Ud - WV @ Wm.T
                b = gc - WV @ gp.ravel()
                np.linalg.cholesky(S)                             # positive definite, or the step is a failed solve
                dc = np.linalg.solve(S, -b)
        except (np.linalg.LinAlgError, FloatingPointError):
            seq.append(3)
            lam *= 10.0
            if lam > 1e16:
                break
            continue
        dp = -np.einsum("tij,tj->ti", Vi, gp + (Wm.T @ dc).reshape(-1, 3))
        Xn, Rn, tn = X.copy(), R.copy(), t.copy()
        Xn[tracks] += dp
        for pl in range(nb):
            d = dc[6 * pl:6 * pl + 6]
            Rn[p0 + pl] = expso3(d[:3]) @ R[p0 + pl]
            if pl == 0:
                tt = t[p0] + basis[0] * d[3] + basis[1] * d[4]
                tn[p0] = tt / np.linalg.norm(tt)
            else:
                tn[p0 + pl] = t[p0 + pl] + d[3:]
        nbasis = tangent_basis(tn[p0])
        with np.errstate(all="ignore"):
            nc, nsq = cost_of(Xn, Rn, tn, nbasis)
        if nc < cost:
            rel = (cost - nc) / cost
            cost, sq, X, R, t, basis = nc, nsq, Xn, Rn, tn, nbasis
            rep["accepted"] += 1
            lam /= 10.0
            seq.append(1)
            if not rel >= min_rel:
                rep["status"] = CONVERGED
                break
        else:
            seq.append(2)
            lam *= 10.0
            if lam > 1e16:
                break
    rep.update(final_rms_px=rms(sq), final_cost=cost, lambda_=lam)
    return rep, seq, X, R, t


def adjust_chain(pairs, K, fused, max_iterations=10, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3, max_track_views=8):
    """The whole call.  Returns cams (k, 2, 12) float64, points (4, T), used (T), err (T), reports (a dict per segment root, keyed
    by the root), accepts (the accept sequence per root), blocks (per observation) and blockobs (used observations per block)."""
    root = np.asarray(fused["root"])
    k, T, W = len(root), len(fused["flags"]), max_track_views
    ob = observations(pairs, K, fused)
    R, t = start_cameras(fused)
    used, X = used_tracks(fused, ob, R, t, W)
    lens = np.diff(fused["track_offset"])
    blockobs = np.zeros(k, int)
    uob = ob[used[ob[:, 0].astype(int)]] if len(ob) else ob
    for b in uob[:, 2].astype(int):
        if b >= 0:
            blockobs[b] += 1
    cams_in = np.asarray(fused["cams"], np.float64)
    cams, pts = cams_in.copy(), np.asarray(fused["points"], np.float64).copy()
    reports, accepts = {}, {}
    for p0 in range(k):
        if root[p0] != p0:
            continue
        p1 = p0 + 1
        while p1 < k and root[p1] == p0:
            p1 += 1
        seg = uob[(root[uob[:, 1].astype(int)] == p0)] if len(uob) else uob
        degenerate = blockobs[p0] < MIN_ROOT or bool((blockobs[p0 + 1:p1] < MIN_OTHER).any())
        rep, seq, Xs, Rs, ts = adjust_segment(seg, X, R, t, p0, p1, max_iterations, huber_px, min_rel_decrease, initial_lambda, degenerate)
        heads = fused["obs_cam"][fused["track_offset"][:-1]] >> 1 if T else np.zeros(0, int)
        rep["num_over_long"] = int(((lens > W) & (root[heads] == p0)).sum()) if T else 0
        reports[p0], accepts[p0] = rep, seq
        if not degenerate:
            X, R, t = Xs, Rs, ts
            for p in range(p0, p1):
                cams[p, 1] = np.concatenate([R[p].ravel(), t[p]])
                if p > p0:
                    cams[p, 0] = cams[p - 1, 1]
            mine = np.unique(seg[:, 0].astype(int)) if len(seg) else np.zeros(0, int)
            pts[:3, mine] = X[mine].T
            pts[3, mine] = 1.0
    # the largest pixel error of every track under the returned cameras, +inf behind one
    err = np.zeros(T)
    with np.errstate(all="ignore"):
        for tr in range(T):
            x = pts[:3, tr] / pts[3, tr]
            e2 = 0.0
            for r in ob[ob[:, 0] == tr]:
                q, b = int(r[1]), int(r[2])
                deg = reports[int(root[q])]["status"] == DEGENERATE
                if deg:                                           # the cameras as they are returned: the input slots
                    slot = 1 if b == q else 0
                    Rm, tm = cams_in[q, slot, :9].reshape(3, 3), cams_in[q, slot, 9:]
                elif b < 0:
                    Rm, tm = np.eye(3), np.zeros(3)
                else:
                    Rm, tm = R[b], t[b]
                Y = Rm @ x + tm
                ex, ey = Y[0] / Y[2] - r[3], Y[1] / Y[2] - r[4]
                v = (r[5] * ex + r[6] * ey) ** 2 + (r[7] * ey) ** 2
                e2 = max(e2, v if (Y[2] > 0 and v <= 3.0e38) else np.inf)
            err[tr] = np.sqrt(e2)
    blocks = ob[:, 2].astype(int) if len(ob) else np.zeros(0, int)
    return dict(cams=cams, points=pts, used=used, err=err, reports=reports, accepts=accepts, blocks=blocks, blockobs=blockobs)
