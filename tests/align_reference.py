"""fp64 numpy twin of sfm_align_pair (helper, not a test), independent of csrc/align_math.hpp: the gate, the sampler, Umeyama's
similarity by SVD on the same three samples, the two-way pixel test, and the 7-parameter Levenberg-Marquardt with a dense
4m x 7 Jacobian.  A link is (s, R, t) with X_B = s R X_A + t."""
import numpy as np

import refine_reference as RR

M32 = 0xFFFFFFFF


def hash32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def sample3(seed, hyp, m):
    """Three distinct candidate ids, the library's hash sampler as a plain loop (device_math.hpp: sample_distinct)."""
    base = hash32(hash32(seed) + hyp)
    idx, k = [], 0
    while len(idx) < 3 and k < 256:
        c = (hash32(base + k * 0x9E3779B9) * m) >> 32
        k += 1
        if c not in idx:
            idx.append(c)
    c = 0
    while len(idx) < 3:
        if c not in idx:
            idx.append(c % max(m, 1))
        c += 1
    return idx


def umeyama(a, b):
    """(s, R, t) minimising sum |b - (s R a + t)|^2 over the rows of a, b (Umeyama 1991), or None for a degenerate set."""
    ma, mb = a.mean(0), b.mean(0)
    da, db = a - ma, b - mb
    va = (da * da).sum()
    U, D, Vt = np.linalg.svd(db.T @ da)
    if not (va > 0 and D[1] > 1e-12 * D[0]):
        return None
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = np.sqrt((db * db).sum() / va)              # the ratio of the spreads (exact for 3 points; the header's definition)
    return s, R, mb - s * R @ ma


def cams(K):
    K = np.asarray(K, np.float64)
    return np.array([[K[0, 0], K[0, 1]], [0.0, K[1, 1]]])


def gather(A, B, index):
    """Candidates in record order: (records j, Xa, Xb, oa, ob), fp64."""
    na, nb = A["n"], B["n"]
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < nb)
    k = np.clip(index, 0, nb - 1)

    def usable(P, v):
        P = np.asarray(P, np.float32)
        with np.errstate(all="ignore"):
            u = np.isfinite(P).all(0) & (P[3] != 0) & (P[2] / P[3] > 0)
        return u if v is None else u & (np.asarray(v) != 0)
    ok &= usable(A["points"], A.get("valid")) & usable(B["points"], B.get("valid"))[k]
    j = np.flatnonzero(ok)
    kb = k[j]
    Pa, Pb = np.asarray(A["points"], np.float64), np.asarray(B["points"], np.float64)
    Xa = (Pa[:3, j] / Pa[3, j]).T
    Xb = (Pb[:3, kb] / Pb[3, kb]).T
    X0a, X0b = np.asarray(A["X0"], np.float64), np.asarray(B["X0"], np.float64)
    oa = (X0a[:2, j] / X0a[2, j]).T
    ob = (X0b[:2, kb] / X0b[2, kb]).T
    return j, Xa, Xb, oa, ob


def residuals(Ka, Kb, sim, Xa, Xb, oa, ob):
    """m x 4 pixel residuals (forward x, y, backward x, y) and the two depths."""
    s, R, t = sim
    Y = s * Xa @ R.T + t
    Z = (Xb - t) @ R
    with np.errstate(all="ignore"):
        rf = (Y[:, :2] / Y[:, 2:] - ob) @ Kb.T
        rb = (Z[:, :2] / Z[:, 2:] - oa) @ Ka.T
    return np.hstack([rf, rb]), Y[:, 2], Z[:, 2]


def errors(Ka, Kb, sim, Xa, Xb, oa, ob):
    """The larger of the two pixel errors per candidate, +inf behind a camera."""
    r, zf, zb = residuals(Ka, Kb, sim, Xa, Xb, oa, ob)
    e = np.maximum(np.hypot(r[:, 0], r[:, 1]), np.hypot(r[:, 2], r[:, 3]))
    return np.where((zf > 0) & (zb > 0) & np.isfinite(e), e, np.inf)


def jacobian(Ka, Kb, sim, Xa, Xb):
    """Dense 4m x 7: d r / d (omega, dt, dsigma) for R <- exp([omega]x) R, t <- t + dt, s <- s exp(dsigma)."""
    s, R, t = sim
    m = len(Xa)
    q = s * Xa @ R.T
    Y = q + t
    d = Xb - t
    Z = d @ R

    def dproj(K2, P):
        iz = 1.0 / P[:, 2]
        D = np.zeros((m, 2, 3))
        D[:, 0, 0] = iz; D[:, 0, 2] = -P[:, 0] * iz * iz
        D[:, 1, 1] = iz; D[:, 1, 2] = -P[:, 1] * iz * iz
        return np.einsum("ab,mbc->mac", K2, D)

    def skew(v):
        S = np.zeros((m, 3, 3))
        S[:, 0, 1], S[:, 0, 2] = -v[:, 2], v[:, 1]
        S[:, 1, 0], S[:, 1, 2] = v[:, 2], -v[:, 0]
        S[:, 2, 0], S[:, 2, 1] = -v[:, 1], v[:, 0]
        return S
    Jf, Jb = dproj(Kb, Y), dproj(Ka, Z)
    J = np.zeros((m, 4, 7))
    J[:, :2, :3] = -Jf @ skew(q)
    J[:, :2, 3:6] = Jf
    J[:, :2, 6] = np.einsum("mac,mc->ma", Jf, q)
    J[:, 2:, :3] = Jb @ (R.T[None] @ skew(d))
    J[:, 2:, 3:6] = -Jb @ R.T[None]
    return J


def huber(r2, h):
    """Per residual pair (m x 2): cost and IRLS weight, refine_math.hpp's rule."""
    e2 = (r2 * r2).sum(1)
    e = np.sqrt(e2)
    big = (h > 0) & (e2 > h * h)
    with np.errstate(all="ignore"):
        return np.where(big, 2 * h * e - h * h, e2), np.where(big, h / e, 1.0)


def refine(Ka, Kb, sim, Xa, Xb, oa, ob, max_iterations=10, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3):
    """The LM chain with LmControl's rules.  Returns (sim, dict(iterations, accepted, converged, initial_rms, final_rms, cost))."""
    def cost(sm):
        r, _, _ = residuals(Ka, Kb, sm, Xa, Xb, oa, ob)
        return huber(r[:, :2], huber_px)[0].sum() + huber(r[:, 2:], huber_px)[0].sum(), (r * r).sum()
    m = len(Xa)
    c, sq = cost(sim)
    sq0 = sq
    lam, it, acc, conv = float(initial_lambda), 0, 0, False
    while it < max_iterations:
        r, _, _ = residuals(Ka, Kb, sim, Xa, Xb, oa, ob)
        J = jacobian(Ka, Kb, sim, Xa, Xb)
        w = np.repeat(np.stack([huber(r[:, :2], huber_px)[1], huber(r[:, 2:], huber_px)[1]], 1), 2, axis=1)      # m x 4
        Jw = J * w[:, :, None]
        H = np.einsum("mai,maj->ij", Jw, J)
        g = np.einsum("mai,ma->i", Jw, r)
        Hd = H + lam * np.diag(np.diag(H))
        it += 1
        try:
            L = np.linalg.cholesky(Hd)
        except np.linalg.LinAlgError:
            lam *= 10
            if lam > 1e16:
                break
            continue
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        s, R, t = sim
        trial = (s * np.exp(d[6]), RR.expso3(d[:3]) @ R, t + d[3:6])
        nc, nsq = cost(trial)
        if nc < c:
            rel = (c - nc) / c
            sim, c, sq = trial, nc, nsq
            acc += 1
            lam /= 10
            if not rel >= min_rel_decrease:
                conv = True
                break
        else:
            lam *= 10
            if lam > 1e16:
                break
    rms = lambda v: float(np.sqrt(v / (4.0 * m))) if m else 0.0
    return sim, dict(iterations=it, accepted=acc, converged=conv, initial_rms=rms(sq0), final_rms=rms(sq), cost=float(c))


def score(Ka, Kb, thr, sim, c):
    return errors(Ka, Kb, sim, *c[1:]) < thr


def run(A, B, index, Ka, Kb, num_hypotheses=4096, seed=0x5EED5F3D, threshold_px=4.0, inliers=None, start=None, **lm):
    """The whole call in fp64.  inliers (bool over the candidates) and start (s, R, t) replace the RANSAC stage where given, so
    the LM can be compared from the same inlier set.  Returns a dict: records, counts, best, ransac (s, R, t), sim, inlier (n),
    err (n), margin (per candidate: larger pixel error / threshold under sim), lm."""
    Ka, Kb = cams(Ka), cams(Kb)
    c = gather(A, B, index)
    j, Xa, Xb, oa, ob = c
    m = len(j)
    counts, best, win = None, None, start
    if start is None:
        counts = np.zeros(num_hypotheses, np.int64)
        sims = [None] * num_hypotheses
        if m >= 3:
            for h in range(num_hypotheses):
                i = sample3(seed, h, m)
                sims[h] = umeyama(Xa[i], Xb[i])
                if sims[h] is not None:
                    counts[h] = int(score(Ka, Kb, threshold_px, sims[h], c).sum())
        best = int(np.argmax(counts))
        win = sims[best]
    degenerate = m < 3 or win is None
    if win is None:
        win = (1.0, np.eye(3), np.zeros(3))
    inl = (score(Ka, Kb, threshold_px, win, c) if inliers is None else np.asarray(inliers, bool)) if not degenerate else np.zeros(m, bool)
    degenerate = degenerate or inl.sum() < 6
    sim, info = win, None
    if not degenerate:
        sim, info = refine(Ka, Kb, win, Xa[inl], Xb[inl], oa[inl], ob[inl], **lm)
    e = errors(Ka, Kb, sim, Xa, Xb, oa, ob)
    na = A["n"]
    err = np.full(na, np.inf); err[j] = e
    flag = np.zeros(na, bool); flag[j] = (e < threshold_px) & (not degenerate)
    return dict(records=j, counts=counts, best=best, ransac=win, ransac_inliers=inl, sim=sim, inlier=flag, err=err,
                margin=e / threshold_px, lm=info, degenerate=degenerate)


def pack(sim):
    s, R, t = sim
    return np.concatenate([[s], np.asarray(R).ravel(), t])


def compose(l2, l1):
    """The link l2 after l1: X -> s2 R2 (s1 R1 X + t1) + t2."""
    s1, R1, t1 = l1
    s2, R2, t2 = l2
    return s1 * s2, R2 @ R1, s2 * R2 @ t1 + t2
