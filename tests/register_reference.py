"""fp64 numpy twin of the view registration (csrc/register.hip, csrc/register_math.hpp) for the tests: an independent P3P
(the three distance equations solved by one-dimensional root bracketing in lambda1, the pose by Kabsch alignment), the pixel
error and the inlier test, and the pose-only Levenberg-Marquardt with the same parameterisation, loss, damping and stop rules
as the GPU's (R <- exp([w]x) R, t <- t + dt; Huber on the 2-D pixel residual)."""
import numpy as np

from refine_reference import expso3, rotation_angle  # noqa: F401  (re-exported for the tests)


def kabsch(A, B):
    """R, t with B ~ R A + t (rows are points), least squares."""
    ca, cb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((A - ca).T @ (B - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cb - R @ ca


def p3p(bearings, X, samples=20000):
    """Every pose (R, t) with R X_i + t = l_i y_i, l_i > 0, for unit bearings y (3 x 3) and points X (3 x 3): l2 and l3 as
    functions of l1 from the first two distance equations (four sign branches), the roots of the third by bracketing on a
    dense grid and bisection."""
    y = np.asarray(bearings, np.float64); X = np.asarray(X, np.float64)
    cg, cb, ca = y[0] @ y[1], y[0] @ y[2], y[1] @ y[2]
    c2, b2, a2 = np.sum((X[0] - X[1]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[1] - X[2]) ** 2)
    sg2, sb2 = 1.0 - cg * cg, 1.0 - cb * cb
    lmax = min(np.sqrt(c2 / sg2), np.sqrt(b2 / sb2))

    def branch(l1, s2, s3):
        l2 = l1 * cg + s2 * np.sqrt(np.maximum(c2 - l1 * l1 * sg2, 0.0))
        l3 = l1 * cb + s3 * np.sqrt(np.maximum(b2 - l1 * l1 * sb2, 0.0))
        return l2, l3, l2 * l2 + l3 * l3 - 2.0 * l2 * l3 * ca - a2

    out = []
    grid = np.linspace(lmax * 1e-9, lmax, samples)
    for s2 in (1.0, -1.0):
        for s3 in (1.0, -1.0):
            f = branch(grid, s2, s3)[2]
            for i in np.flatnonzero(np.sign(f[:-1]) * np.sign(f[1:]) < 0):
                lo, hi = grid[i], grid[i + 1]
                flo = f[i]
                for _ in range(80):
                    mid = 0.5 * (lo + hi)
                    fm = branch(mid, s2, s3)[2]
                    if np.sign(fm) == np.sign(flo):
                        lo, flo = mid, fm
                    else:
                        hi = mid
                l1 = 0.5 * (lo + hi)
                l2, l3, _ = branch(l1, s2, s3)
                if l2 > 0 and l3 > 0:
                    out.append(kabsch(X, y * np.array([l1, l2, l3])[:, None]))
    return out


def pixel_residual(cam, R, t, X, obs):
    """K2x2 (pi(R X + t) - obs) per point (n x 2) and the depths."""
    fx, s, fy = cam
    Y = X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    px, py = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
    ex, ey = px - obs[:, 0], py - obs[:, 1]
    return np.stack([fx * ex + s * ey, fy * ey], 1), Y[:, 2]


def pixel_error(cam, R, t, X, obs):
    r, z = pixel_residual(cam, R, t, X, obs)
    return np.where(z > 0, np.hypot(r[:, 0], r[:, 1]), np.inf)


def jacobian(cam, R, t, X, obs):
    """Residuals (n x 2) and d r / d (omega, dt) (n x 2 x 6) for R <- exp([omega]x) R, t <- t + dt."""
    fx, s, fy = cam
    q = X @ np.asarray(R, np.float64).T
    Y = q + np.asarray(t, np.float64)
    iz = 1.0 / Y[:, 2]
    px, py = Y[:, 0] * iz, Y[:, 1] * iz
    r = np.stack([fx * (px - obs[:, 0]) + s * (py - obs[:, 1]), fy * (py - obs[:, 1])], 1)
    Jy = np.zeros((len(X), 2, 3))
    Jy[:, 0, 0] = fx * iz; Jy[:, 0, 1] = s * iz; Jy[:, 0, 2] = -(fx * px + s * py) * iz
    Jy[:, 1, 1] = fy * iz; Jy[:, 1, 2] = -fy * py * iz
    J = np.zeros((len(X), 2, 6))
    J[:, :, :3] = np.cross(q[:, None, :], Jy)          # row j of Jy times -[q]x is q x j
    J[:, :, 3:] = Jy
    return r, J


def huber(r, h):
    e2 = np.sum(r * r, 1)
    if h <= 0:
        return e2, np.ones(len(r))
    e = np.sqrt(e2)
    big = e2 > h * h
    return np.where(big, 2.0 * h * e - h * h, e2), np.where(big, h / np.maximum(e, 1e-300), 1.0)


def refine_pose(cam, R, t, X, obs, max_iterations=10, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3):
    """The GPU's pose LM in fp64 over the given correspondences."""
    R = np.asarray(R, np.float64).copy(); t = np.asarray(t, np.float64).copy()
    X = np.asarray(X, np.float64); obs = np.asarray(obs, np.float64)
    n = len(X)

    def cost(R_, t_):
        r, _ = pixel_residual(cam, R_, t_, X, obs)
        rho, _ = huber(r, huber_px)
        return rho.sum(), np.sum(r * r)

    c, sq = cost(R, t)
    rms0 = np.sqrt(sq / (2 * n))
    lam, iters, accepted, status = float(initial_lambda), 0, 0, 1
    while iters < max_iterations:
        r, J = jacobian(cam, R, t, X, obs)
        _, w = huber(r, huber_px)
        H = np.einsum("n,nki,nkj->ij", w, J, J)
        g = np.einsum("n,nki,nk->i", w, J, r)
        A = H + lam * np.diag(np.diag(H))
        iters += 1
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            lam *= 10.0
            if lam > 1e16:
                break
            continue
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        Rt, tt = expso3(d[:3]) @ R, t + d[3:]
        nc, nsq = cost(Rt, tt)
        if nc < c:
            rel = (c - nc) / c
            R, t, c, sq = Rt, tt, nc, nsq
            accepted += 1
            lam /= 10.0
            if not rel >= min_rel_decrease:
                status = 0
                break
        else:
            lam *= 10.0
            if lam > 1e16:
                break
    return {"R": R, "t": t, "status": status, "iterations": iters, "accepted": accepted, "initial_rms_px": rms0,
            "final_rms_px": np.sqrt(sq / (2 * n)), "final_cost": c}
