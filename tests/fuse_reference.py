"""fp64 numpy twin of sfm_fuse_chain (cuda-sfm_amd/csrc/fuse_math.hpp, fuse.hip), written independently of it: the frames by
cuda_sfm_amd.chain_links' arithmetic per segment, the tracks built with dictionaries (best proposer per target, successor per
node), a dense Levenberg-Marquardt per track (all residuals of the track stacked, numpy's solver) under LmControl's damping /
accept / stop rules, the acceptance test stated on the pixel error.  Takes the chain dict of tests/fuse_scene.py."""
import numpy as np

REFINED, KEPT = 1, 2
DEGENERATE = 2
DEFAULTS = dict(threshold_px=4.0, max_iterations=5, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3)


def link_valid(L):
    sim = np.asarray(L["sim"], np.float64)
    return L["status"] != DEGENERATE and bool(np.isfinite(sim).all()) and sim[0] > 0


def frames(chain):
    """Per pair (s, R, t) into its segment's root frame (fp64), the roots and the number of segments."""
    out, roots = [], []
    for i in range(len(chain["pairs"])):
        if i == 0 or not link_valid(chain["links"][i - 1]):
            out.append((1.0, np.eye(3), np.zeros(3))); roots.append(i)
            continue
        v = np.asarray(chain["links"][i - 1]["sim"], np.float64)
        s, R, t = v[0], v[1:10].reshape(3, 3), v[10:13]
        si, Ri, ti = 1.0 / s, R.T, -(R.T @ t) / s
        s0, R0, t0 = out[-1]
        out.append((s0 * si, R0 @ Ri, s0 * (R0 @ ti) + t0)); roots.append(roots[-1])
    return out, np.array(roots, np.int32), len(set(roots))


def cameras(chain, fr):
    """(k, 2) cameras (R, t) of the root frame."""
    cams = []
    for P, (s, R, t) in zip(chain["pairs"], fr):
        pose = np.asarray(P["pose"], np.float64)
        R2, t2 = pose[:9].reshape(3, 3), pose[9:]
        cams.append(((R.T, -R.T @ t), (R2 @ R.T, s * t2 - R2 @ R.T @ t)))
    return cams


def live_nodes(P):
    pts = np.asarray(P["points"], np.float64)
    with np.errstate(all="ignore"):
        return (np.asarray(P["valid"]) != 0) & np.isfinite(pts).all(0) & (pts[3] != 0) & (pts[2] / pts[3] > 0)


def tracks(chain):
    """The track table: track (N), track_offset (T + 1), obs_cam (M), obs_record (M), the longest track in views."""
    pairs, links = chain["pairs"], chain["links"]
    k = len(pairs)
    off = np.concatenate([[0], np.cumsum([P["n"] for P in pairs])]).astype(int)
    live = [live_nodes(P) for P in pairs]
    best = {}                                                   # (pair, record) -> (err bits, proposer) of the winning edge
    for i in range(k - 1):
        L = links[i]
        if not link_valid(L):
            continue
        bits = np.asarray(L["err"], np.float32).view(np.uint32)
        for j in range(pairs[i]["n"]):
            m = int(L["index"][j])
            if not (L["inlier"][j] != 0 and 0 <= m < pairs[i + 1]["n"] and np.isfinite(L["err"][j]) and live[i][j] and live[i + 1][m]):
                continue
            key = (int(bits[j]), j)
            if (i + 1, m) not in best or key < best[(i + 1, m)]:
                best[(i + 1, m)] = key
    succ = {(i - 1, key[1]): (i, m) for (i, m), key in best.items()}
    track = np.full(off[-1], -1, np.int32)
    offsets, ocam, orec, longest = [0], [], [], 0
    for i in range(k):
        for j in range(pairs[i]["n"]):
            if not live[i][j] or (i, j) in best:
                continue
            t = len(offsets) - 1
            node = (i, j)
            while True:
                track[off[node[0]] + node[1]] = t
                ocam.append(2 * node[0]); orec.append(node[1])
                if node not in succ:
                    break
                node = succ[node]
            ocam.append(2 * node[0] + 1); orec.append(node[1])
            offsets.append(len(ocam))
            longest = max(longest, offsets[-1] - offsets[-2])
    return track, np.array(offsets, np.int32), np.array(ocam, np.int32), np.array(orec, np.int32), longest


def _residual(K, R, t, X, xy):
    """Pixel residual (2), its Jacobian by X (2 x 3) and the depth of X in camera [R|t]."""
    Y = R @ X + t
    with np.errstate(all="ignore"):
        iz = 1.0 / Y[2]
        px, py = Y[0] * iz, Y[1] * iz
        e = np.array([px - xy[0], py - xy[1]])
        r = K[:2, :2] @ e
        J = K[:2, :2] @ np.array([[iz, 0.0, -px * iz], [0.0, iz, -py * iz]]) @ R
    return r, J, Y[2]


def _huber(r, h):
    e2 = float(r @ r)
    if h > 0 and e2 > h * h:
        e = np.sqrt(e2)
        return h / e, 2 * h * e - h * h
    return 1.0, e2


def _cost(K, views, X, h):
    with np.errstate(all="ignore"):
        return sum(_huber(_residual(K, R, t, X, xy)[0], h)[1] for R, t, xy in views)


def point_lm(K, views, X0, max_iterations, huber_px, min_rel_decrease, initial_lambda):
    """Dense LM of one point over its views [(R, t, xy)]."""
    X = np.array(X0, np.float64)
    lam, cost, it = float(initial_lambda), _cost(K, views, X0, huber_px), 0
    while it < max_iterations:
        rows, res = [], []
        for R, t, xy in views:
            r, J, _ = _residual(K, R, t, X, xy)
            w = np.sqrt(_huber(r, huber_px)[0])
            rows.append(w * J); res.append(w * r)
        J = np.vstack(rows); r = np.concatenate(res)
        V = J.T @ J
        D = V + lam * np.diag(np.diag(V))
        it += 1
        ok = np.isfinite(D).all() and abs(np.linalg.det(D)) > 0
        if ok:
            Xt = X - np.linalg.solve(D, J.T @ r)
            ok = bool(np.isfinite(Xt).all())
        nc = _cost(K, views, Xt, huber_px) if ok else np.inf
        if ok and nc < cost:
            rel = (cost - nc) / cost
            X, cost, lam = Xt, nc, lam / 10.0
            if not rel >= min_rel_decrease:
                break
        else:
            lam *= 10.0
            if lam > 1e16:
                break
    return X


def pixel_error(K, views, X):
    """The largest pixel error over the views (inf behind a camera or where it is not finite)."""
    worst = 0.0
    for R, t, xy in views:
        r, _, z = _residual(K, R, t, X, xy)
        with np.errstate(all="ignore"):
            e = np.sqrt(r @ r)
        worst = max(worst, e if (z > 0 and np.isfinite(e)) else np.inf)
    return worst


def observation(P, slot, rec):
    X = np.asarray(P["X1" if slot else "X0"], np.float64)
    return X[:2, rec] / X[2, rec]


def fuse(chain, **kw):
    """The whole call.  Returns the dict cuda_sfm_amd.fuse_chain returns, all fp64, + start (T x 3: the mean of the path's points)
    and X (T x 3: the LM result, stored or not)."""
    p = dict(DEFAULTS); p.update(kw)
    K = np.asarray(chain["K"], np.float64)
    pairs = chain["pairs"]
    k = len(pairs)
    fr, roots, segs = frames(chain)
    cams = cameras(chain, fr)
    track, offsets, ocam, orec, longest = tracks(chain)
    T = len(offsets) - 1
    pts = np.ones((4, T)); flags = np.zeros(T, np.uint8); err = np.zeros(T); start = np.zeros((T, 3)); Xlm = np.zeros((T, 3))
    for t in range(T):
        o0, o1 = offsets[t], offsets[t + 1]
        carried = []
        for o in range(o0, o1 - 1):
            i, rec = ocam[o] >> 1, orec[o]
            x = np.asarray(pairs[i]["points"], np.float64)[:, rec]
            s, R, tt = fr[i]
            carried.append(s * (R @ (x[:3] / x[3])) + tt)
        start[t] = np.mean(carried, 0)
        views = [(cams[ocam[o] >> 1][ocam[o] & 1][0], cams[ocam[o] >> 1][ocam[o] & 1][1], observation(pairs[ocam[o] >> 1], ocam[o] & 1, orec[o]))
                 for o in range(o0, o1)]
        Xlm[t] = point_lm(K, views, start[t], p["max_iterations"], p["huber_px"], p["min_rel_decrease"], p["initial_lambda"])
        err[t] = pixel_error(K, views, Xlm[t])
        ok = err[t] < p["threshold_px"]
        flags[t] = REFINED if ok else KEPT
        pts[:3, t] = Xlm[t] if ok else start[t]
    counts = dict(tracks=T, observations=int(offsets[-1]), refined=int((flags == REFINED).sum()), kept=int((flags == KEPT).sum()), segments=segs,
                  longest_track=longest)
    return dict(frames=np.array([np.concatenate([[s], R.ravel(), t]) for s, R, t in fr]).reshape(k, 13), root=roots,
                cams=np.array([[np.concatenate([c[0].ravel(), c[1]]) for c in pc] for pc in cams]).reshape(k, 2, 12), track=track,
                track_offset=offsets, obs_cam=ocam, obs_record=orec, points=pts, flags=flags, err=err, counts=counts, start=start, X=Xlm)
