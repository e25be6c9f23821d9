"""The fp64 twin of sfm_adjust_ring (helper, not a test): chain_adjust_reference's Levenberg-Marquardt over a CLOSED ring.

One camera per VIEW: an observation with obs_cam = c is of view ((c >> 1) + (c & 1)) mod k; view 0 is the fixed [I|0] whichever
pair observes it, view v >= 1 is block v - 1 (k - 1 blocks), block 0 with 5 degrees of freedom.  A track is used when its flag
is REFINED or SEAM_REFINED (the rest of the used test is chain_adjust_reference's).  H is dense over all blocks -- no band, no
fold, no assumption about which blocks share a track -- the Schur complement and its solve are numpy's; the LM rules are
chain_adjust_reference.adjust_segment's, called as it is with the ring's blocks.  dense_system gives the reduced system itself,
for the band claim of DESIGN 6l and for the host build's reduction."""
import numpy as np

import chain_adjust_reference as CR

REFINED, SEAM_REFINED = 1, 3
CLOSED = 0
MIN_ROOT, MIN_OTHER = CR.MIN_ROOT, CR.MIN_OTHER
DEGENERATE = CR.DEGENERATE


def view_of(obs_cam, k):
    return ((obs_cam >> 1) + (obs_cam & 1)) % k


def fold_pos(block, nb):
    """The folded position of a block: positions 0, 1, 2, 3, ... hold blocks 0, nb - 1, 1, nb - 2, ..."""
    return 2 * block if block <= (nb - 1) // 2 else 2 * (nb - 1 - block) + 1


def band_width(W, nb):
    return min(2 * W, nb)


def observations(pairs, K, fused):
    """chain_adjust_reference.observations with the ring's blocks in column 2."""
    k = len(pairs)
    ob = CR.observations(pairs, K, dict(fused, root=np.zeros(k, int)))
    if len(ob):
        ob[:, 2] = [view_of(int(c), k) - 1 for c in fused["obs_cam"][:len(ob)]]
    return ob


def start_cameras(fused):
    """R, t of blocks 0 .. k - 2 from slot 2p + 1 (block 0's t normalised); slot 2 (k - 1) + 1 is not read."""
    k = len(fused["cams"])
    R, t = CR.start_cameras(dict(fused, root=np.zeros(k, int)))
    return R[:k - 1], t[:k - 1]


def used_tracks(fused, ob, R, t, W):
    flags = np.asarray(fused["flags"]).copy()
    flags[flags == SEAM_REFINED] = REFINED
    return CR.used_tracks(dict(fused, flags=flags), ob, R, t, W)


def dense_system(ob, X, R, t, huber, lam):
    """The damped reduced camera system S (6 nb x 6 nb, the unit row in place) and -b of the used observations ob at the state:
    chain_adjust_reference.adjust_segment's assembly, returned instead of solved.  Also the undamped per-block U, for scales."""
    nb = len(R)
    basis = CR.tangent_basis(t[0])
    tracks = np.unique(ob[:, 0].astype(int))
    slot = {tr: i for i, tr in enumerate(tracks)}
    tl = np.array([slot[int(x)] for x in ob[:, 0]], int)
    bl = ob[:, 2].astype(int)
    r, Jp, Jc, w, rho, _ = CR.terms(ob, X, R, t, basis, huber, 0)
    U = np.zeros((6 * nb, 6 * nb)); gc = np.zeros(6 * nb)
    Wm = np.zeros((6 * nb, 3 * len(tracks)))
    V = np.zeros((len(tracks), 3, 3)); gp = np.zeros((len(tracks), 3))
    np.add.at(V, tl, w[:, None, None] * np.einsum("mri,mrj->mij", Jp, Jp))
    np.add.at(gp, tl, w[:, None] * np.einsum("mri,mr->mi", Jp, r))
    for m in np.flatnonzero(bl >= 0):
        b, c = 6 * bl[m], 3 * tl[m]
        U[b:b + 6, b:b + 6] += w[m] * Jc[m].T @ Jc[m]
        gc[b:b + 6] += w[m] * Jc[m].T @ r[m]
        Wm[b:b + 6, c:c + 3] += w[m] * Jc[m].T @ Jp[m]
    Ud = U + lam * np.diag(np.diag(U))
    Ud[5, 5] = 1.0
    Vi = np.linalg.inv(V + lam * np.einsum("tij,ij->tij", V, np.eye(3)))
    WV = np.einsum("ctk,tkj->ctj", Wm.reshape(6 * nb, len(tracks), 3), Vi).reshape(6 * nb, -1)
    return Ud - WV @ Wm.T, -(gc - WV @ gp.ravel()), U


def band_check(Sd, W):
    """The band claim on a dense reduced system: (every block that is not exactly zero lies within band_width of the diagonal under
    the fold, some non-zero block lies in a corner of the unfolded matrix -- further than W - 1 blocks from the diagonal)."""
    nb = Sd.shape[0] // 6
    Wf = band_width(W, nb)
    inside, corner = True, False
    for P in range(nb):
        for Q in range(nb):
            if not Sd[6 * P:6 * P + 6, 6 * Q:6 * Q + 6].any():
                continue
            inside = inside and abs(fold_pos(P, nb) - fold_pos(Q, nb)) < Wf
            corner = corner or abs(P - Q) > W - 1
    return inside, corner


def adjust_ring(pairs, K, fused, ring_status=CLOSED, max_iterations=10, huber_px=1.0, min_rel_decrease=1e-6, initial_lambda=1e-3, max_track_views=8):
    """The whole call.  Returns cams (k, 2, 12) float64, points (4, T), used (T), err (T), report (a dict), accepts, blocks (per
    observation), blockobs (used observations per block) and band (the band claim held on the first system; None when none was
    formed)."""
    k, T, W = len(pairs), len(fused["flags"]), max_track_views
    cams_in = np.asarray(fused["cams"], np.float64)
    cams, pts = cams_in.copy(), np.asarray(fused["points"], np.float64).copy()
    ob = observations(pairs, K, fused)
    blocks = ob[:, 2].astype(int) if len(ob) else np.zeros(0, int)
    lens = np.diff(fused["track_offset"])
    if ring_status != CLOSED:
        rep = dict(ring_status=ring_status, status=0, iterations=0, accepted=0, num_cameras=0, num_tracks=0, num_seam_tracks=0, num_observations=0,
                   num_over_long=0, initial_rms_px=0.0, final_rms_px=0.0, final_cost=0.0, lambda_=0.0)
        used = np.zeros(T, bool)
        through, R, t = True, None, None
        seq, band, blockobs = [], None, np.zeros(k - 1, int)
    else:
        R, t = start_cameras(fused)
        used, X = used_tracks(fused, ob, R, t, W)
        uob = ob[used[ob[:, 0].astype(int)]] if len(ob) else ob
        blockobs = np.zeros(k - 1, int)
        for b in uob[:, 2].astype(int):
            if b >= 0:
                blockobs[b] += 1
        degenerate = bool(blockobs[0] < MIN_ROOT or (blockobs[1:] < MIN_OTHER).any())
        band = None
        if not degenerate and max_iterations > 0:
            band = band_check(dense_system(uob, X, R, t, huber_px, initial_lambda)[0], W)[0]
            assert band, "a non-zero block of the reduced system lies outside the folded band"
        rep, seq, Xs, Rs, ts = CR.adjust_segment(uob, X, R, t, 0, k - 1, max_iterations, huber_px, min_rel_decrease, initial_lambda, degenerate)
        del rep["root"]
        rep.update(ring_status=CLOSED, num_over_long=int((lens > W).sum()),
                   num_seam_tracks=int((used & (np.asarray(fused["flags"]) == SEAM_REFINED)).sum()))
        through = degenerate
        if not degenerate:
            R, t = Rs, ts
            for p in range(k):
                cams[p, 0] = cams_in[0, 0] if p == 0 else np.concatenate([R[p - 1].ravel(), t[p - 1]])
                cams[p, 1] = cams_in[0, 0] if p == k - 1 else np.concatenate([R[p].ravel(), t[p]])
            mine = np.flatnonzero(used)
            pts[:3, mine] = Xs[mine].T
            pts[3, mine] = 1.0
    # the largest pixel error of every track under the returned cameras, +inf behind one
    err = np.zeros(T)
    with np.errstate(all="ignore"):
        for tr in range(T):
            x = pts[:3, tr] / pts[3, tr]
            e2 = 0.0
            o0 = int(fused["track_offset"][tr])
            for i, r in enumerate(ob[ob[:, 0] == tr]):
                c, b = int(fused["obs_cam"][o0 + i]), int(r[2])
                if through:
                    Rm, tm = cams_in[c >> 1, c & 1, :9].reshape(3, 3), cams_in[c >> 1, c & 1, 9:]
                elif b < 0:
                    Rm, tm = np.eye(3), np.zeros(3)
                else:
                    Rm, tm = R[b], t[b]
                Y = Rm @ x + tm
                ex, ey = Y[0] / Y[2] - r[3], Y[1] / Y[2] - r[4]
                v = (r[5] * ex + r[6] * ey) ** 2 + (r[7] * ey) ** 2
                e2 = max(e2, v if (Y[2] > 0 and v <= 3.0e38) else np.inf)
            err[tr] = np.sqrt(e2)
    return dict(cams=cams, points=pts, used=used, err=err, report=rep, accepts=seq, blocks=blocks, blockobs=blockobs, band=band)
