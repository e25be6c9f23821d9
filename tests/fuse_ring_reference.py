"""fp64 numpy twin of sfm_fuse_ring (cuda-sfm_amd/csrc/fuse_ring_math.hpp, fuse_ring.hip), written independently of it:
fuse_reference.tracks over the first k - 1 links gives the chain tracks as lists of nodes; the join rule is applied to those lists
with dictionaries (no keys, no successors, no walks); then fuse_reference's frames, cameras, dense LM and acceptance.  Takes the
ring chain dict of tests/fuse_ring_scene.py."""
import numpy as np

import fuse_reference as FR
from refine_reference import rotation_angle

REFINED, KEPT, SEAM_REFINED, SEAM_KEPT = 1, 2, 3, 4
CLOSED, OPEN, REJECTED = 0, 1, 2
GATES = dict(max_closure_rotation_rad=1e-3, max_closure_log_scale=1e-3)


def closure(ring, fr):
    """(status, first invalid link or -1, ln s, rotation angle, |t|) of D = F_{k-1} o L_{k-1}^-1."""
    bad = [i for i, L in enumerate(ring["links"]) if not FR.link_valid(L)]
    if bad:
        return OPEN, bad[0], 0.0, 0.0, 0.0
    v = np.asarray(ring["links"][-1]["sim"], np.float64)
    s, R, t = v[0], v[1:10].reshape(3, 3), v[10:13]
    s0, R0, t0 = fr[-1]
    sD, RD, tD = s0 / s, R0 @ R.T, t0 - (s0 / s) * (R0 @ R.T @ t)
    angle = rotation_angle(np.eye(3), RD)                       # (not arccos of the trace: fp32 links are orthonormal to 1e-7 only)
    return None, -1, float(np.log(sD)), angle, float(np.linalg.norm(tD))


def join(ring, chain_tracks, where):
    """The join rule over the chain tracks (lists of (pair, record) nodes); where: node -> its chain track's number.  Returns the
    joined tracks in head order, which of them cross the seam, and (proposals, ineligible, joins)."""
    pairs, L = ring["pairs"], ring["links"][-1]
    k = len(pairs)
    live_last, live_first = FR.live_nodes(pairs[-1]), FR.live_nodes(pairs[0])
    bits = np.asarray(L["err"], np.float32).view(np.uint32)
    proposals = ineligible = 0
    best = {}                                                   # record m of pair 0 -> (err bits, proposer) among the ELIGIBLE
    for j in range(pairs[-1]["n"]):
        m = int(L["index"][j])
        if not (L["inlier"][j] != 0 and 0 <= m < pairs[0]["n"] and np.isfinite(L["err"][j]) and live_last[j] and live_first[m]):
            continue
        proposals += 1
        A, B = chain_tracks[where[(k - 1, j)]], chain_tracks[where[(0, m)]]
        assert A[-1] == (k - 1, j) and B[0] == (0, m)           # A ends at the seam, every live node of pair 0 heads its track
        if not len(B) < A[0][0]:
            ineligible += 1
            continue
        key = (int(bits[j]), j)
        if m not in best or key < best[m]:
            best[m] = key
    merged, gone = {}, set()
    for m, (_, j) in best.items():
        a, b = where[(k - 1, j)], where[(0, m)]
        assert a not in merged and b not in gone
        merged[a] = chain_tracks[a] + chain_tracks[b]
        gone.add(b)
    assert not (set(merged) & gone)                             # a track crosses the seam at most once
    out, seam = [], []
    for t, nodes in enumerate(chain_tracks):
        if t in gone:
            continue
        out.append(merged.get(t, nodes)); seam.append(t in merged)
    return out, np.array(seam, bool), (proposals, ineligible, len(best))


def fuse(ring, **kw):
    """The whole call: the dict cuda_sfm_amd.fuse_ring returns, all fp64, + start, X (as fuse_reference.fuse) and seam (T, bool)."""
    p = dict(FR.DEFAULTS); p.update(GATES); p.update(kw)
    K = np.asarray(ring["K"], np.float64)
    pairs = ring["pairs"]
    k = len(pairs)
    chain = dict(ring, links=ring["links"][:-1])
    fr, roots, segs = FR.frames(chain)
    cams = FR.cameras(chain, fr)
    off = np.concatenate([[0], np.cumsum([P["n"] for P in pairs])]).astype(int)
    _, offsets, ocam, orec, _ = FR.tracks(chain)
    chain_tracks = [[(int(ocam[o]) >> 1, int(orec[o])) for o in range(offsets[t], offsets[t + 1] - 1)] for t in range(len(offsets) - 1)]
    where = {node: t for t, nodes in enumerate(chain_tracks) for node in nodes}
    status, first_invalid, ls, angle, tn = closure(ring, fr)
    if status is None:
        status = CLOSED if angle <= p["max_closure_rotation_rad"] and abs(ls) <= p["max_closure_log_scale"] else REJECTED
    counts3 = (0, 0, 0)
    tracks, seam = chain_tracks, np.zeros(len(chain_tracks), bool)
    if status == CLOSED:
        tracks, seam, counts3 = join(ring, chain_tracks, where)
    T = len(tracks)
    track = np.full(off[-1], -1, np.int32)
    offs, oc, orc = [0], [], []
    for t, nodes in enumerate(tracks):
        assert len(nodes) <= k and all(b[0] == (a[0] + 1) % k for a, b in zip(nodes, nodes[1:]))    # every view at most once
        for i, j in nodes:
            track[off[i] + j] = t
            oc.append(2 * i); orc.append(j)
        oc.append(2 * nodes[-1][0] + 1); orc.append(nodes[-1][1])
        offs.append(len(oc))
    pts = np.ones((4, T)); flags = np.zeros(T, np.uint8); err = np.zeros(T); start = np.zeros((T, 3)); Xlm = np.zeros((T, 3))
    for t, nodes in enumerate(tracks):
        carried = []
        for i, rec in nodes:
            x = np.asarray(pairs[i]["points"], np.float64)[:, rec]
            s, R, tt = fr[i]
            carried.append(s * (R @ (x[:3] / x[3])) + tt)
        start[t] = np.mean(carried, 0)
        obs = [(i, 0, rec) for i, rec in nodes] + [(nodes[-1][0], 1, nodes[-1][1])]
        views = [(cams[i][slot][0], cams[i][slot][1], FR.observation(pairs[i], slot, rec)) for i, slot, rec in obs]
        Xlm[t] = FR.point_lm(K, views, start[t], p["max_iterations"], p["huber_px"], p["min_rel_decrease"], p["initial_lambda"])
        err[t] = FR.pixel_error(K, views, Xlm[t])
        ok = err[t] < p["threshold_px"]
        flags[t] = (REFINED if ok else KEPT) + (2 if seam[t] else 0)
        pts[:3, t] = Xlm[t] if ok else start[t]
    refined = int(np.isin(flags, (REFINED, SEAM_REFINED)).sum())
    counts = dict(tracks=T, observations=len(oc), refined=refined, kept=T - refined, segments=segs,
                  longest_track=max([len(n) + 1 for n in tracks], default=0))
    report = dict(status=status, first_invalid=first_invalid, closure_log_scale=ls, closure_rotation_rad=angle, closure_t=tn,
                  seam_proposals=counts3[0], seam_ineligible=counts3[1], seam_tracks=counts3[2],
                  seam_refined=int((flags == SEAM_REFINED).sum()), seam_kept=int((flags == SEAM_KEPT).sum()))
    return dict(frames=np.array([np.concatenate([[s], R.ravel(), t]) for s, R, t in fr]).reshape(k, 13), root=roots,
                cams=np.array([[np.concatenate([c[0].ravel(), c[1]]) for c in pc] for pc in cams]).reshape(k, 2, 12), track=track,
                track_offset=np.array(offs, np.int32), obs_cam=np.array(oc, np.int32), obs_record=np.array(orc, np.int32), points=pts,
                flags=flags, err=err, counts=counts, start=start, X=Xlm, seam=seam, report=report)
