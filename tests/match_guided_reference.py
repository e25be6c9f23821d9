"""fp64 twin of sfm_match_guided (helper, not a test).  It shares no code with the library or the host build: the gate is stated
on DISTANCES IN PIXELS -- a row is in the band when it lies within `band` pixels of the query's epipolar line in view 2 and the
query within `band` pixels of the row's line in view 1 -- the scores are one fp64 matrix product, and the top two come from a
sort.

The library decides the same gate in fp32 without a division (d^2 <= band^2 |l|^2).  Its d = l0 x2 + l1 y2 + l2 is formed from an
fp32 line through pixel coordinates of up to ~1000: each of the at most 11 roundings on the way (three per line coefficient with
an fma chain of two, two more in the residual, the limit's three) is at most 2^-24 of a term no larger than ~1000 |(l0, l1)|, so the
fp32 distance is off by at most about 11 * 2^-24 * 1000 = 6.6e-4 px.  TIE_PX = 1e-3 px is that bound with a margin.  A row whose
fp64 distance (either one) lies within TIE_PX of the band is one that fp32 may decide either way; the twin therefore computes every
query twice, with all such rows counted IN and with all of them counted OUT."""
import numpy as np

TIE_PX = 1e-3
TIE_SCORE = 2e-5            # two fp32 chains of 128 non-negative terms <= 1: 129 roundings of at most 2^-24 relative each


def _lines(F, x, y):
    u = np.stack([x, y, np.ones_like(x)], 1)               # n x 3
    return u @ F.T                                          # row i: F u_i


def distances(sift1, sift2, F):
    """(dist2, dist1), n1 x n2 each: the distance of row j to query i's line in view 2, and of query i to row j's line in view 1;
    inf where a line is undefined (norm 0 or not finite) and nan where a position is."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    x1, y1 = sift1["xpos"].astype(np.float64), sift1["ypos"].astype(np.float64)
    x2, y2 = sift2["xpos"].astype(np.float64), sift2["ypos"].astype(np.float64)
    with np.errstate(all="ignore"):
        l = _lines(F, x1, y1)                               # lines in view 2
        lt = _lines(F.T, x2, y2)                            # lines in view 1
        d = l[:, 0:1] * x2[None, :] + l[:, 1:2] * y2[None, :] + l[:, 2:3]
        n2v = np.hypot(l[:, 0], l[:, 1])[:, None]
        n1v = np.hypot(lt[:, 0], lt[:, 1])[None, :]
        dist2 = np.where((n2v > 0) & np.isfinite(n2v), np.abs(d) / n2v, np.inf)
        dist1 = np.where((n1v > 0) & np.isfinite(n1v), np.abs(d) / n1v, np.inf)
    return dist2, dist1


def scores(sift1, sift2):
    return sift1["data"].astype(np.float64) @ sift2["data"].astype(np.float64).T


def top2(S, allowed):
    """best, second, index per row of S over the allowed columns; start values (0, 0, -1), strict '>', lowest index on ties"""
    n1, n2 = S.shape
    M = np.where(allowed, S, -np.inf)
    idx = np.argmax(M, 1) if n2 else np.zeros(n1, np.int64)
    best = M[np.arange(n1), idx] if n2 else np.full(n1, -np.inf)
    M2 = M.copy()
    if n2:
        M2[np.arange(n1), idx] = -np.inf
    second = M2.max(1) if n2 else np.full(n1, -np.inf)
    idx2 = np.argmax(M2, 1) if n2 else np.zeros(n1, np.int64)
    none = ~(best > 0)
    return (np.where(none, 0.0, best), np.where(none, 0.0, np.maximum(second, 0.0)), np.where(none, -1, idx).astype(np.int64),
            np.where(none | ~(second > 0), -1, idx2).astype(np.int64))


def result(S, allowed, sift2):
    best, second, idx, idx2 = top2(S, allowed)
    safe = np.maximum(idx, 0)
    return {"score": best, "second": second, "match": idx, "runner_up": idx2,
            "match_xpos": np.where(idx >= 0, sift2["xpos"][safe].astype(np.float64), 0.0) if len(sift2) else np.zeros(len(idx)),
            "match_ypos": np.where(idx >= 0, sift2["ypos"][safe].astype(np.float64), 0.0) if len(sift2) else np.zeros(len(idx)),
            "ambiguity": second / (best + 1e-6),
            "tied": (idx >= 0) & (best - second <= TIE_SCORE)}


def match_guided(sift1, sift2, F, band):
    """(wide, narrow, undecided): the twin's result with every row within TIE_PX of the band counted in / counted out, and the
    queries where the two differ in `match`."""
    S = scores(sift1, sift2)
    dist2, dist1 = distances(sift1, sift2, F)
    with np.errstate(invalid="ignore"):
        far = np.maximum(dist1, dist2)                      # (nan propagates: never in the band)
        wide = result(S, far <= band + TIE_PX, sift2)
        narrow = result(S, far <= band - TIE_PX, sift2)
    return wide, narrow, wide["match"] != narrow["match"]


def match_plain(sift1, sift2):
    S = scores(sift1, sift2)
    return result(S, np.ones(S.shape, bool), sift2)
