"""GPU: which of a pair's results are current after which call.  One pair on a small synthetic scene is walked
through a fixed sequence that visits every row of the transition table; after every step every getter and every
sfm_pair_device_ptr id is asked, and the answer (OK or SFM_E_STATE; pointer-is-NULL and size for the buffer ids) is compared
with a model of the two tables kept in this file.  Calls that fail must leave every answer as it was."""
import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd_synth import synth
from helpers import to_dev
import register_scene as RS

pytestmark = pytest.mark.gpu

POINTS, E, P, POSE, POINTS3D, REFINED, VIEW = "points", "E", "P", "pose", "points3d", "refined", "view"
ALL = frozenset((POINTS, E, P, POSE, POINTS3D, REFINED, VIEW))


class Model:
    """The first table: what a successful call sets and clears."""

    def __init__(self, n):
        self.have = set()
        self.n = n
        self.last_count = 0          # hypotheses the plain count / candidate getters describe
        self.scored = False          # the per-shard buffers exist (grown by the first scoring launch)
        self.view_hyps = 0

    def reset(self, n):
        self.have.clear(); self.n = n; self.last_count = 0

    def points_replaced(self):
        self.have = {POINTS}; self.last_count = 0

    def E_finalized(self):
        self.have -= {P, POSE, POINTS3D}; self.have.add(E)

    def scored_shard(self, count):
        self.last_count = count; self.scored = True

    def candidates(self):
        self.have -= {POSE, POINTS3D}; self.have.add(P)

    def pose_chosen(self):
        self.have.discard(POINTS3D); self.have.add(POSE)

    def chain(self):
        self.have |= {P, POSE, POINTS3D}


def code_of(fn):
    try:
        fn()
    except S.SfmError as e:
        return e.code
    return S.OK


def probe(pair, m, vbo, where):
    """Every getter and every buffer id against the second table."""
    n, ld = m.n, (m.n + 127) // 128 * 128
    assert (pair.num_points, pair.ld) == (n, ld), where
    need = lambda *stages: S.OK if m.have.issuperset(stages) else S.E_STATE
    getters = [
        ("get_XU", lambda: pair.get_XU(S.BUF_X0), S.OK), ("get_key", pair.get_key, S.OK),
        ("get_inlier_counts", lambda: pair.get_inlier_counts(4096), S.OK), ("get_E_candidates", lambda: pair.get_E_candidates(4096), S.OK),
        ("get_E", pair.get_E, need(E)), ("get_best", pair.get_best, need(E)), ("get_inlier_mask", pair.get_inlier_mask, need(E)),
        ("get_pose_candidates", pair.get_pose_candidates, need(P)),
        ("get_pose_inverses", pair.get_pose_inverses, need(POSE)), ("get_pose_index", pair.get_pose_index, need(POSE)),
        ("get_result", pair.get_result, need(E, POSE)),
        ("get_points", pair.get_points, need(POINTS3D)), ("copy_points_to_vbo", lambda: pair.copy_points_to_vbo(vbo[0], vbo[1]), need(POINTS3D)),
        ("get_refine_report", pair.get_refine_report, need(REFINED)), ("get_refined_pose", pair.get_refined_pose, need(REFINED)),
        ("get_refined_points", pair.get_refined_points, need(REFINED)), ("get_reprojection_errors", pair.get_reprojection_errors, need(REFINED)),
        ("get_register_report", pair.get_register_report, need(VIEW)), ("get_view_pose", pair.get_view_pose, need(VIEW)),
        ("get_view_errors", pair.get_view_errors, need(VIEW)), ("get_view_counts", pair.get_view_counts, need(VIEW)),
    ]
    for name, fn, want in getters:
        assert code_of(fn) == want, f"{where}: {name} with {sorted(m.have)}"
    r, v = REFINED in m.have, VIEW in m.have
    sizes = {                      # id -> (pointer is not NULL, bytes)
        S.BUF_X0: (True, 12 * ld), S.BUF_X1: (True, 12 * ld), S.BUF_U0: (True, 12 * ld), S.BUF_U1: (True, 12 * ld),
        S.BUF_E: (True, 36), S.BUF_P: (True, 256), S.BUF_PINV: (True, 256), S.BUF_POINTS: (True, 16 * n),
        S.BUF_COUNTS: (m.scored, 4 * m.last_count), S.BUF_MASK: (True, n), S.BUF_KEY: (True, 8),
        S.BUF_ECAND: (m.scored, 36 * m.last_count), S.BUF_PIND: (True, 4),
        S.BUF_REFINED_POSE: (r, 100 if r else 0), S.BUF_REFINED_POINTS: (r, 16 * n if r else 0), S.BUF_REPROJ: (r, 5 * n if r else 0),
        S.BUF_VIEW_POSE: (v, 128 if v else 0), S.BUF_VIEW_COUNTS: (v, 4 * m.view_hyps if v else 0), S.BUF_VIEW_REPROJ: (v, 5 * n if v else 0),
    }
    assert sorted(sizes) == list(range(19))
    for which, (there, nbytes) in sizes.items():
        ptr, got = pair.device_ptr(which)
        assert (ptr is not None, got) == (there, nbytes), f"{where}: buffer id {which} with {sorted(m.have)}"
    assert code_of(lambda: pair.device_ptr(19)) == S.E_INVALID


def test_every_transition_and_every_getter(gpu):
    torch, dev, ctx = gpu
    n, H = 1024, 256
    sc = synth.two_view_scene(n, seed=61, noise_px=0.3, outlier_frac=0.2)
    d_sift = to_dev(torch, dev, sc["sift"])
    rec3, _ = RS.third_view(sc, seed=61, noise_px=0.5)
    d_rec3 = to_dev(torch, dev, rec3)
    d_pts = torch.from_numpy(RS.homogeneous(sc["points3d"])).to(dev)
    vbo = (torch.zeros(4 * n, dtype=torch.float32, device=dev), torch.zeros(4 * n, dtype=torch.float32, device=dev))
    key_t = torch.zeros(1, dtype=torch.int64, device=dev)
    prm = lambda count=H, **kw: S.default_params(n, num_hypotheses=count, seed=61, **kw)
    rp = S.refine_params(max_iterations=5)

    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    m = Model(n)
    step = [0]

    def did(what):
        step[0] += 1
        probe(pair, m, vbo, f"step {step[0]} ({what})")

    def refused(what, calls, code=S.E_STATE):
        """Each call fails with `code` and nothing the getters say changes."""
        for name, fn in calls:
            assert code_of(fn) == code, f"{what}: {name} with {sorted(m.have)}"
            did(f"{what}: {name} refused")

    def estimateE(count=H):
        pair.estimateE(prm(count)); m.scored_shard(count); m.E_finalized()

    needs_E = [("pose_candidates", pair.computePosecandidates), ("pose_chain", pair.pose_chain),
               ("pose_chain correct", lambda: pair.pose_chain(S.POSE_CORRECT)), ("refine", lambda: pair.refine_enqueue(rp))]
    needs_points = [("estimateE", lambda: pair.estimateE(prm())), ("estimateE_pipelined", lambda: pair.estimateE_pipelined(prm())),
                    ("ransac_score", lambda: pair.ransac_score(prm())), ("ransac_score_into", lambda: pair.ransac_score(prm(), key_t)),
                    ("ransac_score_candidates", lambda: pair.ransac_score_candidates(prm(), d_pts)),
                    ("ransac_finalize", lambda: pair.ransac_finalize(prm(), 0)), ("ransac_finalize_key", lambda: pair.ransac_finalize_key(prm(), key_t)),
                    ("ransac_finalize_key_on", lambda: pair.ransac_finalize_key_on(prm(), key_t)),
                    ("register_view", lambda: pair.register_enqueue(d_rec3, S.register_params(points=d_pts)))]

    did("create")
    refused("fresh pair", needs_points + needs_E + [("choosePose", pair.choosePose), ("triangulate", pair.linear_triangulation)])
    pair.fillXU(d_sift); m.points_replaced(); did("fillXU")
    refused("points only", needs_E + [("choosePose", pair.choosePose), ("triangulate", pair.linear_triangulation),
                                      ("register_view without points", lambda: pair.register_enqueue(d_rec3, S.register_params()))])
    refused("bad arguments", [("estimateE", lambda: pair.estimateE(prm(jacobi_sweeps=65))), ("set_points", lambda: pair.set_points(None, None))], S.E_INVALID)
    estimateE(); did("estimateE")
    refused("E only", [("choosePose", pair.choosePose), ("triangulate", pair.linear_triangulation)])
    refused("bad arguments", [("pose_candidates", lambda: pair.computePosecandidates(7)), ("refine", lambda: pair.refine_enqueue(S.refine_params(max_iterations=-1)))],
            S.E_INVALID)
    pair.pose_chain(S.POSE_REFERENCE); m.chain(); did("pose_chain reference")
    estimateE(128); did("estimateE over a pose")
    pair.computePosecandidates(); m.candidates(); did("pose_candidates")
    refused("E and P", [("triangulate", pair.linear_triangulation)])
    pair.choosePose(); m.pose_chosen(); did("choosePose")
    pair.linear_triangulation(); m.have.add(POINTS3D); did("triangulate")
    pair.choosePose(); m.pose_chosen(); did("choosePose over points")
    pair.linear_triangulation(); m.have.add(POINTS3D); did("triangulate")
    pair.computePosecandidates(); m.candidates(); did("pose_candidates over a pose")
    pair.pose_chain(S.POSE_CORRECT); m.chain(); did("pose_chain correct")
    pair.refine_enqueue(rp); m.have.add(REFINED); did("refine")
    refused("bad arguments", [("register_view", lambda: pair.register_enqueue(d_rec3, S.register_params(num_hypotheses=0)))], S.E_INVALID)
    pair.register_enqueue(d_rec3, S.register_params(num_hypotheses=256)); m.have.add(VIEW); m.view_hyps = 256; did("register_view on the refined points")
    estimateE(); did("estimateE over everything")            # refined and view stay: they are stale only after new points
    pair.ransac_score(prm(64)); m.scored_shard(64); did("ransac_score")
    pair.ransac_score(prm(96), key_t); m.scored_shard(96); did("ransac_score_into")
    pair.pose_chain(); m.chain(); did("pose_chain")
    hyp, _ = pair.get_best()
    pair.ransac_finalize(prm(), hyp); m.E_finalized(); did("ransac_finalize")
    pair.ransac_score_candidates(prm(32), torch.from_numpy(np.random.default_rng(0).normal(size=(32, 9)).astype(np.float32)).to(dev))
    m.scored_shard(32); did("ransac_score_candidates")
    refused("supplied candidates", [("ransac_finalize", lambda: pair.ransac_finalize(prm(32), 3))])      # (not a stage: ransac.hip)
    pair.pose_chain(); m.chain(); did("pose_chain")
    for _ in range(3):
        pair.estimateE_pipelined(prm()); m.E_finalized(); m.last_count = 0; m.scored = True
    did("pipelined burst")
    pair.pose_chain(); m.chain(); did("pose_chain")
    pair.ransac_score(prm()); m.scored_shard(H); pair.export_key(key_t)
    pair.ransac_finalize_key(prm(), key_t); m.E_finalized(); did("ransac_finalize_key")
    pair.pose_chain(); m.chain(); did("pose_chain")
    pair.ransac_finalize_key_on(prm(), key_t); m.E_finalized(); did("ransac_finalize_key_on")
    pair.register_enqueue(d_rec3, S.register_params(points=d_pts, num_hypotheses=512)); m.view_hyps = 512; did("register_view, more hypotheses")
    X0, X1 = pair.get_XU(S.BUF_X0), pair.get_XU(S.BUF_X1)
    pair.set_points(to_dev(torch, dev, X0), to_dev(torch, dev, X1)); m.points_replaced(); did("set_points")
    estimateE(); pair.pose_chain(); m.chain(); did("estimateE + pose_chain on set points")
    pair.refine_enqueue(rp); m.have.add(REFINED)
    pair.register_enqueue(d_rec3, S.register_params()); m.have.add(VIEW); m.view_hyps = 4096; did("refine + register_view")
    assert m.have == ALL
    refused("bad arguments", [("reset", lambda: pair.reset(n + 1))], S.E_INVALID)
    pair.reset(512); m.reset(512); did("reset")
    refused("after reset", needs_points + needs_E)
    pair.fillXU(d_sift); m.points_replaced(); did("fillXU again")
    pair.estimateE(S.default_params(512, num_hypotheses=64)); m.scored_shard(64); m.E_finalized(); did("estimateE")
    pair.pose_chain(); m.chain(); did("pose_chain")
    pair.fillXU(d_sift); m.points_replaced(); did("fillXU over everything")
    pair.close()
