"""GPU: sfm_pair_fundamentals against the single calls (sfm_pair_fundamental) and the host build
(tests/hostcheck/libmatchguidedcheck.so): both `refined` values bit for bit, more pairs than one block holds, the contract with the
table compared before and after every refusal."""
import ctypes as C

import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
import match_guided_scene as MS
from helpers import to_dev

pytestmark = pytest.mark.gpu


def make_pair(gpu, ctx, n, seed, hyps):
    torch, dev, _ = gpu
    sc = synth.two_view_scene(n, seed=seed)
    d_sift = to_dev(torch, dev, sc["sift"])
    pair = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, n)
    pair.fillXU(d_sift)
    pair.estimateE(S.default_params(n, num_hypotheses=hyps))
    return pair, d_sift, sc


def handles(pairs):
    return (C.c_void_p * len(pairs))(*[p._h.value if p is not None else None for p in pairs])


def test_three_pairs_equal_the_single_calls_and_the_host_build(gpu):
    torch, dev, ctx = gpu
    made = [make_pair(gpu, ctx, 256, 700 + k, 1024) for k in range(3)]
    pairs = [m[0] for m in made]
    S.refine_pairs(pairs, max_iterations=10)
    for refined in (False, True):
        got = S.pair_fundamentals(pairs, refined=refined).cpu().numpy()
        assert got.shape == (3, 9) and got.dtype == np.float32
        for k, (pair, _, sc) in enumerate(made):
            single = pair.fundamental(refined=refined).cpu().numpy()
            assert np.array_equal(got[k].view(np.uint32), single.view(np.uint32)), (refined, k)
            E = pair.get_refined_pose()[1] if refined else pair.get_E()
            assert np.array_equal(got[k].view(np.uint32), MS.host_fundamental(E, sc["Kinv"], 1 if refined else 0).view(np.uint32)), (refined, k)
            assert abs(float(np.linalg.norm(got[k].astype(np.float64))) - 1.0) < 1e-6
        assert len({got[k].tobytes() for k in range(3)}) == 3                # every pair its own F
    # a list in another order gives the rows in that order, into a caller's table
    table = torch.full((3, 9), -3.0, dtype=torch.float32, device=dev)
    back = S.pair_fundamentals(pairs[::-1], refined=True, out=table).cpu().numpy()
    assert np.array_equal(back[::-1], got)
    for p in pairs:
        p.close()


def test_more_pairs_than_one_block(gpu):
    """66 pairs: lanes of two blocks, the last block two lanes full"""
    torch, dev, ctx = gpu
    made = [make_pair(gpu, ctx, 128, 800 + k, 256) for k in range(66)]
    pairs = [m[0] for m in made]
    table = torch.full((67, 9), -3.0, dtype=torch.float32, device=dev)
    S.pair_fundamentals(pairs, refined=False, out=table)
    each = torch.stack([p.fundamental(refined=False) for p in pairs])
    torch.cuda.synchronize()
    assert torch.equal(table[:66], each)
    assert torch.all(table[66] == -3.0)                                     # nothing past the last pair's nine floats
    for p in pairs:
        p.close()


def test_contract(gpu):
    torch, dev, ctx = gpu
    L = S.lib()
    made = [make_pair(gpu, ctx, 256, 710 + k, 1024) for k in range(4)]
    pairs = [m[0] for m in made]
    S.refine_pairs(pairs[:3], max_iterations=5)
    other = S.Context(0, torch.cuda.current_stream().cuda_stream)
    foreign = make_pair(gpu, other, 256, 720, 1024)[0]
    table = torch.full((4, 9), -3.0, dtype=torch.float32, device=dev)
    t = table.data_ptr()
    refusals = [
        (None, 3, 0, t, S.E_INVALID), (handles(pairs), 3, 0, None, S.E_INVALID),                         # null arguments
        (handles(pairs), -1, 0, t, S.E_INVALID),                                                         # num_pairs < 0
        (handles(pairs), 3, 2, t, S.E_INVALID), (handles(pairs), 3, -1, t, S.E_INVALID),                 # refined outside {0, 1}
        (handles([pairs[0], None]), 2, 0, t, S.E_INVALID),                                               # a null pair
        (handles([pairs[0], foreign]), 2, 0, t, S.E_INVALID),                                            # pairs of different contexts
        (handles([pairs[0], pairs[1], pairs[0]]), 3, 0, t, S.E_INVALID),                                 # a pair named twice
        (handles(pairs), 4, 1, t, S.E_STATE),                                                            # pairs[3] has no refinement
    ]
    fresh = S.ImagePair(ctx, made[0][2]["K"], made[0][2]["Kinv"], 2, 256)
    fresh.fillXU(made[0][1])
    refusals.append((handles([pairs[0], fresh]), 2, 0, t, S.E_STATE))                                    # a pair without E
    for i, (h, n, refined, out, code) in enumerate(refusals):
        assert L.sfm_pair_fundamentals(h, n, refined, out) == code, i
        torch.cuda.synchronize()
        assert torch.all(table == -3.0), i
    assert L.sfm_pair_fundamentals(handles(pairs), 0, 0, t) == S.OK                                      # no pair: a no-op
    torch.cuda.synchronize()
    assert torch.all(table == -3.0)
    with pytest.raises(S.SfmError) as e:
        S.pair_fundamentals(pairs, refined=True)
    assert e.value.code == S.E_STATE
    # the pairs' own results stay as they were
    E0, pose0 = pairs[0].get_E(), pairs[0].get_refined_pose()[1]
    got = S.pair_fundamentals(pairs, refined=False, out=table).cpu().numpy()
    assert np.array_equal(got[3], pairs[3].fundamental(refined=False).cpu().numpy())
    assert np.array_equal(pairs[0].get_E(), E0) and np.array_equal(pairs[0].get_refined_pose()[1], pose0)
    for p in pairs + [foreign, fresh]:
        p.close()
