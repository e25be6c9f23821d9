"""sfm_process_pairs: the batched path against the per-pair path (SFM_PAIRS_UNBATCHED) on a list that has what the dino lists
lack -- unusable pairs in the middle, first / stride under the batch, a first view that comes back later in the list, a run
broken by a different n, and a second view that the tail quirk trims to nothing.  The per-pair path is the reference (itself
pinned to the oracle chain by tests/test_gpu_dino.py): records, status and every byte of every view's device records must be
the same after either path.  No tolerance is involved."""
import numpy as np
import pytest

import cuda_sfm_amd as S
from cuda_sfm_amd import synth
from helpers import same_bits, to_dev

pytestmark = pytest.mark.gpu

H = 64
SIZES = {"A": 640, "B": 577, "C": 500, "D": 333, "T": 20}
# (first view, n1 or None = all of it, second view, n2 or None)
PAIRS = [("A", None, "B", None), ("A", None, "C", None), ("A", None, "D", None),       # a run of three on one first view
         ("A", SIZES["A"] - 40, "B", None),                                            # same first view, other n: breaks the run
         ("B", None, "C", None),
         ("B", 5, "C", None),                                                          # unusable, in the middle
         ("C", None, "T", None),                                                       # n2 = 20: nothing left under the tail quirk
         ("C", None, "D", None), ("D", None, "A", None), ("D", None, "B", None),
         ("B", None, "A", None), ("C", None, "A", None),
         ("D", None, "C", 0),                                                          # unusable
         ("A", None, "B", None),                                                       # back to an earlier first view
         ("T", None, "A", None), ("B", None, "D", None), ("D", None, "C", None), ("C", None, "B", None)]
UNUSABLE = (5, 12)


@pytest.fixture(scope="module")
def views():
    """Five views of one descriptor set (different noise each), random keypoint positions."""
    n = 700
    d1 = synth.descriptors(n, 11, sparsity=0.5)[0]
    desc = {"A": d1[:SIZES["A"]], "T": d1[100:100 + SIZES["T"]]}
    for name, noise in (("B", 0.05), ("C", 0.08), ("D", 0.03)):
        desc[name] = synth.descriptors(n, 11, noise=noise, sparsity=0.5)[1][:SIZES[name]]
    return {name: synth.sift_records(np.ascontiguousarray(desc[name]), seed=300 + i) for i, name in enumerate("ABCDT")}


def run_path(torch, dev, ctx, views, K, Kinv, rank, world):
    """Fresh copies of the views (the matcher writes the first view's fields), one call; (records, status, views afterwards)."""
    d = {name: to_dev(torch, dev, v) for name, v in views.items()}
    descs = [(d[a], SIZES[a] if n1 is None else n1, d[b], SIZES[b] if n2 is None else n2) for (a, n1, b, n2) in PAIRS]
    rec, status = S.process_pairs_local(ctx, descs, K, Kinv, rank=rank, world=world, num_hypotheses=H)
    torch.cuda.synchronize()
    return rec.copy(), status.copy(), {name: t.cpu().numpy().copy() for name, t in d.items()}, ctx.last_pairs_batched()


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("quirks", [0, S.QUIRK_MATCH_TAIL | S.QUIRK_MATCH_AMBIGUITY])
def test_batched_path_equals_per_pair_path(gpu, views, monkeypatch, quirks, rank, world):
    torch, dev, _ = gpu
    assert len(PAIRS) == 18
    owned = list(range(rank, len(PAIRS), world))
    assert sum(i not in UNUSABLE for i in owned) >= 8                    # four lanes, also for rank 1 of 2
    K, Kinv = synth.camera()
    ctx = S.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        ctx.set_quirks(quirks)
        monkeypatch.delenv("SFM_PAIRS_UNBATCHED", raising=False)
        rec_b, st_b, views_b, batched = run_path(torch, dev, ctx, views, K, Kinv, rank, world)
        assert batched
        monkeypatch.setenv("SFM_PAIRS_UNBATCHED", "1")
        rec_p, st_p, views_p, batched = run_path(torch, dev, ctx, views, K, Kinv, rank, world)
        assert not batched
    finally:
        ctx.close()
    assert rec_b.shape == rec_p.shape == (len(owned), 28)
    print("status", st_b.tolist(), st_p.tolist())
    for slot, i in enumerate(owned):
        assert same_bits(rec_b[slot], rec_p[slot]), f"pair {i} (slot {slot}): records differ"
        if i in UNUSABLE:
            assert st_b[slot] == S.E_INVALID and np.all(rec_b[slot] == -1.0), f"pair {i} (slot {slot})"
        else:
            assert st_b[slot] in (S.OK, S.E_SINGULAR) and not np.all(rec_b[slot] == -1.0), f"pair {i} (slot {slot})"
    assert np.array_equal(st_b, st_p)
    for name in views:
        diff = np.flatnonzero((views_b[name] != views_p[name]).any(axis=1))
        assert diff.size == 0, f"view {name}: device records {diff[:8].tolist()} differ between the two paths"
    # the call did write match fields: the check above is not comparing two untouched uploads
    a = views_b["A"].reshape(-1).view(synth.SIFT_DTYPE)
    assert (a["match"] >= 0).any()
