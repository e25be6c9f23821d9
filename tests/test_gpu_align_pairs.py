"""GPU: sfm_align_pairs (many links in one batched call) against sfm_align_pair -- every output byte for byte wherever a link
stands in the list, the per-hypothesis counts under the batched launch's other share count, a pair that is b of one link and a
of the next, and the refusals that name links[i] with nothing written."""
import numpy as np
import pytest

import cuda_sfm_amd as S
from helpers import to_dev
import align_scene as AS
from test_gpu_align import chain, filled, first_candidates, read_back, u8, untouched

pytestmark = pytest.mark.gpu
# (records, seed, candidates of link 0, of link 1): three scenes of four views, so pair 1 of each is b of one link and a of the next
SCENES = [(2048, 31, 1024, 300), (384, 32, 257, 64), (128, 33, 8, 2)]


@pytest.fixture(scope="module")
def links(gpu):
    """The six links on the device: (a, b, index tensor, candidates)."""
    torch, dev, ctx = gpu
    out, made_all = [], []
    for n, seed, m0, m1 in SCENES:
        sc = AS.build(n, seed)
        made, reports = chain(gpu, sc, good_masks=True)
        assert all(r["status"] != S.REFINE_DEGENERATE for r in reports)
        state = [read_back(p) for p in made]
        for v, m in enumerate((m0, m1)):
            index = first_candidates(state[v], state[v + 1], sc["links"][v]["index"], m)
            out.append((made[v], made[v + 1], to_dev(torch, dev, index), m))
        made_all += made
    yield out
    for p in made_all:
        p.close()


def as_bytes(res):
    return tuple(u8(a).tobytes() for a in res[:4]) + (res[4],)


@pytest.mark.parametrize("order", ["listed", "permuted"])
def test_batched_call_equals_the_single_calls(gpu, links, order):
    torch, dev, ctx = gpu
    use = links if order == "listed" else [links[k] for k in (3, 5, 0, 4, 2, 1)]
    single = [a.align_to(b, idx) for a, b, idx, _ in use]
    for (a, b, idx, m), r in zip(use, single):
        assert r[4]["num_candidates"] == m and (r[4]["status"] == S.REFINE_DEGENERATE) == (m < 6), (m, r[4])
    params = S.align_params()
    outs = [filled(torch, dev, a.num_points, params.num_hypotheses) for a, _, _, _ in use]
    S.align_pairs_enqueue([l[0] for l in use], [l[1] for l in use], [l[2] for l in use], params, outs)
    ctx.synchronize()
    for (a, b, idx, m), want, got in zip(use, single, outs):
        for name, x, y in zip(("sim", "inlier", "err", "counts"), want, got):
            assert np.array_equal(u8(x), u8(y.cpu().numpy())), (order, m, name)
        r = S.AlignReport.from_buffer_copy(got[4].cpu().numpy().tobytes())
        assert {f: getattr(r, f) for f, _ in S.AlignReport._fields_} == want[4], (order, m)
    again = S.align_pairs([l[0] for l in use], [l[1] for l in use], [l[2] for l in use])
    assert [as_bytes(r) for r in again] == [as_bytes(r) for r in single]
    # other hypothesis counts, so other share counts in both launches: the counts still agree
    few = S.align_pairs([l[0] for l in use], [l[1] for l in use], [l[2] for l in use], num_hypotheses=256, max_iterations=0)
    for (a, b, idx, m), got in zip(use, few):
        assert as_bytes(a.align_to(b, idx, num_hypotheses=256, max_iterations=0)) == as_bytes(got), m


def test_refusals_name_the_link_and_write_nothing(gpu, links):
    torch, dev, ctx = gpu
    params = S.align_params()
    A, B, I = [l[0] for l in links], [l[1] for l in links], [l[2] for l in links]
    sc = AS.build(64, 5)
    bare = S.ImagePair(ctx, sc["K"], sc["Kinv"], 2, 64)
    bare.fillXU(to_dev(torch, dev, sc["pairs"][0]["sift"]))
    bare_index = to_dev(torch, dev, np.full(64, -1, np.int32))
    share_out = lambda o: o[:2] + [o[2][:2] + (o[0][2],) + o[2][3:]] + o[3:]               # link 2's errors in link 0's (larger) array
    share_in = lambda o: o[:2] + [(o[2][0], o[2][1], I[0]) + o[2][3:]] + o[3:]               # link 2's errors on link 0's index
    index0 = I[0].cpu().numpy().copy()
    cases = [(A[:2] + [bare] + A[2:], B[:2] + [B[0]] + B[2:], I[:2] + [bare_index] + I[2:], S.E_STATE, "links[2]: a:", None),
             (A[:2] + [A[5]] + A[2:], B[:2] + [bare] + B[2:], I[:2] + [I[5]] + I[2:], S.E_INVALID, "listed twice as a", None),
             (A[:2] + [A[5]] + A[2:5], B[:2] + [bare] + B[2:5], I[:2] + [I[5]] + I[2:5], S.E_STATE, "links[2]: b:", None),
             (A, B, I, S.E_INVALID, "overlaps a buffer of links[0]", share_out),
             (A, B, I, S.E_INVALID, "overlaps a buffer of links[0]", share_in),
             (A[:2] + [A[2]] + A[3:], B[:2] + [A[2]] + B[3:], I, S.E_INVALID, "links[2]: a and b are the same pair", None)]
    for as_, bs, idx, code, text, tweak in cases:
        outs = [filled(torch, dev, a.num_points, params.num_hypotheses) for a in as_]
        if tweak:
            outs = tweak(outs)
        with pytest.raises(S.SfmError) as e:
            S.align_pairs_enqueue(as_, bs, idx, params, outs)
        assert e.value.code == code and text in str(e.value), str(e.value)
        if "listed twice" in text:
            assert "links[6]" in str(e.value) or "links[2]" in str(e.value), str(e.value)
        else:
            assert "links[2]" in str(e.value), str(e.value)
        ctx.synchronize()
        assert all(untouched(o) for k, o in enumerate(outs) if not (tweak is share_in and k == 2))           # (that one holds an input)
        assert np.array_equal(I[0].cpu().numpy(), index0)
    bare.close()
