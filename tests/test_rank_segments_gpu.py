"""The segmented rank kernel (csrc/kernels/rank.hip) on the GPU: one launch
over segments of every length at which the kernel takes another path, against
the numpy reference order of tests/rank_cases.py and against ops.sort_scores,
bit for bit; top-k prefixes; argument errors; and rank_arena over a device
request arena."""
import os
import sys

import numpy as np
import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.ops import native
from distributed_tf_serving_amd.serving.arena import ArenaLayout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
F = 43
SV, SI = -7.5, -99  # sentinels the outputs are pre-filled with


@pytest.fixture(scope="module")
def buf():
    """The score buffer of every rank_segments test here (never written)."""
    scores, offsets, segs = rc.make_buffer(rc.GPU_LENGTHS, seed=7)
    return scores, offsets, segs


def _run(cuda, scores, offsets, descending, k):
    vals = torch.full((scores.size,), SV, device=cuda)
    idx = torch.full((scores.size,), SI, dtype=torch.int64, device=cuda)
    s = torch.from_numpy(scores).to(cuda)
    rv, ri = ops.rank_segments(s, torch.from_numpy(offsets), descending, k, out=(vals, idx))
    assert rv is vals and ri is idx
    assert np.array_equal(rc.bits(s), rc.bits(scores))  # the scores are only read
    return vals.cpu(), idx.cpu()


@pytest.mark.parametrize("descending", [False, True])
def test_every_length_in_one_launch_matches_reference(cuda, buf, descending):
    scores, offsets, segs = buf
    vals, idx = _run(cuda, scores, offsets, descending, -1)
    want_v, want_i = rc.expected(scores, segs, descending, -1, SV, SI)
    for a, b in segs:  # per segment first, for a readable failure
        assert np.array_equal(idx[a:b].numpy(), want_i[a:b]), f"permutation of the {b - a}-score segment"
        assert np.array_equal(rc.bits(vals[a:b]), rc.bits(want_v[a:b])), f"values of the {b - a}-score segment"
    # whole buffers: the scores in front of the first and behind the last
    # segment kept their sentinels
    assert np.array_equal(idx.numpy(), want_i) and np.array_equal(rc.bits(vals), rc.bits(want_v))
    # ... and it is ops.sort_scores per segment where that kernel applies
    for a, b in segs:
        if 0 < b - a <= 8192:
            s, p = ops.sort_scores(torch.from_numpy(scores[a:b]).to(cuda), descending)
            assert torch.equal(p.cpu(), idx[a:b])
            assert np.array_equal(rc.bits(s), rc.bits(vals[a:b]))


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("k", [1, 10, 16384])  # 16384: k = n of the longest segment, everything of the others
def test_top_k_prefix_and_fill(cuda, buf, descending, k):
    scores, offsets, segs = buf
    vals, idx = _run(cuda, scores, offsets, descending, k)
    want_v, want_i = rc.expected(scores, segs, descending, k, SV, SI)
    assert np.array_equal(idx.numpy(), want_i) and np.array_equal(rc.bits(vals), rc.bits(want_v))


def test_small_classes_and_fresh_outputs(cuda):
    """Launches whose longest segment selects the 1024- and the 4096-slot
    kernels (the big buffer always selects the 16384-slot one), with outputs
    the op allocates: 0 / -1 outside the segments. k = n is k = -1."""
    for lengths in ((1, 65, 0, 1024, 513, 2), (1025, 64, 4096, 1500, 4095)):
        scores, offsets, segs = rc.make_buffer(lengths, seed=len(lengths))
        for descending in (False, True):
            v, i = ops.rank_segments(torch.from_numpy(scores).to(cuda), offsets.tolist(), descending, max(lengths))
            want_v, want_i = rc.expected(scores, segs, descending, -1, 0.0, -1)
            assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(rc.bits(v), rc.bits(want_v))


def test_argument_errors_raise_before_any_launch(cuda):
    s = torch.zeros(20000, device=cuda)
    vals = torch.full((20000,), SV, device=cuda)
    idx = torch.full((20000,), SI, dtype=torch.int64, device=cuda)
    for offsets in ([0, 16385], [0, 50, 40], [0, 50, 20001]):
        with pytest.raises(ValueError):
            ops.rank_segments(s, offsets, out=(vals, idx))
        with pytest.raises(ValueError):  # the binding checks for itself too
            ops.hip().rank_segments(s, torch.tensor(offsets), False, -1, vals, idx)
    torch.cuda.synchronize()
    assert bool((vals == SV).all()) and bool((idx == SI).all())


def _req(rows, g):
    ids = torch.randint(0, 1 << 40, (rows, F), generator=g)
    wts = torch.rand(rows, F, generator=g)
    return native().encode_predict_request("DCN", "serving_default", None, [("feat_ids", ids), ("feat_wts", wts)],
                                           True)


@pytest.mark.parametrize("pinned", [False, True])
def test_rank_arena_on_a_device_arena(cuda, pinned):
    """Requests of 1, 37, 512 and 1500 rows in an arena built by the project's
    own builder: ranked per request when the header says somebody asked,
    untouched outputs when it says nobody did. pinned: scores and outputs in
    pinned host memory, as the served step has them."""
    g = torch.Generator().manual_seed(4)
    rows = (1, 37, 512, 1500)
    B = 2048 + 512  # the 4096-slot kernel; a second size class than the big buffer's
    A = ArenaLayout(F, B)
    reqs = [_req(r, g) for r in rows]
    rng = np.random.default_rng(9)
    scores = np.concatenate([rc.segment_scores(r, rng) for r in rows] + [rng.random(B - sum(rows), dtype=np.float32)])

    def place(t):
        return t.pin_memory() if pinned else t.to(cuda)

    for n_ranked in (2, 0):
        host = A.alloc()
        ab = A.build(host, A.place(host, reqs), n_ranked=n_ranked)
        assert not any(ab.errors) and ab.total_rows == sum(rows)
        segs = [(o, o + r) for o, r in zip(ab.offsets, ab.rows)]
        vals, idx = place(torch.full((B,), SV)), place(torch.full((B,), SI, dtype=torch.int64))
        ops.rank_arena(host.to(cuda), place(torch.from_numpy(scores)), vals, idx)
        torch.cuda.synchronize()
        want_v, want_i = rc.expected(scores, segs if n_ranked else [], False, -1, SV, SI)
        assert np.array_equal(idx.cpu().numpy(), want_i)
        assert np.array_equal(rc.bits(vals), rc.bits(want_v))
