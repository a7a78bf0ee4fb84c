"""ops.rank_segments / ops.rank_arena on the CPU (the forms a CPU servable's
step uses) against the numpy reference order of tests/rank_cases.py, and the
arena header's n_ranked field."""
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

F = 43
SV, SI = -7.5, -99  # sentinels the outputs are pre-filled with


def test_reference_order_is_sort_scores_order():
    rng = np.random.default_rng(1)
    for n in (1, 2, 63, 64, 65, 511, 512, 513, 1500):
        v = rc.segment_scores(n, rng)
        for desc in (False, True):
            s, p = ops.sort_scores(torch.from_numpy(v), desc)
            want = rc.ref_order(v, desc)
            assert np.array_equal(p.numpy(), want)
            assert np.array_equal(rc.bits(s), rc.bits(v[want]))


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("k", [-1, 1, 10])
def test_rank_segments_cpu(descending, k):
    scores, offsets, segs = rc.make_buffer(rc.CPU_LENGTHS, seed=3)
    vals = torch.full((scores.size,), SV)
    idx = torch.full((scores.size,), SI, dtype=torch.int64)
    rv, ri = ops.rank_segments(torch.from_numpy(scores), torch.from_numpy(offsets), descending, k, out=(vals, idx))
    assert rv is vals and ri is idx
    want_v, want_i = rc.expected(scores, segs, descending, k, SV, SI)
    assert np.array_equal(rc.bits(vals), rc.bits(want_v))
    assert np.array_equal(idx.numpy(), want_i)
    # fresh outputs: 0 / -1 outside the segments
    fv, fi = ops.rank_segments(torch.from_numpy(scores), offsets.tolist(), descending, k)
    want_v, want_i = rc.expected(scores, segs, descending, k, 0.0, -1)
    assert np.array_equal(rc.bits(fv), rc.bits(want_v)) and np.array_equal(fi.numpy(), want_i)


def test_rank_segments_argument_errors_cpu():
    s = torch.zeros(100)
    with pytest.raises(ValueError):
        ops.rank_segments(s, [0, 50, 40])
    with pytest.raises(ValueError):
        ops.rank_segments(s, [0, 50, 101])
    with pytest.raises(ValueError):
        ops.rank_segments(s, [-1, 50])


def _req(rows, g):
    ids = torch.randint(0, 1 << 40, (rows, F), generator=g)
    wts = torch.rand(rows, F, generator=g)
    return native().encode_predict_request("DCN", "serving_default", None, [("feat_ids", ids), ("feat_wts", wts)],
                                           True)


def test_arena_header_n_ranked_and_rank_arena_cpu():
    g = torch.Generator().manual_seed(4)
    rows = (1, 37, 512, 300)
    A = ArenaLayout(F, 1024)
    reqs = [_req(r, g) for r in rows]
    plain, asked = A.alloc(), A.alloc()
    ab0 = A.build(plain, A.place(plain, reqs))
    ab = A.build(asked, A.place(asked, reqs), n_ranked=2)
    assert not any(ab.errors) and ab.total_rows == sum(rows)
    # the field is the only difference, and it is 0 when nobody asks
    assert int(plain[44:48].view(torch.int32)) == 0 and int(asked[44:48].view(torch.int32)) == 2
    diff = (plain != asked).nonzero().flatten().tolist()
    assert diff == [44] and ab0.used_bytes == ab.used_bytes
    with pytest.raises(ValueError):
        A.build(asked, A.place(asked, reqs), n_ranked=5)

    rng = np.random.default_rng(9)
    scores = np.concatenate([rc.segment_scores(r, rng) for r in rows] + [rng.random(1024 - sum(rows), dtype=np.float32)])
    segs = [(o, o + r) for o, r in zip(ab.offsets, ab.rows)]
    for arena, touched in ((asked, True), (plain, False)):
        vals = torch.full((1024,), SV)
        idx = torch.full((1024,), SI, dtype=torch.int64)
        ops.rank_arena(arena, torch.from_numpy(scores), vals, idx)
        want_v, want_i = rc.expected(scores, segs if touched else [], False, -1, SV, SI)
        assert np.array_equal(rc.bits(vals), rc.bits(want_v))
        assert np.array_equal(idx.numpy(), want_i)
