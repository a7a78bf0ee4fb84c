"""Request arenas for the exact tests (test_kernels_exact_gpu.py,
test_gather_exact_gpu.py): requests with integer weights placed in an arena,
and the ids / weights its rows decode to."""
import torch

import exact_cases as xc


def arena_case(F, sizes, B, seed, rows=None):
    """Requests with integer weights (raw and packed-varint encodings) placed
    in a request arena; returns the arena and the ids / weights of its B rows
    (rows past the requests' are padding: id 0, weight 0). ``rows`` = (ids,
    wts): the requests carry these rows in order instead of random ones."""
    from distributed_tf_serving_amd.ops import native
    from distributed_tf_serving_amd.serving.arena import ArenaLayout

    g = torch.Generator().manual_seed(seed)
    A = ArenaLayout(F, 256)
    ar = A.alloc()
    reqs, ids_all, wts_all = [], [], []
    at = 0
    for n, raw in sizes:
        if rows is not None:
            ids, wts = rows[0][at:at + n].contiguous(), rows[1][at:at + n].contiguous().float()
            at += n
        else:
            ids = torch.randint(-(1 << 62), 1 << 62, (n, F), generator=g)
            ids.view(-1)[:4] = torch.tensor(xc.EDGE_IDS, dtype=torch.int64)
            wts = torch.randint(0, 3, (n, F), generator=g).float()
        reqs.append(native().encode_predict_request("DCN", "serving_default", None,
                                                    [("feat_ids", ids), ("feat_wts", wts)], raw))
        ids_all.append(ids)
        wts_all.append(wts)
    ab = A.build(ar, A.place(ar, reqs))
    total = sum(n for n, _ in sizes)
    assert not any(ab.errors) and ab.total_rows == total and ab.n_gpu_varint >= 1 and total < B
    ids_all.append(torch.zeros(B - total, F, dtype=torch.int64))
    wts_all.append(torch.zeros(B - total, F))
    return A, ar, torch.cat(ids_all), torch.cat(wts_all)
