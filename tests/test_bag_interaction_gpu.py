"""csrc/kernels/interaction_bag.hip: the multi-hot bag pooling inside the dot
interaction against the fp64 reference of tests/test_bag_interaction_cpu.py,
the multi-hot DLRM served from the arena, and the launcher limits."""
import copy
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig, ServingConfig
from distributed_tf_serving_amd.models import build_model
from distributed_tf_serving_amd.ops import native
from distributed_tf_serving_amd.serving.arena import ArenaLayout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bag_interaction_cpu import bag_interaction_ref, small_integer_case  # noqa: E402

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _request(ids, wts, raw=True):
    t = [("feat_ids", ids.contiguous()), ("feat_wts", wts.contiguous())]
    return native().encode_predict_request("DCN", "serving_default", None, t, raw)


def _arena(ids, wts, cuda, max_rows=64):
    A = ArenaLayout(ids.shape[1], max_rows)
    ar = A.alloc()
    A.build(ar, A.place(ar, [_request(ids, wts)]))
    dev = ar.to(cuda)
    A.decode_varints(dev)
    return ops.ArenaRows(dev, ids.shape[0], ids.shape[1])


# every T, hot (2, 3 = U + 1 on bf16 rows, 5 = U + 1 on code rows, 16), B, id source and weight form, both stores
@pytest.mark.parametrize("T,hot,B,src,weighted", [
    (1, 2, 1, "int32", True), (1, 16, 5, "arena", True), (15, 3, 5, "int64_slice", False),
    (15, 5, 1, "arena", True), (31, 2, 5, "int64_slice", True), (31, 3, 1, "int32", False),
    (31, 5, 5, "int32", True), (31, 16, 5, "int64_slice", True), (31, 16, 1, "arena", True)])
@pytest.mark.parametrize("fp8", [False, True])
def test_bag_interaction_exact(cuda, T, hot, B, src, weighted, fp8):
    """Small integers: pooled values and dots are exact in fp32 in any order, so
    the kernel must equal bf16(fp64 reference) element for element; the fp8
    kernel bit for bit the bf16 kernel on the same (dequantised) rows."""
    rows = 97
    dense, table, ids, wts, mod, off = small_integer_case(T, hot, B, rows, 31 * T + hot, weighted)
    if src == "int32":
        ids = ids.to(torch.int32)  # the low words: both signs
    want = bag_interaction_ref(dense, table, ids, wts, hot, rows, ops.interaction_cols(T))
    dc, tc, mc, oc = (t.to(cuda) for t in (dense, table, mod, off))
    wc = None if wts is None else wts.to(cuda)
    if src == "arena":
        ic, wc = _arena(ids, wts, cuda), None
    elif src == "int32":
        ic = ids.to(cuda)
    else:  # int64 rows as a column slice of a wider tensor, the weights likewise
        ic = torch.cat([torch.full((B, 3), 7), ids, torch.full((B, 2), -7)], 1).to(cuda)[:, 3:3 + T * hot]
        wc = None if wc is None else torch.cat([wc.new_full((B, 5), 9.0), wc], 1)[:, 5:]
    got = ops.dot_interaction_bag(dc, tc, ic, wc, hot, mc, oc)
    if fp8:
        q = table.to(F8)
        assert torch.equal(q.float(), table.float())
        got16, got = got, ops.dot_interaction_bag_fp8(dc, q.to(cuda), torch.ones(T, device=cuda), ic, wc, hot, mc, oc)
        assert torch.equal(got.cpu().view(torch.int16), got16.cpu().view(torch.int16))
    got = got.cpu()
    used = 64 + (T + 1) * T // 2
    assert got.dtype == torch.bfloat16 and torch.equal(got[:, :64], dense) and (got[:, used:] == 0).all()
    assert torch.equal(got, want)


def test_bag_interaction_random_values_within_derived_bound(cuda):
    """Two bf16 roundings (pooled value, product), 2^-9 relative each: the error
    of entry (i, j) is at most 2^-7 sum_k A_ik A_jk + 2^-9 |Z_ij| with A_t =
    sum_j |w_j row_j| (A_0 = |dense|); asserted at 2^-6 sum_k A_ik A_jk."""
    T, hot, B, rows = 30, 4, 64, 1000
    g = torch.Generator().manual_seed(4)
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16)
    table = ((torch.rand(T * rows, 64, generator=g) - 0.5) / 4).to(torch.bfloat16)
    ids = torch.randint(0, 1 << 40, (B, T * hot), generator=g)
    wts = torch.rand(B, T * hot, generator=g)
    mod = torch.full((T,), rows, dtype=torch.int64)
    off = torch.arange(T, dtype=torch.int64) * rows
    got = ops.dot_interaction_bag(*(t.to(cuda) for t in (dense, table, ids, wts)), hot, mod.to(cuda), off.to(cuda))
    vals = table.double()[torch.arange(T).repeat_interleave(hot) * rows + ids % rows] * wts.double().unsqueeze(-1)
    X = torch.cat([dense.double().unsqueeze(1), vals.view(B, T, hot, 64).sum(2)], 1)
    A = torch.cat([dense.double().abs().unsqueeze(1), vals.abs().view(B, T, hot, 64).sum(2)], 1)
    li, lj = torch.tril_indices(T + 1, T + 1, offset=-1)
    ref = (X @ X.transpose(1, 2))[:, li, lj]
    bound = 2.0 ** -6 * (A @ A.transpose(1, 2))[:, li, lj]
    err = (got.cpu().double()[:, 64:64 + li.numel()] - ref).abs()
    ratio = (err / bound).max().item()
    print(f"bag interaction: largest err / bound {ratio:.4f}")
    assert ratio <= 1.0, f"largest err / bound = {ratio:.4f}"


@pytest.mark.parametrize("table_dtype", ["bf16", "fp8"])
def test_multi_hot_dlrm_served_from_the_arena(cuda, table_dtype):
    """forward_arena == the unfused path == the CPU model (2e-2, the model's own
    bound against its CPU twin), and a request through the live server."""
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.fanout import FanoutEngine
    from distributed_tf_serving_amd.serving.executor import ShardExecutor
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.packing import PackedLayout
    from distributed_tf_serving_amd.wire import schema as pb
    from distributed_tf_serving_amd.wire import tensor as wt

    cfg = ModelConfig(family="dlrm", num_fields=13 + 15 * 2, num_dense=13, table_rows=50_021, embed_dim=64,
                      multi_hot=2, bottom_mlp=(512, 256, 64), mlp_dims=(1024, 512, 256), table_dtype=table_dtype)
    cm = build_model(cfg, "cpu")
    gm = copy.deepcopy(cm).to(cuda)
    assert gm.supports_arena
    F, B = cfg.num_fields, 512
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 1 << 40, (300, F), generator=g)
    wts = torch.rand(300, F, generator=g)
    A = ArenaLayout(F, B)
    ar = A.alloc()
    A.build(ar, A.place(ar, [_request(ids[:17], wts[:17]), _request(ids[17:], wts[17:], raw=False)]))
    dev = ar.to(cuda)
    A.decode_varints(dev)
    got = gm.forward_arena(dev, B).float().cpu()[:300]
    fused = gm(ids.to(cuda), wts.to(cuda)).float().cpu()
    gm.use_bag_interaction = False
    unfused = gm(ids.to(cuda), wts.to(cuda)).float().cpu()
    del gm.use_bag_interaction
    assert (got - fused).abs().max().item() <= 1e-6  # the arena-fed step against the same kernels on tensors
    assert (got - unfused).abs().max().item() < 2e-2
    assert (got - cm(ids, wts).float()).abs().max().item() < 2e-2

    ex = ShardExecutor(gm, PackedLayout(F), [B], cuda, slots=2)
    eng = FanoutEngine(ex, DistContext(device=cuda), mode="local", ingest="arena", arena=ArenaLayout(F, max_rows=B))
    eng.prepare(B)
    sc = ServingConfig(max_batch_rows=B, allowed_batch_sizes=(B,), batch_timeout_us=100)
    live = LiveScheduler(eng, sc, buckets=[B], depth=2)
    try:
        resp = pb.PredictResponse.FromString(live.predict_bytes(_request(ids, wts), 30.0))
        served = torch.from_numpy(wt.to_ndarray(resp.outputs["prediction_node"]))
        assert served.shape == (300,) and (served - fused).abs().max().item() < 1e-5
    finally:
        live.close()


def test_bag_interaction_launcher_limits(cuda):
    """T = 32, hot = 1 and T * hot past the staging cap raise through the binding without a launch."""
    def call(T, hot):
        dense = torch.zeros(2, 64, dtype=torch.bfloat16, device=cuda)
        table = torch.zeros(T * 4, 64, dtype=torch.bfloat16, device=cuda)
        ids = torch.zeros(2, T * hot, dtype=torch.int64, device=cuda)
        mod = torch.full((T,), 4, dtype=torch.int64, device=cuda)
        off = torch.arange(T, dtype=torch.int64, device=cuda) * 4
        ops.dot_interaction_bag(dense, table, ids, None, hot, mod, off, out_cols=1024)
        ops.dot_interaction_bag_fp8(dense, table.to(F8), torch.ones(T, device=cuda), ids, None, hot, mod, off,
                                    out_cols=1024)

    call(31, 16)  # the largest served shape
    for T, hot in ((32, 2), (4, 1), (31, 17), (2, 257)):
        with pytest.raises(RuntimeError):
            call(T, hot)
    torch.cuda.synchronize()
