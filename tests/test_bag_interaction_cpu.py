"""The multi-hot bag interaction ops on the CPU (plain fp32 torch math) against
an fp64 computation written out here, and the model's arena support."""
import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model


def bag_interaction_ref(dense, table, ids, wts, hot, rows, out_cols):
    """fp64: gather, weight, sum over hot, round to bf16, dots, lower triangle -> bf16 [B, out_cols]."""
    B, T = dense.shape[0], ids.shape[1] // hot
    t_of = torch.arange(T).repeat_interleave(hot)
    g = t_of * rows + torch.remainder(ids.long(), rows)
    vals = table.double()[g]  # [B, T * hot, 64]
    if wts is not None:
        vals = vals * wts.double().unsqueeze(-1)
    pooled = vals.view(B, T, hot, 64).sum(2).to(torch.bfloat16).double()
    X = torch.cat([dense.double().unsqueeze(1), pooled], 1)
    Z = X @ X.transpose(1, 2)
    li, lj = torch.tril_indices(T + 1, T + 1, offset=-1)
    out = torch.zeros(B, out_cols, dtype=torch.float64)
    out[:, :64] = dense.double()
    out[:, 64:64 + li.numel()] = Z[:, li, lj]
    return out.to(torch.bfloat16)


def small_integer_case(T, hot, B, rows, seed, weighted=True):
    """Integers in [-4, 4] (exact in e4m3 at scale 1), weights in {0, 1, 2}, ids negative and past 2^31."""
    g = torch.Generator().manual_seed(seed)
    dense = torch.randint(-4, 5, (B, 64), generator=g).to(torch.bfloat16)
    table = torch.randint(-4, 5, (T * rows, 64), generator=g).to(torch.bfloat16)
    ids = torch.randint(-(1 << 40), 1 << 40, (B, T * hot), generator=g)
    ids[0, 0], ids[0, -1] = -1, (1 << 33) + rows - 1
    wts = torch.randint(0, 3, (B, T * hot), generator=g).float() if weighted else None
    mod = torch.full((T,), rows, dtype=torch.int64)
    off = torch.arange(T, dtype=torch.int64) * rows
    return dense, table, ids, wts, mod, off


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("hot", [2, 3])
def test_bag_interaction_cpu_equals_fp64(hot, weighted):
    T, rows = 5, 97
    dense, table, ids, wts, mod, off = small_integer_case(T, hot, 7, rows, hot, weighted)
    want = bag_interaction_ref(dense, table, ids, wts, hot, rows, ops.interaction_cols(T))
    got = ops.dot_interaction_bag(dense, table, ids, wts, hot, mod, off)
    q = table.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), table.float())
    got8 = ops.dot_interaction_bag_fp8(dense, q, torch.ones(T), ids, wts, hot, mod, off)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want) and torch.equal(got8, want)


@pytest.mark.parametrize("table_dtype", ["bf16", "fp8"])
def test_multi_hot_dlrm_supports_arena(table_dtype):
    cfg = ModelConfig(family="dlrm", num_fields=13 + 15 * 2, num_dense=13, table_rows=101, embed_dim=64, multi_hot=2,
                      bottom_mlp=(512, 256, 64), mlp_dims=(64, 32), table_dtype=table_dtype)
    m = build_model(cfg, "cpu")
    assert m.supports_arena is True and m.narrow_weight_cols() == 0
    m.use_bag_interaction = False
    assert m.supports_arena is False
