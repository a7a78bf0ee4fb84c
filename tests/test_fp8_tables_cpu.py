"""fp8 DLRM embedding tables (ModelConfig.table_dtype: fp8) on the CPU: the
storage format (e4m3 codes + one power-of-two scale per table), the chunked
init, the reference forward, config / build errors, the preset and the
checkpoint round trip."""
import copy
import math

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig, load_preset
from distributed_tf_serving_amd.models import build_model
from distributed_tf_serving_amd.models.ctr import DLRM


def _cfg(**kw):
    base = dict(family="dlrm", table_rows=500, mlp_dims=(64, 32), bottom_mlp=(32, 64))
    base.update(kw)
    return ModelConfig(**base)


def _is_pow2(s: torch.Tensor) -> bool:
    m, _ = torch.frexp(s.double())
    return bool((m == 0.5).all())


def _tables():
    g = torch.Generator().manual_seed(7)
    rnd = (torch.randn(4, 300, 64, generator=g) * torch.tensor([1.0, 0.01, 37.0, 1e-3]).view(4, 1, 1)).to(torch.bfloat16)
    edge = torch.zeros(300, 64)
    edge[0, :4] = torch.tensor([3.0, -3.0, 0.0, -0.0])  # +-amax
    edge[1] = 3.0 * 2.0 ** -torch.arange(64)  # down through the subnormal range to zero
    edge[2] = -edge[1]
    edge[3] = torch.linspace(-3, 3, 64)
    edge[4:] = torch.randn(296, 64, generator=g) * 1e-3  # tiny against amax
    return {"random": rnd, "edge": edge.to(torch.bfloat16).unsqueeze(0), "zero": torch.zeros(1, 8, 64, dtype=torch.bfloat16)}


@pytest.mark.parametrize("kind", ["random", "edge", "zero"])
def test_quantiser_format_and_half_ulp_bounds(kind):
    x = _tables()[kind]  # [T, rows, 64] bf16
    T = x.shape[0]
    amax = x.float().abs().amax(dim=(1, 2))
    scale = ops.table_scale_fp8(amax)
    assert scale.dtype == torch.float32 and scale.shape == (T,) and _is_pow2(scale)
    # the exponent rule: the smallest e with amax / 2^e <= 448 (0 for an all-zero table)
    for t in range(T):
        if amax[t] == 0:
            assert scale[t] == 1.0
        else:
            assert amax[t] / scale[t] <= 448 and amax[t] / (scale[t] / 2) > 448
    q = torch.stack([ops.quant_table_fp8(x[t], float(scale[t])) for t in range(T)])
    assert q.dtype == torch.float8_e4m3fn
    assert ((q.view(torch.uint8) & 0x7F) != 0x7F).all(), "NaN code"
    rows = torch.arange(T * x.shape[1])
    tables = rows // x.shape[1]
    deq = ops.dequant_table_fp8(q.view(-1, 64), scale, rows, tables).view_as(x)
    assert deq.dtype == torch.float32
    xf, s = x.float(), scale.view(T, 1, 1)
    err = (deq - xf).abs()
    normal = xf.abs() >= 2.0 ** -6 * s
    assert (err[normal] <= 2.0 ** -4 * xf.abs()[normal]).all()
    assert (err[~normal] <= (2.0 ** -10 * s).expand_as(err)[~normal]).all()
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)  # every value is exactly a bf16 value


def test_every_e4m3_code_times_a_power_of_two_is_a_bf16_value():
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F].view(torch.float8_e4m3fn)
    assert codes.numel() == 254
    for e in (-20, -11, 0, 5):
        v = codes.float() * 2.0 ** e
        assert torch.equal(v.to(torch.bfloat16).float(), v)


def test_chunked_init_equals_quantised_bf16_table():
    cfg = _cfg(table_rows=5000)
    ref = build_model(cfg)
    f8 = copy.deepcopy(cfg)
    f8.table_dtype = "fp8"
    m = build_model(f8, table_chunk_rows=1536)  # 5000 = 3 * 1536 + 392: chunk boundaries inside every table
    assert m.emb is None and m.emb_q.dtype == torch.float8_e4m3fn and m.emb_q.shape == (30 * 5000, 64)
    assert m.emb_q.is_contiguous() and m.emb_scale.dtype == torch.float32 and m.emb_scale.shape == (30,)
    scale = ops.table_scale_fp8(torch.full((30,), m.table_bound))
    assert torch.equal(m.emb_scale, scale) and _is_pow2(scale)
    assert float(scale[0]) == 2.0 ** -11  # 0.125 / 2^-11 = 256 <= 448 < 512
    want = ops.quant_table_fp8(ref.emb.detach(), float(scale[0]))
    assert torch.equal(m.emb_q.view(torch.uint8), want.view(torch.uint8))
    # the default chunk (2^19 rows) gives the same store
    m2 = build_model(f8)
    assert torch.equal(m2.emb_q.view(torch.uint8), m.emb_q.view(torch.uint8))
    # the store is in the state dict and counted, the bf16 table is not there
    sd = m.state_dict()
    assert "emb_q" in sd and "emb_scale" in sd and "emb" not in sd
    assert ref.param_bytes() - m.param_bytes() == 30 * 5000 * 64 - 30 * 4
    assert m.narrow_weight_cols() == ref.narrow_weight_cols() == 13
    assert m.supports_arena == ref.supports_arena


def test_quantize_tables_imports_a_bf16_table():
    cfg = _cfg(table_rows=700, table_dtype="fp8")
    m = build_model(cfg)
    g = torch.Generator().manual_seed(3)
    mag = 2.0 ** torch.randint(-6, 6, (30,), generator=g).float()
    table = (torch.randn(30, 700, 64, generator=g) * mag.view(30, 1, 1)).to(torch.bfloat16).view(-1, 64)
    m.quantize_tables_(table, chunk_rows=256)
    amax = table.float().view(30, -1).abs().amax(1)
    scale = ops.table_scale_fp8(amax)
    assert torch.equal(m.emb_scale, scale) and _is_pow2(scale) and scale.unique().numel() > 1
    want = torch.cat([ops.quant_table_fp8(table[t * 700:(t + 1) * 700], float(scale[t])) for t in range(30)])
    assert torch.equal(m.emb_q.view(torch.uint8), want.view(torch.uint8))
    rows = torch.tensor([0, 699, 700, 30 * 700 - 1])
    deq = m.dequant_rows(rows)
    assert deq.dtype == torch.float32 and deq.shape == (4, 64)
    assert torch.equal(deq, want[rows].float() * scale[rows // 700].view(-1, 1))
    assert (deq - table[rows].float()).abs().max() <= 2.0 ** -4 * amax.max()
    with pytest.raises(ValueError):
        m.quantize_tables_(table[:-1])
    with pytest.raises(ValueError):
        build_model(_cfg(table_rows=700)).quantize_tables_(table)


@pytest.mark.parametrize("hot", [1, 2])
def test_cpu_forward_equals_bf16_model_holding_the_dequantised_table(hot):
    kw = dict(table_rows=500)
    if hot == 2:
        kw.update(multi_hot=2, num_fields=13 + 2 * 15)
    cfg = _cfg(**kw)
    f8 = copy.deepcopy(cfg)
    f8.table_dtype = "fp8"
    m8 = build_model(f8)
    g = torch.Generator().manual_seed(11)
    # per-table scales that differ: import a table whose tables have different ranges
    T = m8.T
    table = (torch.randn(T, 500, 64, generator=g) * (2.0 ** -(torch.arange(T) % 5).float()).view(T, 1, 1))
    m8.quantize_tables_(table.to(torch.bfloat16).view(-1, 64))
    assert m8.emb_scale.unique().numel() > 1
    m16 = build_model(cfg)
    m16.emb.data.copy_(m8.dequant_table())
    assert torch.equal(m16.emb.float(), m8.dequant_rows(torch.arange(T * 500)))
    ids = torch.randint(-10**12, 10**12, (37, 43), generator=g)
    wts = torch.rand(37, 43, generator=g)
    y8, y16 = m8(ids, wts), m16(ids, wts)
    assert y8.shape == (37,) and torch.isfinite(y8).all()
    assert torch.equal(y8, y16)
    # lookup(): the same rows / bags
    assert torch.equal(m8.lookup(ids, wts).float(), m16.lookup(ids, wts).float())
    if hot == 1:  # the fused op's CPU reference is the same math
        z8 = ops.dot_interaction_gather_fp8(m8.bottom_out(wts), m8.emb_q, m8.emb_scale, m8.sparse_ids(ids), m8.modulo_f,
                                            m8.offset_f, m8.inter_cols)
        z16 = ops.dot_interaction_gather(m16.bottom_out(wts), m16.emb, m16.sparse_ids(ids), m16.modulo_f, m16.offset_f,
                                         m16.inter_cols)
        assert torch.equal(z8.float(), z16.float())


def test_build_model_errors():
    with pytest.raises(ValueError, match="table_dtype"):
        build_model(ModelConfig(family="deepfm", vocab_size=1000, table_dtype="fp8"))
    with pytest.raises(ValueError, match="table_dtype"):
        build_model(_cfg(table_dtype="int4"))
    with pytest.raises(ValueError, match="table_dtype"):
        build_model(_cfg(table_dtype="fp16"))


def test_sharded_paths_reject_fp8_tables():
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import ShardedDLRM, build_parallel_model

    cfg = _cfg(table_dtype="fp8")
    with pytest.raises(ValueError, match="single-rank"):
        build_parallel_model(cfg, "cpu", shard_tables="on")
    with pytest.raises(ValueError, match="single-rank"):
        ShardedDLRM(cfg, DistContext(device=torch.device("cpu")), device="cpu")
    # one rank, unsharded: the fp8 model itself
    m = build_parallel_model(cfg, "cpu", shard_tables="auto")
    assert isinstance(m, DLRM) and m.emb_q is not None


def test_preset_loads():
    cfg = load_preset("dlrm_fp8_1gpu")  # load only: 192 GB of tables
    ref = load_preset("dlrm_sharded8")
    assert cfg.model.table_dtype == "fp8" and cfg.model.table_rows == 100_000_000 and cfg.client.backends == 1
    same = ("family", "num_fields", "num_dense", "embed_dim", "bottom_mlp", "mlp_dims", "param_dtype", "multi_hot")
    assert all(getattr(cfg.model, k) == getattr(ref.model, k) for k in same)
    assert ref.model.table_dtype == "bf16" and ModelConfig().table_dtype == "bf16"
    # the towers are built without the tables; the store would be 30 x 100M x 64 bytes
    m = DLRM(cfg.model, "cpu", materialize_tables=False)
    assert m.emb_q is None and m.emb is None and not m.supports_arena
    assert 30 * 100_000_000 * 64 + m.param_bytes() < 0.8 * 288e9


def test_checkpoint_round_trip(tmp_path):
    from distributed_tf_serving_amd.utils import checkpoint as ck

    cfg = _cfg(table_rows=300, table_dtype="fp8")
    m = build_model(cfg)
    g = torch.Generator().manual_seed(5)
    m.quantize_tables_((torch.randn(30 * 300, 64, generator=g) * 3).to(torch.bfloat16))
    path = str(tmp_path / "dlrm_fp8.safetensors")
    ck.save_model(m, path)
    rc = ck.read_config(path)
    assert rc.table_dtype == "fp8" and rc == cfg
    other = copy.deepcopy(rc)
    other.seed = cfg.seed + 1
    m2 = build_model(other)
    assert not torch.equal(m2.emb_q.view(torch.uint8), m.emb_q.view(torch.uint8))
    ck.load_model(m2, path)
    assert m2.emb_q.dtype == torch.float8_e4m3fn
    assert torch.equal(m2.emb_q.view(torch.uint8), m.emb_q.view(torch.uint8))
    assert torch.equal(m2.emb_scale, m.emb_scale)
    ids = torch.randint(0, 10**9, (9, 43), generator=g)
    wts = torch.rand(9, 43, generator=g)
    assert torch.equal(m2(ids, wts), m(ids, wts))
    assert math.isclose(float(m.emb_scale[0]), 2.0 ** round(math.log2(float(m.emb_scale[0]))))
