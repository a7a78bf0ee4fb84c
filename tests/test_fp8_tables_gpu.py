"""fp8 DLRM embedding tables on the GPU (csrc/kernels/interaction_fp8.hip): the
fused gather + interaction and the bag kernel against their bf16 twins on the
dequantised table (bit for bit where the format makes that possible) and the
fp32 CPU reference, the arena form, the model and the served step."""
import concurrent.futures as cf
import copy

import numpy as np
import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig, load_preset
from distributed_tf_serving_amd.models import build_model

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _close(a, b, rtol, atol, what=""):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    print(f"{what}: max err {err.max().item():.4g}")
    assert bad == 0, f"{what}: {bad}/{a.numel()} mismatches, max err {err.max().item():.4g}"


def _quantise(table: torch.Tensor, T: int, rows: int):
    """[T * rows, 64] -> (codes, scales by the exponent rule, the dequantised bf16 table)."""
    scale = ops.table_scale_fp8(table.float().view(T, -1).abs().amax(1))
    q = torch.cat([ops.quant_table_fp8(table[t * rows:(t + 1) * rows], float(scale[t])) for t in range(T)])
    return q, scale


def _dequant(q: torch.Tensor, scale: torch.Tensor, rows: int) -> torch.Tensor:
    g = torch.arange(q.shape[0])
    deq = ops.dequant_table_fp8(q, scale, g, g // rows)
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)
    return deq.to(torch.bfloat16)


# code bytes: +-448, +-the smallest subnormal, +-0, the smallest normal, 1.0
EXTREMES = torch.tensor([0x7E, 0xFE, 0x01, 0x81, 0x00, 0x80, 0x08, 0x38], dtype=torch.uint8)


@pytest.mark.parametrize("T,ids64,B", [(1, True, 517), (26, False, 517), (30, True, 517), (31, False, 517),
                                       (30, True, 1)])
def test_dot_interaction_gather_fp8(cuda, T, ids64, B):
    """The fused kernel on e4m3 codes == the bf16 kernel on the dequantised
    table, bit for bit (row view of the ids, per-table modulo + offset + scale,
    negative ids, every code extreme in the store's last row), and the fp32
    CPU reference on the dequantised rows."""
    g = torch.Generator().manual_seed(100 + T + B)
    rows = 1000
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16)
    # table t drawn at 2^-(t % 5): the rule's scales differ per table
    mag = (2.0 ** -(torch.arange(T) % 5).float()).repeat_interleave(rows).view(-1, 1)
    q, scale = _quantise((torch.randn(T * rows, 64, generator=g) * mag).to(torch.bfloat16), T, rows)
    assert T < 5 or scale.unique().numel() == 5
    q.view(torch.uint8)[-1] = EXTREMES.repeat(8)
    full = torch.randint(-(1 << 40), 1 << 40, (B, T + 13), generator=g)
    full[0, -1] = rows - 1 - 7 * rows  # a negative id onto the last row of the last table
    if B > 2:
        full[2, -1] = rows - 1 + (1 << 33) // rows * rows
    fi = full if ids64 else full.to(torch.int32)
    ids = fi[:, 13:]  # a row view, like DLRM.sparse_ids
    mod = torch.full((T,), rows, dtype=torch.int64)
    off = torch.arange(T, dtype=torch.int64) * rows
    assert (off[-1] + torch.remainder(ids[0, -1].long(), rows)).item() == T * rows - 1
    deq = _dequant(q, scale, rows)
    dc, qc, sc, dq, ic, mc, oc = (t.to(cuda) for t in (dense, q, scale, deq, fi, mod, off))
    z = ops.dot_interaction_gather_fp8(dc, qc, sc, ic[:, 13:], mc, oc)
    z16 = ops.dot_interaction_gather(dc, dq, ic[:, 13:], mc, oc)
    zr = ops.dot_interaction_gather_fp8(dense, q, scale, ids, mod, off)
    torch.cuda.synchronize()
    assert z.dtype == torch.bfloat16 and z.shape == zr.shape == (B, ops.interaction_cols(T, 64))
    assert torch.equal(z.cpu().view(torch.int16), z16.cpu().view(torch.int16))
    _close(z, zr, 1e-2, 5e-2, "dot gather fp8")
    used = 64 + (T + 1) * T // 2
    assert (z[:, used:] == 0).all() and torch.equal(z[:, :64].cpu(), dense)


@pytest.mark.parametrize("T,ids64", [(5, True), (31, False)])
def test_dot_interaction_gather_fp8_exact_small_integers(cuda, T, ids64):
    """Codes and dense are integers in [-2, 2], scales 1 and 2^-3 mixed per
    table: every product is a multiple of 2^-6 and every dot is below 256 in
    magnitude, so fp32 accumulation rounds nothing in any order and the
    output must equal the fp32 CPU reference rounded to bf16."""
    g = torch.Generator().manual_seed(T)
    B, rows = 37, 200
    dense = torch.randint(-2, 3, (B, 64), generator=g).to(torch.bfloat16)
    q = torch.randint(-2, 3, (T * rows, 64), generator=g).float().to(F8)
    assert torch.equal(q.float(), q.float().round()) and q.float().abs().max() == 2
    scale = torch.where(torch.arange(T) % 2 == 0, 1.0, 0.125).float()
    ids = torch.randint(-(1 << 40), 1 << 40, (B, T), generator=g)
    ids = ids if ids64 else ids.to(torch.int32)
    mod = torch.full((T,), rows, dtype=torch.int64)
    off = torch.arange(T, dtype=torch.int64) * rows
    z = ops.dot_interaction_gather_fp8(*(t.to(cuda) for t in (dense, q, scale, ids, mod, off)))
    zr = ops.dot_interaction_gather_fp8(dense, q, scale, ids, mod, off)
    torch.cuda.synchronize()
    assert zr.dtype == torch.bfloat16 and zr.float().abs().max() <= 256
    assert torch.equal(z.cpu(), zr)
    assert (z[:, 64 + (T + 1) * T // 2:] == 0).all()


def test_forward_arena_matches_packed_fp8(cuda):
    """K0 fused: the fp8 interaction reads the sparse ids from the raw request bytes."""
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.serving.arena import ArenaLayout
    from distributed_tf_serving_amd.serving.packing import PackedLayout

    cfg = ModelConfig(family="dlrm", table_rows=5000, table_dtype="fp8")
    m = build_model(cfg, cuda)
    assert m.supports_arena and m.emb is None and m.emb_q.dtype == F8 and m.emb_q.is_cuda
    A, L = ArenaLayout(43, 2048), PackedLayout(43)
    ar = A.alloc()
    s = SyntheticRequests(dist="zipf", id_space=1 << 50, seed=9)
    reqs = [s.message(n, raw=r).SerializeToString() for n, r in ((3, True), (250, True), (17, False), (200, True))]
    ab = A.build(ar, A.place(ar, reqs))
    dev = ar.to(cuda)
    A.decode_varints(dev)
    B = 512  # > total_rows: padding rows must score like zero-weight rows
    packed = A.unpack_cpu(ar, L.alloc(B))
    want = m(L.ids(packed).to(cuda), L.wts(packed).to(cuda)).cpu()
    got = m.forward_arena(dev, B).cpu()
    assert ab.total_rows == 470
    _close(got, want, 0, 2e-5, "dlrm fp8 arena vs packed")
    out = torch.zeros(B, dtype=torch.float32).pin_memory()
    m.forward_arena(dev, B, out=out)
    torch.cuda.synchronize()
    _close(out, want, 0, 2e-5, "dlrm fp8 arena into pinned host")


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("idx64", [True, False])
def test_embedding_bag_fp8(cuda, T, idx64):
    """bag_fp8_kernel (bag b scaled by table b mod T) vs the bf16 bag kernel
    and the fp32 CPU reference on the dequantised table."""
    g = torch.Generator().manual_seed(T)
    rows, nb = 3000 // T, 41
    R = T * rows
    mag = (2.0 ** -(2 * torch.arange(T)).float()).repeat_interleave(rows).view(-1, 1)
    q, scale = _quantise(((torch.rand(R, 64, generator=g) - 0.5) * mag).to(torch.bfloat16), T, rows)
    assert scale.unique().numel() == T
    deq = _dequant(q, scale, rows)
    lens = torch.randint(0, 9, (nb,), generator=g)
    lens[:3] = torch.tensor([0, 8, 1])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    bag = torch.repeat_interleave(torch.arange(nb), lens)
    # bag b reads rows of table b mod T (raw ids: R * k + the row, hashed back by modulo = R)
    idx = (bag % T) * rows + torch.randint(0, rows, (bag.numel(),), generator=g)
    idx = idx + R * torch.randint(0, 300, idx.shape, generator=g) if idx64 else idx.to(torch.int32)
    psw = torch.rand(idx.numel(), generator=g)
    qc, sc, ic, oc, pc = (t.to(cuda) for t in (q, scale, idx, offsets, psw))
    out = ops.embedding_bag_fp8(qc, sc, ic, oc, pc, modulo=R)
    ref = ops.embedding_bag(deq, idx, offsets, psw, modulo=R)
    _close(out, ref, 1e-4, 1e-4, "bag fp8 vs fp32 CPU on the dequantised table")
    _close(out, ops.embedding_bag(deq.to(cuda), ic, oc, pc, modulo=R), 1e-4, 1e-4, "bag fp8 vs bf16 kernel")
    _close(ops.embedding_bag_fp8(q, scale, idx, offsets, psw, modulo=R), ref, 1e-4, 1e-4, "bag fp8 CPU fallback")
    assert (out[0] == 0).all()  # the empty bag
    # bf16 output into a static buffer, unweighted, mean
    buf = torch.full((nb, 64), 7.0, dtype=torch.bfloat16, device=cuda)
    got = ops.embedding_bag_fp8(qc, sc, ic, oc, pc, modulo=R, out_bf16=True, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf.cpu(), out.cpu().to(torch.bfloat16))
    _close(ops.embedding_bag_fp8(qc, sc, ic, oc, None, modulo=R, mean=True),
           ops.embedding_bag(deq, idx, offsets, None, modulo=R, mean=True), 1e-4, 1e-4, "bag fp8 mean")
    # malformed CSR offsets are clamped, as in the bf16 kernel
    bad = offsets.clone()
    bad[-1] += 1000
    bad[1] = -5
    _close(ops.embedding_bag_fp8(qc, sc, ic, bad.to(cuda), pc, modulo=R)[2:-1], ref[2:-1], 1e-4, 1e-4, "clamped CSR")


@pytest.mark.parametrize("hot", [1, 2])
def test_fp8_model_equals_bf16_model_holding_the_dequantised_table(cuda, hot):
    kw = dict(family="dlrm", table_rows=1000, mlp_dims=(256, 128))
    if hot == 2:
        kw.update(multi_hot=2, num_fields=13 + 2 * 15)
    cfg = ModelConfig(**kw)
    f8 = copy.deepcopy(cfg)
    f8.table_dtype = "fp8"
    m8c = build_model(f8, "cpu")
    g = torch.Generator().manual_seed(hot)
    T = m8c.T
    mag = (2.0 ** -(torch.arange(T) % 5).float()).repeat_interleave(1000).view(-1, 1)
    m8c.quantize_tables_((torch.randn(T * 1000, 64, generator=g) * 0.125 * mag).to(torch.bfloat16))
    assert m8c.emb_scale.unique().numel() > 1
    m16c = build_model(cfg, "cpu")  # the same seed: identical towers
    m16c.emb.data.copy_(m8c.dequant_table())
    m8, m16 = copy.deepcopy(m8c).to(cuda), copy.deepcopy(m16c).to(cuda)
    assert m8.emb_q.is_cuda and m8.emb_q.dtype == F8 and m8.emb is None
    ids = torch.randint(0, 10**9, (300, 43), generator=g)
    wts = torch.rand(300, 43, generator=g)
    y8 = m8(ids.to(cuda), wts.to(cuda))
    y16 = m16(ids.to(cuda), wts.to(cuda))
    torch.cuda.synchronize()
    if hot == 1:
        assert torch.equal(y8.cpu(), y16.cpu())
        # lookup() (off the served path) returns the same rows
        assert torch.equal(m8.lookup(ids.to(cuda)).cpu(), m16.lookup(ids.to(cuda)).cpu())
    else:
        _close(y8, y16, 1e-4, 1e-4, "multi-hot fp8 vs bf16 on the dequantised table")
    _close(y8, m8c(ids, wts), 2e-2, 5e-3, "fp8 dlrm GPU vs its CPU forward")


def test_one_hot_fp8_dlrm_served_matches_eager():
    """The fp8-table DLRM on the GPU live server: host-narrowed requests, the
    arena-reading step, scores equal to the eager forward."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.ops import native
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import schema as pb
    from distributed_tf_serving_amd.wire import tensor as wt

    cfg = load_preset("deepfm_1gpu")
    cfg.model = ModelConfig(family="dlrm", table_rows=20_000, table_dtype="fp8")
    cfg.serving.max_batch_rows = 2048
    cfg.serving.allowed_batch_sizes = (256, 2048)
    srv = ModelServer(cfg, device="cuda:0")
    try:
        s = srv.registry.resolve("DCN")
        live, model = s.scheduler, s.model
        assert isinstance(live, LiveScheduler) and model.supports_arena
        assert model.emb is None and model.emb_q.dtype == F8
        assert live.narrow_wts_cols == 13
        synth = SyntheticRequests(fields=43, id_space=1 << 40, dist="zipf", seed=23)
        reqs = []
        for i in range(20):
            ids, wts = synth.arrays([512, 1, 100, 37, 300][i % 5])
            t = [("feat_ids", torch.from_numpy(ids)), ("feat_wts", torch.from_numpy(wts))]
            reqs.append((native().encode_predict_request("DCN", "serving_default", None, t, i % 2 == 0), ids, wts))
        with cf.ThreadPoolExecutor(8) as pool:
            outs = list(pool.map(lambda r: srv.service.predict_bytes(r[0], 30.0), reqs))
        for (data, ids, wts), resp in zip(reqs, outs):
            want = model(torch.from_numpy(ids).cuda(), torch.from_numpy(wts).cuda()).float().cpu().numpy()
            got = wt.to_ndarray(pb.PredictResponse.FromString(resp).outputs["prediction_node"])
            np.testing.assert_allclose(got, want, atol=2e-5)
        st = live.stats()
        assert st["narrowed"] > 0 and not st["broken"]
    finally:
        srv.stop()


def test_fp8_bindings_reject_bad_arguments(cuda):
    """Wrong code dtype, a scale of the wrong length, T = 32: the binding
    raises before any launch (and the device stays healthy)."""
    T, rows, B = 4, 100, 8
    dense = torch.zeros(B, 64, dtype=torch.bfloat16, device=cuda)
    q = torch.zeros(T * rows, 64, device=cuda).to(F8)
    scale = torch.ones(T, device=cuda)
    ids = torch.zeros(B, T, dtype=torch.int64, device=cuda)
    mod = torch.full((T,), rows, dtype=torch.int64, device=cuda)
    off = torch.arange(T, dtype=torch.int64, device=cuda) * rows
    ok = ops.dot_interaction_gather_fp8(dense, q, scale, ids, mod, off)
    assert (ok == 0).all()
    for bad_q in (q.view(torch.uint8), q.float().to(torch.bfloat16), q[:, :32]):
        with pytest.raises(RuntimeError):
            ops.dot_interaction_gather_fp8(dense, bad_q, scale, ids, mod, off)
    for bad_s in (torch.ones(T + 1, device=cuda), torch.ones(T - 1, device=cuda), scale.double(), scale.cpu()):
        with pytest.raises(RuntimeError):
            ops.dot_interaction_gather_fp8(dense, q, bad_s, ids, mod, off)
    T32 = 32
    with pytest.raises(RuntimeError):
        ops.dot_interaction_gather_fp8(dense, torch.zeros(T32 * rows, 64, device=cuda).to(F8), torch.ones(T32, device=cuda),
                                       torch.zeros(B, T32, dtype=torch.int64, device=cuda),
                                       torch.full((T32,), rows, dtype=torch.int64, device=cuda),
                                       torch.arange(T32, dtype=torch.int64, device=cuda) * rows)
    offsets = torch.tensor([0, 2, 4], device=cuda)
    idx = torch.zeros(4, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError):
        ops.embedding_bag_fp8(q.view(torch.uint8), scale, idx, offsets)
    with pytest.raises(RuntimeError):
        ops.embedding_bag_fp8(q, scale.double(), idx, offsets)
    with pytest.raises(RuntimeError):
        ops.embedding_bag_fp8(q, scale, idx, offsets, modulo=T * rows + 1)
    torch.cuda.synchronize()
    assert (ops.embedding_bag_fp8(q, scale, idx, offsets) == 0).all()
