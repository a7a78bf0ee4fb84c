"""Exact small-integer probes of the MFMA kernels: inputs on which the
kernels' arithmetic does not round (tests/exact_cases.py), compared bit for
bit with references that share no code with distributed_tf_serving_amd.ops.

The tolerance tests of test_kernels_gpu.py cannot see a wrong table row of one
field, swapped h1 columns or a misplaced scale panel (tests/
test_exact_cases_cpu.py pins that and shows that these cases can); here a
single misplaced element, dropped K step or stale ring slot changes an
integer. Every assertion is torch.equal or identical bits."""
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cases as xc  # noqa: E402
from arena_cases import arena_case as _arena_case  # noqa: E402

pytestmark = pytest.mark.gpu

_ACT = {"none": 0, "relu": 1}


class _Layer:
    """The attributes ops.gather_mlp reads off a models.layers.Dense."""

    def __init__(self, W, b, act, dev):
        self.weight, self.bias, self.act, self.fp8 = W.to(torch.bfloat16).to(dev), b.to(dev), act, False
        self.in_dim = self.k = W.shape[1]
        self._packed = ops.pack_frag32(self.weight)

    def packed(self, layout):
        assert layout == "32"
        return self._packed


def _layers(w, act2, act3, dev):
    return [_Layer(w.W1, w.b1, "relu", dev), _Layer(w.W2, w.b2, act2, dev), _Layer(w.W3, w.b3, act3, dev)]


def _tower(dev, c, w, fm, act2, act3, ids, wts, modulo, table=None, lin=None):
    """The one-launch tower, sigmoid off, run twice: the bits must repeat."""
    table = c.table.to(dev) if table is None else table
    lin = c.lin.to(dev) if lin is None else lin
    layers = _layers(w, act2, act3, dev)
    ys = [ops.gather_mlp(table, ids, wts, lin, modulo, w.bias, layers, w.hw.to(dev), w.hbias, fm=fm, sigmoid=False)
          for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)), "two runs of the tower differ"
    return ys[0].cpu()


# ------------------------------------------------------------------ tower
@pytest.mark.parametrize("case", xc.TOWER_CASES + xc.TOWER_MODULO_CASES)
def test_gather_mlp_exact(cuda, case):
    """Row counts around one 64-row workgroup, field counts around the 4-slot
    ring, every activation pattern, and every modulo path (multiply-high,
    modulo 1, rows clamped to V - 1, the plain 64-bit modulo from 2^32 up),
    from int64 ids over the whole range."""
    B, F, V, fm, act2, act3, modulo = case
    c, w, r = xc.tower_case(*case)
    y = _tower(cuda, c, w, fm, act2, act3, c.ids.to(cuda), c.wts.to(cuda), modulo)
    assert torch.equal(y, xc.f32(r.logit))


@pytest.mark.parametrize("case", xc.TOWER_FORM_CASES)
def test_gather_mlp_exact_input_forms(cuda, case):
    """int32 rows, and the strided narrow rows of the candidate fan-out."""
    from distributed_tf_serving_amd.serving.packing import PackedLayout

    B, F, V, fm, act2, act3, modulo = case
    c, w, r = xc.tower_case(*case)
    want = xc.f32(r.logit)
    y = _tower(cuda, c, w, fm, act2, act3, c.rows.to(torch.int32).to(cuda), c.wts.to(cuda), modulo)
    assert torch.equal(y, want)
    L = PackedLayout(F, narrow_modulo=V)
    buf = L.pack(c.ids, c.wts).to(cuda)
    iv, wv = L.ids(buf), L.wts(buf)
    assert not iv.is_contiguous() and iv.dtype == torch.int32
    y = _tower(cuda, c, w, fm, act2, act3, iv, wv, modulo)
    assert torch.equal(y, want)


def test_gather_mlp_exact_arena_rows(cuda):
    """The tower resolving its rows from request bytes (a raw, a packed-varint
    and a one-row request, padding rows past them)."""
    B, F, V = 200, 43, xc.TOWER_V
    A, ar, ids, wts = _arena_case(F, [(3, True), (150, False), (1, True), (37, True)], B, seed=21)
    dev = ar.to(cuda)
    A.decode_varints(dev)
    for fm, act2, act3 in xc.TOWER_ACTS:
        c, w, r = xc.tower_case(B, F, V, fm, act2, act3, V, ids=ids, wts=wts)
        y = _tower(cuda, c, w, fm, act2, act3, ops.ArenaRows(dev, B, F), None, V)
        assert torch.equal(y, xc.f32(r.logit))


# ------------------------------------------------------------------ gather-GEMM
def _embed_gemm_both(dev, table, lin, ids, wts, V, w, fm2):
    W, b = w.W1.to(torch.bfloat16).to(dev), w.b1.to(dev)
    Wp = ops.pack_frag32(W)
    for packed in (None, lambda: Wp):
        h, parts = ops.embed_gemm(table, ids, wts, lin, V, w.bias, W, b, "relu", fm2=fm2, packed_w=packed)
        torch.cuda.synchronize()
        yield ("one-wave" if packed else "8-phase"), h.cpu(), parts.cpu()


@pytest.mark.parametrize("case", xc.GATHER_GEMM_CASES)
def test_embed_gemm_exact(cuda, case):
    """Both gather-GEMM forms: h exact as bf16, and the first-order and FM
    partial logits exact row by row (each on its own, not only their sum)."""
    B, F, N, fm2 = case
    c, w, r = xc.gather_gemm_case(*case)
    d = [t.to(cuda) for t in (c.table, c.lin, c.ids, c.wts)]
    for form, h, parts in _embed_gemm_both(cuda, d[0], d[1], d[2], d[3], c.V, w, fm2):
        assert h.dtype == torch.bfloat16 and torch.equal(h, xc.bf16(r.h)), form
        assert parts.shape[0] == (2 if fm2 else 1)
        assert torch.equal(parts[0, :B], xc.f32(r.part0)), form
        if fm2:
            assert torch.equal(parts[1, :B], xc.f32(r.part1)), form


# ------------------------------------------------------------------ fused MLPs
@pytest.mark.parametrize("M", xc.MLP_M)
def test_mlp_tail_exact(cuda, M):
    for act2, act3 in (("relu", "relu"), ("none", "none"), ("relu", "none")):
        c = xc.mlp_tail_case(M, act2, act3)
        d = {k: v.to(cuda) for k, v in vars(c).items() if isinstance(v, torch.Tensor)}
        y = ops.mlp_tail(d["x"], ops.pack_bfrag(d["W2"]), d["b2"], act2, ops.pack_bfrag(d["W3"]), d["b3"], act3,
                         d["hw"], c.hbias, d["extra"], False)
        assert torch.equal(y.cpu(), c.y), (act2, act3)


@pytest.mark.parametrize("M", xc.MLP_M)
@pytest.mark.parametrize("N,K", xc.LINEAR_HEAD_NK)
def test_linear_head_exact(cuda, M, N, K):
    for act in ("relu", "none"):
        c = xc.linear_head_case(M, N, K, act)
        d = {k: v.to(cuda) for k, v in vars(c).items() if isinstance(v, torch.Tensor)}
        y = ops.linear_head(d["x"], d["W"], d["b"], act, d["hw"], c.hbias, d["extra"], False)
        assert torch.equal(y.cpu(), c.y), act


@pytest.mark.parametrize("M", xc.MLP_M)
@pytest.mark.parametrize("nd", [13, 64])
def test_bottom_mlp3_exact(cuda, M, nd):
    assert tuple(ops.BOTTOM_MLP3_DIMS) == xc.BOTTOM_MLP3_DIMS
    c = xc.bottom_mlp3_case(M, nd)
    y = ops.bottom_mlp3(c.full.to(cuda)[:, :nd + 3], nd, [(W.to(cuda), b.to(cuda)) for W, b in c.layers])
    assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), c.y)


# ------------------------------------------------------------------ GEMM tiles
@pytest.mark.parametrize("variant", xc.GEMM_VARIANTS)
@pytest.mark.parametrize("M,N,K", xc.GEMM_SHAPES)
def test_gemm_variants_exact(cuda, variant, M, N, K):
    """Every kept tile variant (0: the dispatcher's pick), epilogue none / relu,
    fp32 and bf16 output, ragged M and N."""
    for act, out_bf16 in xc.GEMM_EPI_OUT:
        c = xc.gemm_case(M, N, K, out_bf16, act)
        y = ops.hip().gemm(c.A.to(cuda), c.W.to(cuda), c.b.to(cuda), _ACT[act], None, None, not out_bf16, None, None,
                           None, variant)
        assert y.dtype == c.y.dtype and torch.equal(y.cpu(), c.y), (act, out_bf16)


# ------------------------------------------------------------------ fp8 / MX
@pytest.mark.parametrize("M,N,K", xc.FP8_SHAPES)
def test_linear_fp8_exact(cuda, M, N, K):
    for act in ("none", "relu"):
        c = xc.fp8_case(M, N, K, act)
        y = ops.linear_fp8(c.q.to(cuda), c.sx.to(cuda), c.Wq.to(cuda), c.sw.to(cuda), c.b.to(cuda), act, out_f32=True)
        assert torch.equal(y.cpu(), c.y), act


@pytest.mark.parametrize("variant", [17, 18])
def test_gemm_8phase_fp8_exact(cuda, variant):
    M, N, K = xc.FP8_VARIANT_SHAPE
    for act in ("none", "relu"):
        c = xc.fp8_case(M, N, K, act)
        y = ops.hip().gemm(c.q.to(cuda), c.Wq.to(cuda), c.b.to(cuda), _ACT[act], None, None, True, c.sx.to(cuda),
                           c.sw.to(cuda), None, variant)
        assert torch.equal(y.cpu(), c.y), act


def test_gemm_mx_block_scales_exact(cuda):
    """E8M0 exponents drawn per row AND per block: a scale panel read from a
    neighbouring row or block changes the result."""
    M, N, K = xc.MX_SHAPE
    assert K <= ops.MX_MAX_K == xc.MX_MAX_K
    for act in ("none", "relu"):
        c = xc.fp8_case(M, N, K, act, mx=True)
        y = ops.linear_fp8(c.q.to(cuda), None, c.Wq.to(cuda), c.sw.to(cuda), c.b.to(cuda), act, out_f32=True,
                           sx_blk=c.sx_blk.to(cuda))
        assert torch.equal(y.cpu(), c.y), act


@pytest.mark.parametrize("M,N", xc.CROSS_FP8_SHAPES)
def test_cross_gemm_fp8_exact(cuda, M, N):
    assert ops.CROSS_TILE == xc.CROSS_TILE
    c = xc.cross_fp8_case(M, N)
    d = {k: v.to(cuda) for k, v in vars(c).items() if isinstance(v, torch.Tensor)}
    z, dot = ops.cross_gemm_fp8(d["q"], d["sx"], d["Wq"], d["sw"], d["b"], d["x0"], d["xl"], want_z=True,
                                head_w=d["hw"])
    assert torch.equal(z.cpu(), c.z)
    assert dot.shape == c.d.shape and torch.equal(dot.cpu(), c.d)  # each 256-column tile's partial dot


# ------------------------------------------------------------------ interaction
@pytest.mark.parametrize("T", xc.INTERACTION_T)
def test_dot_interaction_exact(cuda, T):
    c = xc.interaction_case(T)
    z = ops.dot_interaction(c.dense.to(cuda), c.emb.to(cuda))
    assert z.shape == c.z.shape and torch.equal(z.cpu(), c.z)


@pytest.mark.parametrize("T", xc.INTERACTION_T)
def test_dot_interaction_gather_exact(cuda, T):
    c = xc.interaction_gather_case(T)
    z = ops.dot_interaction_gather(c.dense.to(cuda), c.table.to(cuda), c.ids.to(cuda), c.mod.to(cuda), c.off.to(cuda))
    assert z.shape == c.z.shape and torch.equal(z.cpu(), c.z)


# ------------------------------------------------------------------ address range
def test_gather_top_of_the_row_range(cuda):
    """Rows up to 2^25 - 1 (byte offsets up to 2^32 - 128 on an SGPR base): the
    tower, both gather-GEMM forms and the gather kernel at table rows on both
    sides of byte offset 2^31. The table is a view 2 GiB into one NaN-filled
    buffer that also extends past it, so a sign-extended or truncated row
    offset reads NaN from inside the same allocation (and fails the
    comparison) instead of leaving it."""
    GiB = 1 << 30
    if torch.cuda.mem_get_info()[0] < 8 * GiB:
        pytest.skip("needs 8 GiB of free device memory")
    V, B, F = xc.RANGE_V, 200, 43
    c, pos, ids = xc.range_case(B, F)
    w = xc.tower_weights(F)
    r = xc.tower_ref(c, w, True, "relu", "relu")
    nbytes = 2 * GiB + V * 128 + (1 << 20)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    buf.view(torch.bfloat16).fill_(float("nan"))
    table = buf[2 * GiB: 2 * GiB + V * 128].view(torch.bfloat16).view(V, 64)
    assert table.is_contiguous() and table.data_ptr() == buf.data_ptr() + 2 * GiB
    lin = torch.full((V,), float("nan"), dtype=torch.float32, device=cuda)
    dpos = pos.to(cuda)
    table[dpos] = c.table.to(cuda)
    lin[dpos] = c.lin.to(cuda)
    dids, dwts = ids.to(cuda), c.wts.to(cuda)

    y = _tower(cuda, c, w, True, "relu", "relu", dids, dwts, V, table=table, lin=lin)
    assert torch.equal(y, xc.f32(r.logit))
    for form, h, parts in _embed_gemm_both(cuda, table, lin, dids, dwts, V, w, True):
        assert torch.equal(h, xc.bf16(r.h1)), form
        assert torch.equal(parts[0, :B], xc.f32(r.first + w.bias)), form
        assert torch.equal(parts[1, :B], xc.f32(r.fm)), form
    x, fm = ops.embed(table, dids, dwts, lin=lin, modulo=V, bias=w.bias, want_x=True, want_fm=True, fm2=True)
    e, _ = xc.embed_ref(c)
    assert torch.equal(x.cpu(), xc.bf16(e.reshape(B, -1)))
    assert torch.equal(fm.cpu(), xc.f32(r.first + w.bias + r.fm))

    # one row more is outside the kernel's range: refused before any launch
    layers = _layers(w, "relu", "relu", cuda)
    over = buf[2 * GiB: 2 * GiB + (V + 1) * 128].view(torch.bfloat16).view(V + 1, 64)
    assert ops.gather_mlp_ok(table, layers, ops.GATHER_MLP_MIN_ROWS)
    assert not ops.gather_mlp_ok(over, layers, ops.GATHER_MLP_MIN_ROWS)
    lin1 = torch.zeros(V + 1, dtype=torch.float32, device=cuda)
    with pytest.raises(RuntimeError, match="outside the kernel's range"):
        ops.gather_mlp(over, dids, dwts, lin1, V, w.bias, layers, w.hw.to(cuda), w.hbias, fm=True, sigmoid=False)
    del buf, table, over, lin, lin1
    torch.cuda.empty_cache()
