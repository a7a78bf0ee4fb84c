"""The MX-fp8 fused MLP tail without a GPU: the weight pack, the CPU form of
ops.mlp_tail_fp8 against the float64 reference of tests/exact_cases_fp8_tail.py,
faults injected into that reference (so the torch.equal comparisons of
tests/test_fp8_tail_gpu.py can fail), and the tail_dtype switch of the model."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cases_fp8_tail as xt  # noqa: E402

from distributed_tf_serving_amd import ops  # noqa: E402
from distributed_tf_serving_amd.config import ModelConfig, load_preset  # noqa: E402
from distributed_tf_serving_amd.models import build_model  # noqa: E402
from distributed_tf_serving_amd.models.layers import Dense, make_generator  # noqa: E402


# ------------------------------------------------------------------ pack
def _codes(N, K):
    """e4m3 [N, K] whose byte at (n, k) identifies the position (n * K + k mod 251)."""
    b = (torch.arange(N * K, dtype=torch.int64) % 251).to(torch.uint8).view(N, K)
    return b.view(torch.float8_e4m3fn), b


def test_pack_bfrag_fp8_layout():
    N, K = 48, 384
    Wq, b = _codes(N, K)
    P = ops.pack_bfrag_fp8(Wq)
    assert P.dtype == torch.float8_e4m3fn and tuple(P.shape) == (N // 16, K // 128, 2, 64, 16) and P.is_contiguous()
    flat = P.view(torch.uint8).reshape(-1)
    # hand-picked (n16, k128, h, lane, e): the docstring formula, on the flat bytes
    for n16, k128, h, lane, e in [(0, 0, 0, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 16, 0), (0, 0, 1, 0, 0), (0, 0, 0, 63, 15),
                                  (0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (2, 2, 1, 37, 9), (1, 2, 0, 50, 3), (2, 0, 1, 15, 15)]:
        fr, fq = lane & 15, lane >> 4
        off = ((n16 * (K // 128) + k128) * 2 + h) * 1024 + 16 * lane + e
        assert flat[off] == b[16 * n16 + fr, 128 * k128 + 64 * h + 16 * fq + e], (n16, k128, h, lane, e)
    # a lane's two halves are 16-byte K chunks fq and fq + 4 of the 128-deep tile
    assert flat[16 * 17] == b[1, 16] and flat[1024 + 16 * 17] == b[1, 64 + 16]


def test_pack_bfrag_fp8_round_trip_and_errors():
    for N, K in [(16, 128), (48, 384), (512, 1024), (256, 512)]:
        Wq, b = _codes(N, K)
        back = ops.unpack_bfrag_fp8(ops.pack_bfrag_fp8(Wq), N, K)
        assert back.dtype == torch.float8_e4m3fn and torch.equal(back.view(torch.uint8), b)
    for shape in [(8, 128), (16, 64), (24, 128), (16, 192)]:
        with pytest.raises(ValueError):
            ops.pack_bfrag_fp8(torch.zeros(shape).to(torch.float8_e4m3fn))
    with pytest.raises(ValueError):
        ops.pack_bfrag_fp8(torch.zeros(16, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.unpack_bfrag_fp8(ops.pack_bfrag_fp8(_codes(16, 128)[0]), 16, 256)


# ------------------------------------------------------------------ exact cases
def _run(c, x=None, **kw):
    return ops.mlp_tail_fp8(c.x if x is None else x, c.W2q, c.sw2, c.b2, c.act2, c.W3q, c.sw3, c.b3, c.act3, c.hw,
                            c.hbias, extra=c.extra[:, :c.M + xt.EXTRA_PAD], sigmoid=False, **kw)


@pytest.mark.parametrize("case", xt.CASES)
def test_cpu_op_equals_reference(case):
    """The generator asserts its exactness conditions; the CPU form of the op
    (fp32 torch on the project's own quantiser) then gives the float64
    reference exactly."""
    c = xt.tail_case(*case)
    y = _run(c)
    assert y.dtype == torch.float32 and torch.equal(y, c.ref)
    out = torch.empty(c.M)
    assert _run(c, out=out) is out and torch.equal(out, c.ref)


def test_reference_quantiser_is_the_projects():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(37, 1024, generator=g) * torch.exp2(torch.randint(-12, 12, (37, 1), generator=g).float()))
    x[3, 64:96] = 0
    x = x.to(torch.bfloat16)
    q, s = ops.quant_mx_fp8(x)
    qr, er = xt.mx_quant(x.double())
    assert torch.equal(q.double(), qr) and torch.equal(s.long() - 127, er)


# ------------------------------------------------------------------ mutants
def _changed(case, **fault):
    c = xt.tail_case(*case)
    return int((xt.tail_ref(c, **fault) != c.ref.double()).sum())


def _visible(family, *faults):
    """Outputs changed by any of ``faults``, per case of the family: at least
    one in every case of more than one row (a single score can coincide: the
    sw2 fault leaves family B's M = 1 score at -524), and some in the family."""
    n = {case: sum(_changed(case, **f) for f in faults) for case in xt.CASES if case[0] == family}
    assert all(v > 0 for case, v in n.items() if case[1] > 1), n
    assert sum(n.values()) > 0
    return n


@pytest.mark.parametrize("family", ["A", "B"])
def test_mutant_x_columns_swapped_across_a_block(family):
    """Codes of columns 95 / 96 (blocks 2 | 3) and 127 / 128 (K tiles 0 | 1) swapped."""
    _visible(family, dict(swap_x=(95, 96)), dict(swap_x=(127, 128)))


def test_mutant_x_scale_from_the_neighbouring_block():
    n = _visible("A", dict(shift_x_scale=True))
    assert all(v > 0 for v in n.values()), n
    # family B's x has one scale byte for every non-zero block: it cannot see this fault's like
    c = xt.tail_case(*[k for k in xt.CASES if k[0] == "B"][2])
    assert xt.tail_ref(c, parts=True).ex.unique().numel() <= 2


def test_mutant_h2_columns_swapped():
    """Neighbours inside a lane's 4 columns, across a 16-column tile and across a block."""
    _visible("B", dict(swap_h2=(1, 2)), dict(swap_h2=(15, 16)), dict(swap_h2=(31, 32)))


def test_mutant_sw2_shifted_by_one_channel():
    _visible("B", dict(shift_sw2=True))


def test_mutant_dropped_k_tile():
    for t in (0, 3, 7):
        _visible("B", dict(drop_k_tile=t))


# ------------------------------------------------------------------ model / config
def _small(**kw):
    base = dict(family="dcn_v2", vocab_size=5000, num_fields=43, embed_dim=64, num_cross_layers=3,
                gemm_dtype="fp8", tail_dtype="fp8")
    base.update(kw)
    return ModelConfig(**base)


def test_tail_dtype_default_and_preset():
    assert ModelConfig().tail_dtype == "bf16"
    assert load_preset("dcn_v2_fp8").model.tail_dtype == "bf16"
    cfg = load_preset("dcn_v2_fp8_tail")
    assert cfg.model.tail_dtype == "fp8" and cfg.model.gemm_dtype == "fp8" and cfg.model.family == "dcn_v2"
    ref = load_preset("dcn_v2_fp8")
    ref.model.tail_dtype = "fp8"
    assert cfg.model == ref.model and cfg.serving == ref.serving and cfg.client == ref.client


def test_tail_dtype_fp8_is_rejected_where_it_does_not_apply():
    for kw in (dict(family="deepfm", gemm_dtype="bf16"), dict(family="deepfm"), dict(gemm_dtype="bf16"),
               dict(mlp_dims=(256, 128)), dict(tail_dtype="fp16")):
        with pytest.raises(ValueError):
            build_model(_small(**kw))


def test_fp8_tail_model_on_cpu_tracks_the_bf16_tail():
    """Same weights (same seed), fp8 tail against bf16 tail: within the
    project's fp8-vs-reference bound on scores (0.05)."""
    m8 = build_model(_small())
    mb = build_model(_small(tail_dtype="bf16"))
    assert m8.mlp.tail_fp8 and all(l.fp8 for l in m8.mlp.layers)
    assert not mb.mlp.tail_fp8 and [l.fp8 for l in mb.mlp.layers] == [True, False, False]
    for a, b in zip(m8.state_dict().values(), mb.state_dict().values()):
        assert torch.equal(a, b)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 1 << 40, (96, 43), generator=g)
    wts = torch.rand(96, 43, generator=g)
    y8, yb = m8(ids, wts), mb(ids, wts)
    assert y8.shape == yb.shape == (96,) and bool(torch.isfinite(y8).all())
    assert (y8 - yb).abs().max() <= 0.05
    assert not torch.equal(y8, yb)  # the switch does change the numerics


def test_forward_head_routes_every_row_count_to_the_fp8_tail(monkeypatch):
    m8 = build_model(_small())
    seen = []
    real = ops.mlp_tail_fp8
    monkeypatch.setattr(ops, "mlp_tail_fp8", lambda *a, **k: (seen.append(a[0].shape[0]), real(*a, **k))[1])
    for rows in (1, 5):
        m8(torch.arange(rows * 43).view(rows, 43), torch.ones(rows, 43))
    assert seen == [1, 5]


# ------------------------------------------------------------------ Dense.packed("16f8")
def test_packed_16f8_repacks_in_place():
    d = Dense(1024, 512, "relu", torch.bfloat16, "cpu", make_generator(3, "cpu"), fp8=True)
    p = d.packed("16f8")
    assert p is d.packed("16f8")
    assert torch.equal(ops.unpack_bfrag_fp8(p, 512, 1024).view(torch.uint8), d.w_fp8.view(torch.uint8))
    old = p.clone()
    with torch.no_grad():
        d.weight.copy_(torch.flip(d.weight, dims=(0, 1)))
    d.quantize_fp8()
    p2 = d.packed("16f8")
    assert p2 is p and p2.data_ptr() == p.data_ptr()  # captured graphs keep reading this buffer
    assert not torch.equal(p2.view(torch.uint8), old.view(torch.uint8))
    assert torch.equal(ops.unpack_bfrag_fp8(p2, 512, 1024).view(torch.uint8), d.w_fp8.view(torch.uint8))
