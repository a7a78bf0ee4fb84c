"""ops.cross_mix on the CPU (DCN-v2 mixture of low-rank cross experts) against
an fp64 reference in the sum-over-experts form, and the model built on it."""
import math

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model


def mix_inputs(M, d, E, r, seed=0, extra_rows=0):
    """Seeded x0, xl ~ N(0, 1) and weights scaled so y = U h + b has about unit
    rms: the cross term is as large as the residual."""
    g = torch.Generator().manual_seed(seed + 1000 * M + d + 7 * E + r)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x0, xl = n(M + extra_rows, d).bfloat16(), n(M + extra_rows, d).bfloat16()
    V, G = (n(E * r, d) / math.sqrt(d)).bfloat16(), (n(E, d) / math.sqrt(d)).bfloat16()
    C = (n(E, r, r) * (1.5 / math.sqrt(r))).bfloat16()
    U = (n(d, E * r) * (1.3 * math.sqrt(E / r))).bfloat16()  # h ~ 0.8 / E per column: y ~ unit rms
    return x0, xl, (V, G, C, U), n(d) * 0.1, n(d) / math.sqrt(d)


def mix_ref(x0, xl, weights, b, head_w):
    """fp64, sum over experts, with the three bf16 roundings of the contract
    (a after the first tanh, p_i c_i, and z) -> (z fp64 of the bf16 values, logit)."""
    V, G, C, U = (t.double() for t in weights)
    E, r = C.shape[:2]
    rb = lambda t: t.float().bfloat16().double()  # noqa: E731
    x0, xl = x0.double(), xl.double()
    a = rb(torch.tanh(xl @ V.t()))
    p = torch.softmax(xl @ G.t(), dim=1)
    z = xl.clone()
    for i in range(E):
        s = slice(i * r, (i + 1) * r)
        h = rb(torch.tanh(a[:, s] @ C[i].t()) * p[:, i:i + 1])
        # p_i x0 * (U_i c_i + b): the gate is inside h, and sum_i p_i b = b
        z += x0 * (h @ U[:, s].t() + p[:, i:i + 1] * b.double())
    z = rb(z)
    return z, z @ head_w.double()


def check_close(got, ref, what):
    """|got - ref| <= 2^-7 |ref| + 2^-7 rms(ref); returns the largest error in units of 2^-8 |ref|."""
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 2.0 ** -7 * ref.pow(2).mean().sqrt()
    worst = (err / (2.0 ** -8 * ref.abs()).clamp_min(1e-30))[err > 0].max().item() if (err > 0).any() else 0.0
    print(f"{what}: max err / (2^-8 |ref|) = {worst:.3f}, max err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), f"{what}: {(err > bound).sum().item()} of {err.numel()} outside the bound"
    return worst


@pytest.mark.parametrize("E,r", [(1, 64), (4, 64), (3, 16)])
def test_cross_mix_cpu_matches_sum_over_experts(E, r):
    x0, xl, w, b, hw = mix_inputs(5, 192, E, r)
    zr, lr = mix_ref(x0, xl, w, b, hw)
    assert (zr - xl.double()).pow(2).mean().sqrt() > 0.5  # the cross term is as large as the residual
    z, _ = ops.cross_mix(x0, xl, w, b)
    none, logit = ops.cross_mix(x0, xl, w, b, want_z=False, head_w=hw)
    assert none is None and z.dtype == torch.bfloat16
    check_close(z, zr, "z")
    check_close(logit, lr, "logit")


def _mix_cfg(**kw):
    base = dict(family="dcn_v2", cross_experts=4, cross_rank=64, num_fields=3, vocab_size=1000, mlp_dims=(64, 32))
    base.update(kw)
    return ModelConfig(**base)


def test_dcn_v2_mix_model_cpu():
    m = build_model(_mix_cfg(), "cpu")
    g = torch.Generator().manual_seed(3)
    y = m(torch.randint(0, 10 ** 9, (70, 3), generator=g), torch.rand(70, 3, generator=g))
    assert y.shape == (70,) and torch.isfinite(y).all() and ((y > 0) & (y < 1)).all()
    assert y.std() > 1e-4


def test_dcn_v2_mix_preset_answers_predict():
    """The preset, shrunk to a CPU-sized table, served in process."""
    import numpy as np

    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import tensor as T

    cfg = load_preset("dcn_v2_mix")
    assert (cfg.model.cross_experts, cfg.model.cross_rank, cfg.model.gemm_dtype) == (4, 64, "bf16")
    cfg.model.vocab_size, cfg.model.num_cross_layers, cfg.model.mlp_dims = 2000, 2, (64, 32)
    cfg.serving.max_batch_rows, cfg.serving.allowed_batch_sizes = 64, (8, 64)
    srv = ModelServer(cfg, device="cpu")
    try:
        msg = SyntheticRequests(fields=43, seed=9).message(20)
        got = T.to_ndarray(srv.service.predict(msg, 30.0).outputs["prediction_node"])
        m = srv.registry.resolve("DCN").model
        want = m(torch.as_tensor(T.to_ndarray(msg.inputs["feat_ids"])), torch.as_tensor(T.to_ndarray(msg.inputs["feat_wts"])))
        np.testing.assert_allclose(got, want.numpy(), atol=1e-5)
    finally:
        srv.stop()


def test_cross_mix_layer_repacks_in_place():
    layer = build_model(_mix_cfg(), "cpu").cross_mix[0]
    before = layer.packed()
    assert layer.packed() is before
    ptrs, old = [t.data_ptr() for t in before[:4]], before[3].clone()
    layer.U.mul_(2.0)
    after = layer.packed()
    assert [t.data_ptr() for t in after[:4]] == ptrs and torch.equal(after[3], old * 2)
    V, G, C, U = layer.raw()
    assert torch.equal(ops.unpack_bfrag(after[0], 256, 192), V) and torch.equal(ops.unpack_bfrag(after[1], 16, 192)[:4], G)
    assert torch.equal(ops.unpack_bfrag(after[2], 256, 256), torch.block_diag(*C))
    Up = ops.unpack_bfrag(after[3], 192, 256).view(6, 2, 4, 4, 256)  # [pair, t, q, s]: U row 8 q + 4 t + s
    assert torch.equal(Up.permute(0, 2, 1, 3, 4).reshape(192, 256), U)


@pytest.mark.parametrize("kw,limit", [(dict(cross_experts=8, cross_rank=64), "E * r <= 256"),
                                      (dict(cross_experts=9, cross_rank=16), "E <= 8"),
                                      (dict(cross_rank=24), "r % 16"), (dict(cross_rank=0), "cross_rank > 0"),
                                      (dict(embed_dim=40), "d % 64")])
def test_dcn_v2_mix_range_checked_at_build(kw, limit):
    with pytest.raises(ValueError, match=limit.replace("*", r"\*")):
        build_model(_mix_cfg(**kw), "cpu")
