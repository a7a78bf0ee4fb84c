"""ops.din_attention on the CPU (DIN target attention) against an fp64 reference
in the paper's unfolded 4-block form, and the model family built on it."""
import math
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cross_mix import check_close  # noqa: E402


def din_inputs(B, P, H, a1, a2, D=64, seed=0, zero_hist=0.3):
    """Seeded inputs: ids uniform in +-1e12 over a 1000-row N(0, 1) table (the
    target and the history collide), weights in [0, 1) with ``zero_hist`` of the
    history weights 0; W1 = [A | B | C | E] whose fold is exact in fp32."""
    g = torch.Generator().manual_seed(seed + 1000 * B + 100 * P + H + 7 * a1 + a2 + D)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    F = P + 1 + H
    table = n(1000, D).bfloat16()
    ids = torch.randint(-10 ** 12, 10 ** 12, (B, F), generator=g)
    wts = torch.rand(B, F, generator=g)
    wts[:, P + 1:] *= (torch.rand(B, H, generator=g) >= zero_hist)
    Wq, Wk, C, Wp = ((n(a1, D) / math.sqrt(3 * D)).bfloat16().float() for _ in range(4))
    W1 = torch.cat([Wq - C, Wk + C, C, Wp], dim=1)  # A + C = Wq, B - C = Wk
    folded = ops.din_fold(W1)
    assert all(torch.equal(f.float(), w) for f, w in zip(folded, (Wq, Wk, Wp)))
    rest = (n(a1) * 0.1, torch.full((a1,), 0.25), (n(a2, a1) * (1.4 / math.sqrt(a1))).bfloat16(), n(a2) * 0.1,
            torch.full((a2,), 0.25), n(a2) * (1.4 / math.sqrt(a2)), n(1) * 0.1)
    return table, ids, wts, W1, (*folded, *rest)


def din_ref(table, ids, wts, P, W1, weights):
    """fp64 on u = [q, k, q - k, q * k] with the contract's bf16 roundings (e, p,
    a1, v) -> (front [B, (P + 1) D] of the bf16 values, v fp64 before its rounding)."""
    b1, al1, W2, b2, al2, w3, b3 = (t.double() for t in weights[3:])
    rb = lambda t: t.float().bfloat16().double()  # noqa: E731
    prelu = lambda z, a: torch.where(z > 0, z, a * z)  # noqa: E731
    e = rb(table[torch.remainder(ids, table.shape[0])].double() * wts.double().unsqueeze(-1))
    q, k = e[:, P:P + 1], e[:, P + 1:]
    u = torch.cat([q.expand_as(k), k, q - k, rb(q * k)], dim=-1)
    a1v = rb(prelu(u @ W1.double().t() + b1, al1))
    s = prelu(a1v @ W2.t() + b2, al2) @ w3 + b3
    return e[:, :P + 1].reshape(e.shape[0], -1), (s.unsqueeze(-1) * k).sum(1)


def check_din(x, table, ids, wts, P, W1, weights, what):
    """Front columns bit-equal, v inside check_close's bound of the fp64 reference."""
    front, v = din_ref(table, ids, wts, P, W1, weights)
    D = table.shape[1]
    assert x.dtype == torch.bfloat16 and tuple(x.shape) == (ids.shape[0], (P + 2) * D)
    assert torch.equal(x[:, :(P + 1) * D].double().cpu(), front), f"{what}: profile / q columns"
    check_close(x[:, (P + 1) * D:], v, what)


@pytest.mark.parametrize("D", [64, 16])
@pytest.mark.parametrize("B,P,H,a1,a2", [(5, 3, 7, 80, 40), (4, 0, 1, 16, 16), (3, 26, 16, 24, 8)])
def test_din_attention_cpu_matches_unfolded_fp64(B, P, H, a1, a2, D):
    table, ids, wts, W1, w = din_inputs(B, P, H, a1, a2, D)
    check_din(ops.din_attention(table, ids, wts, P, H, w), table, ids, wts, P, W1, w, f"v D={D}")


def test_din_zero_weight_is_padding():
    P, H = 2, 9
    table, ids, wts, _, w = din_inputs(6, P, H, 80, 40, zero_hist=0.0)
    wts[:, P + 1 + 4] = 0.0
    keep = [c for c in range(P + 1 + H) if c != P + 1 + 4]
    x = ops.din_attention(table, ids, wts, P, H, w)
    assert torch.equal(x, ops.din_attention(table, ids[:, keep], wts[:, keep], P, H - 1, w))
    wts[:, P + 1:] = 0.0
    v = ops.din_attention(table, ids, wts, P, H, w)[:, (P + 1) * 64:]
    assert (v == 0).all()


@pytest.mark.parametrize("kw", [dict(num_fields=43, seq_len=43), dict(num_fields=10, seq_len=16), dict(seq_len=0)])
def test_din_fields_checked_at_build(kw):
    with pytest.raises(ValueError, match="seq_len"):
        build_model(ModelConfig(family="din", vocab_size=1000, mlp_dims=(64, 32), **kw), "cpu")


def test_din_preset_answers_predict():
    """The preset, shrunk to a CPU-sized table, served in process."""
    import numpy as np

    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import tensor as T

    cfg = load_preset("din_1gpu")
    assert (cfg.model.num_fields, cfg.model.seq_len, tuple(cfg.model.att_dims)) == (77, 50, (80, 40))
    cfg.model.vocab_size, cfg.model.mlp_dims = 2000, (64, 32)
    cfg.serving.max_batch_rows, cfg.serving.allowed_batch_sizes = 64, (8, 64)
    srv = ModelServer(cfg, device="cpu")
    try:
        msg = SyntheticRequests(fields=77, seed=9).message(20)
        got = T.to_ndarray(srv.service.predict(msg, 30.0).outputs["prediction_node"])
        m = srv.registry.resolve("DCN").model
        assert (m.P, m.H) == (26, 50)
        want = m(torch.as_tensor(T.to_ndarray(msg.inputs["feat_ids"])), torch.as_tensor(T.to_ndarray(msg.inputs["feat_wts"])))
        np.testing.assert_allclose(got, want.numpy(), atol=1e-5)
    finally:
        srv.stop()
