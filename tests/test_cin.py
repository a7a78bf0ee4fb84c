"""ops.cin_layer on the CPU (xDeepFM's Compressed Interaction Network) against
an fp64 reference with the contract's two bf16 roundings, and the family built
on it."""
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


def cin_inputs(B, F, H_prev, H, seed=0, D=64, exact=False):
    """x0 [B, F, D], xp [B, H_prev, D] ~ N(0, 1) bf16 and W ~ N(0, 1) / sqrt(H_prev F): unit-rms maps.
    ``exact``: x in [-2, 2], W, bias, w_out in {-1, 0, 1}, all integers."""
    g = torch.Generator().manual_seed(seed + 1000 * B + 7 * F + 13 * H_prev + H)
    if exact:
        r = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
        return (r(-2, 2, B, F, D).bfloat16(), r(-2, 2, B, H_prev, D).bfloat16(), r(-1, 1, H, H_prev, F).bfloat16(),
                r(-1, 1, H), r(-1, 1, H))
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return (n(B, F, D).bfloat16(), n(B, H_prev, D).bfloat16(), (n(H, H_prev, F) / math.sqrt(H_prev * F)).bfloat16(),
            n(H) * 0.1, n(H) / math.sqrt(H))


def cin_ref(x0, xp, W, bias, w_out, exact=False):
    """fp64 with the two roundings (Z and X^k) -> (X^k fp64 of the bf16 values [B, H, D], logit).
    ``exact``: also asserts that every sum of magnitudes stays below 2^24, so
    fp32 partial sums are exact integers in any order."""
    rb = lambda t: t.float().bfloat16().double()  # noqa: E731
    z = rb(xp.double().unsqueeze(2) * x0.double().unsqueeze(1))
    x = rb(torch.einsum("bijd,hij->bhd", z, W.double()) + bias.double().view(1, -1, 1))
    if exact:
        assert torch.einsum("bijd,hij->bhd", z.abs(), W.double().abs()).max() + 1 < 2 ** 24
        assert (x.abs().sum(2) @ w_out.double().abs()).max() < 2 ** 24
    return x, x.sum(2) @ w_out.double()


@pytest.mark.parametrize("B,F,Hp,H,D", [(5, 43, 43, 128, 64), (3, 7, 20, 24, 16), (2, 1, 1, 16, 8)])
def test_cin_layer_cpu_matches_fp64(B, F, Hp, H, D):
    x0, xp, W, bias, w_out = cin_inputs(B, F, Hp, H, D=D)
    xr, lr = cin_ref(x0, xp, W, bias, w_out)
    assert Hp * F < 100 or 0.7 < xr.pow(2).mean().sqrt() < 1.4  # unit-rms maps (where the sums are long enough)
    xk, logit = ops.cin_layer(x0, xp, W, bias, w_out)
    none, again = ops.cin_layer(x0, xp, W, bias, w_out, want_x=False, logit=torch.ones(B))
    assert none is None and xk.dtype == torch.bfloat16 and xk.shape == (B, -(-H // 16) * 16, D)
    assert (xk[:, H:] == 0).all() and torch.equal(again, logit + 1)
    check_close(xk[:, :H], xr, "xk")
    check_close(logit, lr, "logit")


def _cfg(**kw):
    base = dict(family="xdeepfm", num_fields=5, vocab_size=2000, embed_dim=16, mlp_dims=(64, 32), cin_dims=(24, 8))
    base.update(kw)
    return ModelConfig(**base)


def test_xdeepfm_model_cpu():
    m = build_model(_cfg(), "cpu")
    g = torch.Generator().manual_seed(3)
    y = m(torch.randint(0, 10 ** 9, (70, 5), generator=g), torch.rand(70, 5, generator=g))
    assert y.shape == (70,) and torch.isfinite(y).all() and ((y > 0) & (y < 1)).all()
    assert y.std() > 1e-4


def test_xdeepfm_preset_answers_predict():
    """The preset, shrunk to a CPU-sized table, served in process."""
    import numpy as np

    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import tensor as T

    cfg = load_preset("xdeepfm_1gpu")
    assert (cfg.model.family, cfg.model.cin_dims, cfg.model.num_fields) == ("xdeepfm", (128, 128), 43)
    cfg.model.vocab_size, cfg.model.embed_dim, cfg.model.cin_dims, cfg.model.mlp_dims = 2000, 16, (12, 8), (64, 32)
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


def test_cin_repacks_in_place():
    cin = build_model(_cfg(), "cpu").cin
    before = cin.packed()
    assert cin.packed() is before
    ptrs, old = [p[0].data_ptr() for p in before], before[1][0].clone()
    cin.W[1].mul_(2.0)
    after = cin.packed()
    assert [p[0].data_ptr() for p in after] == ptrs and torch.equal(after[1][0], old * 2)
    # layer 2: W [8, 24, 5] -> [pass 1][i / 4 = 6][j / 8 = 1][block 1][fq 4][fr 16][s 8]
    Wp, H, Hp, F = after[1]
    assert (H, Hp, F) == (8, 24, 5) and Wp.shape == (1, 6, 1, 1, 4, 16, 8)
    back = Wp.permute(0, 3, 5, 1, 4, 2, 6).reshape(16, 24, 8)
    assert torch.equal(back[:8, :, :5], cin.W[1]) and (back[8:] == 0).all() and (back[:, :, 5:] == 0).all()


@pytest.mark.parametrize("D,F,Hp,H,limit", [(32, 43, 43, 128, "D = 64"), (64, 65, 65, 128, "F <= 64"),
                                            (64, 43, 257, 128, "H_prev <= 256"), (64, 43, 43, 257, "H <= 256"),
                                            (64, 43, 43, 0, "1 <= H <= 256")])
def test_cin_check_names_the_limit(D, F, Hp, H, limit):
    with pytest.raises(ValueError, match=limit):
        ops.cin_check(D, F, Hp, H)
    if D == 64 and H > 0:
        with pytest.raises(ValueError, match=limit):
            ops.cin_pack(torch.zeros(H, Hp, F, dtype=torch.bfloat16))
