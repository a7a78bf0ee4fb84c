"""ops.autoint on the CPU (AutoInt's multi-head field self-attention stack)
against an fp64 reference with the contract's bf16 roundings, and the family
built on it."""
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


def autoint_inputs(B, F, heads, L, D=64, exact=False):
    """-> x [B, F, D] bf16, L x (Wq, Wk, Wv, Wres) [D, D] bf16, w_out fp32 [F, D]. Random mode: scores of
    spread about 1.4 (attention neither uniform nor saturated, so an unmasked padded key shows).
    ``exact``: x in [-2, 2], weights and w_out in {-1, 0, 1}: integer q, k, v, a saturated softmax."""
    g = torch.Generator().manual_seed(1000 * B + 7 * F + 13 * heads + L + int(exact))
    if exact:
        r = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
        return (r(-2, 2, B, F, D).bfloat16(), [tuple(r(-1, 1, D, D).bfloat16() for _ in range(4)) for _ in range(L)],
                r(-1, 1, F, D))
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    sd, sqk = 1.0 / math.sqrt(D), 1.2 / math.sqrt(D) * (D // heads) ** -0.25
    layers = [tuple((n(D, D) * s).bfloat16() for s in (sqk, sqk, sd, sd)) for _ in range(L)]
    return n(B, F, D).bfloat16(), layers, n(F, D) / math.sqrt(D * F)


def autoint_ref(x, layers, heads, w_out):
    """The contract in fp64 with its bf16 roundings -> (y^L fp64 of the bf16 values, logit)."""
    rb = lambda t: t.float().bfloat16().double()  # noqa: E731
    y = x.double()
    B, F, D = y.shape
    for Wq, Wk, Wv, Wr in layers:
        q, k, v = (rb(y @ W.double()).view(B, F, heads, -1).transpose(1, 2) for W in (Wq, Wk, Wv))
        s = q @ k.transpose(-1, -2)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = (rb(e) @ v) / e.sum(-1, keepdim=True)
        y = rb(torch.relu(o.transpose(1, 2).reshape(B, F, D) + y @ Wr.double()))
    return y, (y * w_out.double()).sum((1, 2))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("B,F,heads,L,D", [(9, 43, 2, 2, 64), (5, 17, 4, 1, 64), (3, 7, 2, 2, 16), (3, 1, 4, 1, 16)])
def test_autoint_cpu_matches_fp64(B, F, heads, L, D, exact):
    x, layers, w_out = autoint_inputs(B, F, heads, L, D, exact)
    yr, lr = autoint_ref(x, layers, heads, w_out)
    y, logit = ops.autoint(x, layers, heads, w_out)
    none, again = ops.autoint(x, layers, heads, w_out, want_x=False, logit=torch.ones(B))
    assert none is None and y.dtype == torch.bfloat16 and y.shape == (B, F, D) and torch.equal(again, logit + 1)
    assert ops.autoint(x, layers, heads)[1] is None
    check_close(y, yr, "y")
    check_close(logit, lr, "logit")


def _cfg(**kw):
    base = dict(family="autoint", num_fields=5, vocab_size=2000, embed_dim=16, mlp_dims=(64, 32), autoint_layers=2)
    base.update(kw)
    return ModelConfig(**base)


def test_autoint_model_cpu():
    m = build_model(_cfg(), "cpu")
    g = torch.Generator().manual_seed(3)
    y = m(torch.randint(0, 10 ** 9, (70, 5), generator=g), torch.rand(70, 5, generator=g))
    assert y.shape == (70,) and torch.isfinite(y).all() and ((y > 0) & (y < 1)).all()
    assert y.std() > 1e-4


def test_autoint_preset_answers_predict():
    """The preset, shrunk to a CPU-sized table, served in process."""
    import numpy as np

    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import tensor as T

    cfg = load_preset("autoint_1gpu")
    mc = cfg.model
    assert (mc.family, mc.autoint_layers, mc.autoint_heads, mc.num_fields) == ("autoint", 3, 2, 43)
    mc.vocab_size, mc.embed_dim, mc.mlp_dims = 2000, 16, (64, 32)
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


def test_autoint_pack_round_trips_and_repacks_in_place():
    st = build_model(_cfg(embed_dim=64, num_fields=19), "cpu").attn
    before = st.packed()
    assert st.packed() is before
    wpack, opack, L = before
    assert L == 2 and wpack.shape == (2, 4, 4, 2, 64, 8) and opack.shape == (2, 2, 4, 16, 8)
    ptrs, old = [wpack.data_ptr(), opack.data_ptr()], wpack[1, 2].clone()
    st.W[6].mul_(2.0)  # layer 1's Wv
    after = st.packed()
    assert [after[0].data_ptr(), after[1].data_ptr()] == ptrs and torch.equal(after[0][1, 2], old * 2)
    # fragment order -> W^T with permuted units (position 16 t + 4 j + s of a group = unit 8 j + 4 t + s) -> W
    for i, w in enumerate(st.W):
        wt = ops.unpack_bfrag(after[0][i // 4, i % 4], 64, 64).reshape(2, 2, 4, 4, 64).transpose(1, 2).reshape(64, 64)
        assert torch.equal(wt.t(), w)
    back = after[1].permute(0, 3, 1, 2, 4).reshape(32, 64)
    assert torch.equal(back[:19], st.w_out) and (back[19:] == 0).all()


@pytest.mark.parametrize("D,F,heads,L,limit", [(32, 43, 2, 3, "D = 64"), (64, 65, 2, 3, "F <= 64"), (64, 0, 2, 3, "1 <= F"),
                                               (64, 43, 3, 3, r"heads in \{1, 2, 4\}"), (64, 43, 2, 5, "L <= 4"),
                                               (64, 43, 2, 0, "1 <= L")])
def test_autoint_check_names_the_limit(D, F, heads, L, limit):
    with pytest.raises(ValueError, match=limit):
        ops.autoint_check(D, F, heads, L)
