"""The fused CIN layer kernel (csrc/kernels/cin.hip) against the matched fp64
reference of tests/test_cin.py, and the xDeepFM family on the GPU."""
import copy
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cin import cin_inputs, cin_ref  # noqa: E402
from test_cross_mix import check_close  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 1, 1, 16),                       # every minimum
    (3, 8, 8, 16),                       # no padding anywhere
    (5, 43, 43, 128), (9, 43, 128, 128),  # the preset's two layers: i padded to 44, j to 48
    (2, 64, 64, 16),                     # largest F
    (4, 7, 200, 200),                    # widths that are not multiples of 16, two column passes
    (3, 9, 256, 256),                    # the maxima
    (7, 43, 44, 48), (8, 43, 44, 48), (9, 43, 44, 48), (17, 43, 44, 48),  # B around a workgroup's 8 candidates
]


def _run(cuda, B, F, Hp, H, exact):
    x0, xp, W, bias, w_out = cin_inputs(B, F, Hp, H, exact=exact)
    xr, lr = cin_ref(x0, xp, W, bias, w_out, exact=exact)
    xk, logit = ops.cin_layer(*(t.to(cuda) for t in (x0, xp, W, bias, w_out)))
    xk, logit = xk.cpu(), logit.cpu()
    assert xk.shape == (B, -(-H // 16) * 16, 64) and (xk[:, H:] == 0).all()
    return xk[:, :H], logit, xr, lr


@pytest.mark.parametrize("B,F,Hp,H", SHAPES)
def test_cin_layer_matches_fp64(cuda, B, F, Hp, H):
    xk, logit, xr, lr = _run(cuda, B, F, Hp, H, exact=False)
    check_close(xk, xr, f"xk {(B, F, Hp, H)}")
    check_close(logit, lr, f"logit {(B, F, Hp, H)}")


@pytest.mark.parametrize("B,F,Hp,H", [SHAPES[0], SHAPES[3], SHAPES[5], SHAPES[10]])
def test_cin_layer_exact_on_small_integers(cuda, B, F, Hp, H):
    """Every product and partial sum is an exact integer below 2^24 (cin_ref
    asserts it): any packing, padding or indexing slip changes a bit."""
    xk, logit, xr, lr = _run(cuda, B, F, Hp, H, exact=True)
    assert torch.equal(xk.double(), xr) and torch.equal(logit.double(), lr)


def test_cin_layer_call_forms(cuda):
    B, F, Hp, H = 11, 43, 44, 40
    x0, xp, W, bias, w_out = cin_inputs(B, F, Hp, H)
    xr, lr = cin_ref(x0, xp, W, bias, w_out)
    big0 = torch.full((B + 1, F * 64 + 24), 5.0, dtype=torch.bfloat16, device=cuda)
    bigp = torch.full((B + 2, (Hp + 4) * 64 + 8), 7.0, dtype=torch.bfloat16, device=cuda)  # 4 maps past H_prev
    buf = torch.full((B + 3, 48 * 64 + 16), 3.0, dtype=torch.bfloat16, device=cuda)
    v0 = big0[:B, 8:8 + F * 64].unflatten(1, (F, 64))
    vp = bigp[:B, :(Hp + 4) * 64].unflatten(1, (Hp + 4, 64))
    out = buf[:B, 8:8 + 48 * 64].unflatten(1, (48, 64))
    v0.copy_(x0)
    vp[:, :Hp].copy_(xp)
    packed = ops.cin_pack(W.to(cuda))
    b, w = bias.to(cuda), w_out.to(cuda)
    xk, logit = ops.cin_layer(v0, vp, packed, b, w, out=out)
    assert xk.data_ptr() == out.data_ptr()
    check_close(xk[:, :H].cpu(), xr, "xk views")
    check_close(logit.cpu(), lr, "logit views")
    assert (xk[:, H:] == 0).all()
    assert (buf[B:] == 3.0).all() and (buf[:, :8] == 3.0).all() and (buf[:, 8 + 48 * 64:] == 3.0).all()
    none, l2 = ops.cin_layer(v0, vp, packed, b, w, want_x=False)
    assert none is None and torch.equal(l2, logit)  # the logit does not depend on writing xk
    pre = torch.arange(B, dtype=torch.float32, device=cuda)
    _, l3 = ops.cin_layer(v0, vp, packed, b, w, want_x=False, logit=pre)
    assert l3.data_ptr() == pre.data_ptr() and torch.equal(l3, torch.arange(B, device=cuda) + logit)


def test_xdeepfm_model_gpu_vs_cpu(cuda):
    cfg = ModelConfig(family="xdeepfm", vocab_size=20000, embed_dim=64, cin_dims=(32, 16), mlp_dims=(256, 128))
    m = build_model(cfg, "cpu")
    mg = copy.deepcopy(m).to(cuda)
    ids = torch.randint(0, 10 ** 9, (70, 43))
    wts = torch.rand(70, 43)
    y, yr = mg(ids.to(cuda), wts.to(cuda)).cpu(), m(ids, wts)
    assert torch.allclose(y, yr, rtol=2e-2, atol=5e-3), (y - yr).abs().max()


@pytest.mark.parametrize("F,Hp,H,D,limit", [(65, 65, 16, 64, "F <= 64"), (8, 8, 257, 64, "H <= 256"),
                                            (8, 8, 16, 32, "D = 64")])
def test_cin_layer_limits_raise(cuda, F, Hp, H, D, limit):
    x0, xp, W, bias, w_out = (t.to(cuda) for t in cin_inputs(2, F, Hp, H, D=D))
    with pytest.raises(ValueError, match=limit):
        ops.cin_layer(x0, xp, W, bias, w_out)
