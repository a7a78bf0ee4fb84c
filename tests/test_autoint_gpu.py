"""The fused AutoInt stack kernel (csrc/kernels/autoint.hip) against the matched
fp64 reference of tests/test_autoint.py, and the autoint family on the GPU."""
import copy
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_autoint import autoint_inputs, autoint_ref  # noqa: E402
from test_cross_mix import check_close  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, F, heads, L): F around every 16-row block edge, each with one head count (43 with all three); B around a
# workgroup's waves (8; 4 for the 4-block 4-head instance); L = 1, 2, 4 with distinct weights per layer
CASES = [(1, 1, 1, 1), (7, 15, 2, 2), (8, 16, 4, 1), (9, 17, 1, 4), (17, 31, 2, 1), (3, 32, 4, 2), (5, 33, 1, 1),
         (9, 43, 1, 2), (9, 43, 2, 4), (9, 43, 4, 1), (4, 48, 2, 2), (3, 63, 4, 4), (4, 64, 1, 1), (17, 64, 4, 2),
         (2, 64, 2, 4)]


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("B,F,heads,L", CASES)
def test_autoint_matches_fp64(cuda, B, F, heads, L, exact):
    x, layers, w_out = autoint_inputs(B, F, heads, L, exact=exact)
    yr, lr = autoint_ref(x, layers, heads, w_out)
    y, logit = ops.autoint(x.to(cuda), [tuple(w.to(cuda) for w in lw) for lw in layers], heads, w_out.to(cuda))
    assert torch.isfinite(y.float()).all() and torch.isfinite(logit).all()
    check_close(y, yr, f"y {(B, F, heads, L, exact)}")
    check_close(logit, lr, f"logit {(B, F, heads, L, exact)}")


def test_autoint_call_forms(cuda):
    B, F, heads, L = 11, 43, 2, 3
    x, layers, w_out = autoint_inputs(B, F, heads, L)
    yr, lr = autoint_ref(x, layers, heads, w_out)
    big = torch.full((B + 1, F * 64 + 24), 5.0, dtype=torch.bfloat16, device=cuda)
    buf = torch.full((B + 3, F * 72 + 16), 3.0, dtype=torch.bfloat16, device=cuda)
    xv = big[:B, 8:8 + F * 64].unflatten(1, (F, 64))
    out = buf[:B, 8:8 + F * 72].unflatten(1, (F, 72))[:, :, :64]  # rows 144 bytes apart
    xv.copy_(x)
    raw, wo = [tuple(w.to(cuda) for w in lw) for lw in layers], w_out.to(cuda)
    packed = ops.autoint_pack(raw, wo)
    y, logit = ops.autoint(xv, packed, heads, out=out)
    assert y.data_ptr() == out.data_ptr()
    check_close(y, yr, "y views")
    check_close(logit, lr, "logit views")
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:B, 8:8 + F * 72].unflatten(1, (F, 72))[:, :, :64] = False
    assert (buf[mask] == 3.0).all() and torch.equal(xv.cpu(), x)
    y2, l2 = ops.autoint(xv, raw, heads, wo)
    assert torch.equal(y2, y) and torch.equal(l2, logit)  # packed weights against raw weights
    none, l3 = ops.autoint(xv, packed, heads, want_x=False)
    assert none is None and torch.equal(l3, logit)  # the logit does not depend on writing y
    pre = torch.arange(B, dtype=torch.float32, device=cuda)
    _, l4 = ops.autoint(xv, packed, heads, want_x=False, logit=pre)
    assert l4.data_ptr() == pre.data_ptr() and torch.equal(l4, torch.arange(B, device=cuda) + logit)


def test_autoint_model_gpu_vs_cpu(cuda):
    cfg = ModelConfig(family="autoint", vocab_size=20000, embed_dim=64, mlp_dims=(256, 128))
    m = build_model(cfg, "cpu")
    mg = copy.deepcopy(m).to(cuda)
    ids = torch.randint(0, 10 ** 9, (70, 43))
    wts = torch.rand(70, 43)
    y, yr = mg(ids.to(cuda), wts.to(cuda)).cpu(), m(ids, wts)
    assert torch.allclose(y, yr, rtol=2e-2, atol=5e-3), (y - yr).abs().max()


@pytest.mark.parametrize("F,heads,L,D,limit", [(65, 2, 1, 64, "F <= 64"), (8, 3, 1, 64, "heads in"), (8, 2, 5, 64, "L <= 4"),
                                               (8, 2, 1, 32, "D = 64"), (8, 2, 1, 68, "16-byte aligned rows")])
def test_autoint_limits_raise(cuda, F, heads, L, D, limit):
    x = torch.zeros(2, F, D, dtype=torch.bfloat16, device=cuda)
    layers = [tuple(torch.zeros(64, 64, dtype=torch.bfloat16, device=cuda) for _ in range(4))] * L
    if D == 68:  # D = 64 rows that start 2 bytes off a 16-byte boundary
        x = x.flatten()[1:1 + 2 * F * 64].unflatten(0, (2, F, 64))
    with pytest.raises(ValueError, match=limit):
        ops.autoint(x, layers, heads)
