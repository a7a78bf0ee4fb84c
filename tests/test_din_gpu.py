"""The fused DIN attention kernel (csrc/kernels/din_attention.hip) against the
matched fp64 reference of tests/test_din.py, and the model family on the GPU."""
import copy
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_din import check_din, din_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,P,H,a1,a2", [
    (1, 0, 1, 16, 16),                                           # every minimum
    (5, 3, 1, 80, 40),                                           # H = 1, padded widths
    (65, 3, 31, 80, 40), (64, 3, 32, 80, 40), (129, 3, 33, 80, 40),  # MFMA block edge in H, B around 64
    (63, 0, 64, 80, 40),                                         # largest H, no profile fields
    (65, 26, 16, 80, 40),                                        # the default layout
    (33, 2, 50, 128, 64),                                        # largest widths
    (64, 2, 17, 24, 8),                                          # widths that are not multiples of 16
])
def test_din_attention_matches_fp64(cuda, B, P, H, a1, a2):
    table, ids, wts, W1, w = din_inputs(B, P, H, a1, a2)
    x = ops.din_attention(table.to(cuda), ids.to(cuda), wts.to(cuda), P, H, tuple(t.to(cuda) for t in w))
    check_din(x.cpu(), table, ids, wts, P, W1, w, f"v {(B, P, H, a1, a2)}")


def test_din_attention_views_int32_and_out(cuda):
    B, P, H, a1, a2 = 65, 3, 33, 80, 40
    F = P + 1 + H
    table, ids, wts, W1, w = din_inputs(B, P, H, a1, a2)
    ids = torch.remainder(ids, 2 ** 31) - 2 ** 30  # int32 range, both signs
    wide_i = torch.full((B, F + 5), 7, dtype=torch.int32, device=cuda)
    wide_w = torch.full((B, F + 3), 9.0, device=cuda)
    wide_i[:, 2:2 + F] = ids.to(cuda)
    wide_w[:, 1:1 + F] = wts.to(cuda)
    cols = (P + 2) * 64
    buf = torch.full((B + 3, cols + 16), 3.0, dtype=torch.bfloat16, device=cuda)
    packed = ops.din_attention_pack(tuple(t.to(cuda) for t in w))
    x = ops.din_attention(table.to(cuda), wide_i[:, 2:2 + F], wide_w[:, 1:1 + F], P, H, packed, out=buf[:B, 8:8 + cols])
    assert x.data_ptr() == buf[:B, 8:8 + cols].data_ptr()
    check_din(x.cpu(), table, ids, wts, P, W1, w, "v views")
    assert (buf[B:] == 3.0).all() and (buf[:, :8] == 3.0).all() and (buf[:, 8 + cols:] == 3.0).all()


def test_din_model_gpu_vs_cpu(cuda):
    cfg = ModelConfig(family="din", vocab_size=20000, embed_dim=64, mlp_dims=(256, 128))
    m = build_model(cfg, "cpu")
    mg = copy.deepcopy(m).to(cuda)
    ids = torch.randint(0, 10 ** 9, (70, 43))
    wts = torch.rand(70, 43)
    y, yr = mg(ids.to(cuda), wts.to(cuda)).cpu(), m(ids, wts)
    assert torch.allclose(y, yr, rtol=2e-2, atol=5e-3), (y - yr).abs().max()


@pytest.mark.parametrize("P,H,a1,a2,limit", [(3, 65, 80, 40, "H <= 64"), (3, 16, 129, 40, "a1 <= 128")])
def test_din_attention_limits_raise(cuda, P, H, a1, a2, limit):
    table, ids, wts, _, w = din_inputs(4, P, H, a1, a2)
    with pytest.raises(ValueError, match=limit):
        ops.din_attention(table.to(cuda), ids.to(cuda), wts.to(cuda), P, H, tuple(t.to(cuda) for t in w))
