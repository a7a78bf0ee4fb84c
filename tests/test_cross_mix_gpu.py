"""csrc/kernels/cross_mix.hip against the matched fp64 sum-over-experts
reference of tests/test_cross_mix.py, and the DCN-v2 models built on it."""
import copy
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cross_mix import check_close, mix_inputs, mix_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# (d, E, r): one K tile and fewer column blocks than waves; 3 K tiles (< ring
# depth), R = 48 padded to 64; R = 256; the served shape; the most experts
SHAPES = {"one_tile": (64, 1, 64), "pad48": (192, 3, 16), "r256": (192, 2, 128), "served": (2752, 4, 64),
          "e8": (2752, 8, 32)}
CASES = [(1, "one_tile"), (129, "one_tile"), (63, "pad48"), (65, "pad48"), (1, "r256"), (64, "r256"), (129, "r256"),
         (1, "served"), (63, "served"), (65, "served"), (64, "e8"), (129, "e8")]


@pytest.mark.parametrize("M,shape", CASES)
def test_cross_mix_kernel(cuda, M, shape):
    """Both forms of the call within 2^-7 |ref| + 2^-7 rms(ref) of the matched
    reference: the kernel differs from it by fp32 summation order and the tanh /
    exp implementation only, which can flip one bf16 rounding (2^-8 relative)."""
    d, E, r = SHAPES[shape]
    x0, xl, w, b, hw = mix_inputs(M, d, E, r)
    zr, lr = mix_ref(x0, xl, w, b, hw)
    packed = ops.cross_mix_pack(*(t.to(cuda) for t in w))
    z, none = ops.cross_mix(x0.to(cuda), xl.to(cuda), packed, b.to(cuda))
    z2, logit = ops.cross_mix(x0.to(cuda), xl.to(cuda), packed, b.to(cuda), want_z=False, head_w=hw.to(cuda))
    assert none is None and z2 is None and z.shape == (M, d) and logit.shape == (M,)
    check_close(z, zr, f"z M={M} {shape}")
    check_close(logit, lr, f"logit M={M} {shape}")


def test_cross_mix_strided_rows_out_and_nothing_past_m(cuda):
    """Row views of wider buffers for x0 / xl / out, M = 65: the rows of the
    out buffer past M and the columns beside the view keep their sentinel."""
    M, (d, E, r) = 65, SHAPES["pad48"]
    x0, xl, w, b, hw = mix_inputs(M, d, E, r)
    zr, lr = mix_ref(x0, xl, w, b, hw)
    wide = torch.zeros(2, M, d + 64, dtype=torch.bfloat16, device=cuda)
    wide[0, :, :d], wide[1, :, :d] = x0.to(cuda), xl.to(cuda)
    buf = torch.full((M + 63, d + 8), 7.0, dtype=torch.bfloat16, device=cuda)
    z, logit = ops.cross_mix(wide[0, :, :d], wide[1, :, :d], tuple(t.to(cuda) for t in w), b.to(cuda),
                             head_w=hw.to(cuda), out=buf[:M, :d])
    assert z.data_ptr() == buf.data_ptr()
    check_close(buf[:M, :d], zr, "z (strided, out=)")
    check_close(logit, lr, "logit (with z)")
    assert (buf[M:] == 7.0).all() and (buf[:, d:] == 7.0).all()


@pytest.mark.parametrize("experts", [4, 0])
def test_dcn_v2_low_rank_models_gpu_vs_cpu(cuda, experts):
    """The mixture model, and the plain two-GEMM low-rank model beside it."""
    cfg = ModelConfig(family="dcn_v2", cross_experts=experts, cross_rank=64, num_fields=3, vocab_size=1000,
                      mlp_dims=(64, 32))
    m = build_model(cfg, "cpu")
    mg = copy.deepcopy(m).to(cuda)
    g = torch.Generator().manual_seed(11)
    ids, wts = torch.randint(0, 10 ** 9, (70, 3), generator=g), torch.rand(70, 3, generator=g)
    y, yr = mg(ids.to(cuda), wts.to(cuda)).float().cpu(), m(ids, wts).float()
    # the tolerance of test_kernels_gpu.test_models_gpu_vs_cpu
    assert torch.allclose(y, yr, rtol=2e-2, atol=5e-3), (y - yr).abs().max().item()
