"""The MX-fp8 fused MLP tail on the GPU (csrc/kernels/mlp_tail_fp8.hip): exact
small-integer cases (tests/exact_cases_fp8_tail.py), random data against the
float64 reference of the op's contract, the DCN-v2 model with tail_dtype fp8
against its own CPU forward and the bf16 tail, and the served preset."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cases_fp8_tail as xt  # noqa: E402

from distributed_tf_serving_amd import ops  # noqa: E402
from distributed_tf_serving_amd.config import ModelConfig, load_preset  # noqa: E402
from distributed_tf_serving_amd.models import build_model  # noqa: E402
from distributed_tf_serving_amd.models.layers import Dense, make_generator  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu_args(c, dev):
    return (c.x.to(dev), ops.pack_bfrag_fp8(c.W2q).to(dev), c.sw2.to(dev), c.b2.to(dev), c.act2,
            ops.pack_bfrag_fp8(c.W3q).to(dev), c.sw3.to(dev), c.b3.to(dev), c.act3, c.hw.to(dev), c.hbias)


# ------------------------------------------------------------------ exact
@pytest.mark.parametrize("case", xt.CASES)
def test_exact_cases(cuda, case):
    """Every sum is an integer (or half-integer) below 2^24 and both MX round
    trips are identities (asserted by the generator): the kernel must give the
    float64 reference bit for bit, twice, and once more into pinned host memory."""
    c = xt.tail_case(*case)
    args = _gpu_args(c, cuda)
    extra = c.extra.to(cuda)[:, :c.M + xt.EXTRA_PAD]  # the [2, M + 37] view: row stride > M
    assert extra.shape[1] > c.M
    y1 = ops.mlp_tail_fp8(*args, extra=extra, sigmoid=False)
    y2 = ops.mlp_tail_fp8(*args, extra=extra, sigmoid=False)
    torch.cuda.synchronize()
    assert y1.dtype == torch.float32 and tuple(y1.shape) == (c.M,)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), "two runs differ"
    got = y1.cpu()
    bad = (got != c.ref).nonzero().flatten()
    assert torch.equal(got, c.ref), (f"{bad.numel()} of {c.M} rows differ, first {bad[:8].tolist()}: "
                                     f"{got[bad[:8]].tolist()} != {c.ref[bad[:8]].tolist()}")
    out = torch.full((c.M,), float("nan")).pin_memory()
    r = ops.mlp_tail_fp8(*args, extra=extra, sigmoid=False, out=out)
    torch.cuda.synchronize()
    assert r is out and torch.equal(out, c.ref)


def test_zero_rows_and_sigmoid(cuda):
    c = xt.tail_case(*xt.CASES[2])
    args = _gpu_args(c, cuda)
    y0 = ops.mlp_tail_fp8(args[0][:0], *args[1:], sigmoid=False)
    assert tuple(y0.shape) == (0,)
    # extra as a plain [M] vector, sigmoid on: against the CPU form of the op
    e1 = c.extra[0, :c.M].contiguous()
    want = ops.mlp_tail_fp8(c.x, c.W2q, c.sw2, c.b2, c.act2, c.W3q, c.sw3, c.b3, c.act3, c.hw * 0.001, 0.25,
                            extra=e1 * 0.125, sigmoid=True)
    got = ops.mlp_tail_fp8(*args[:9], (c.hw * 0.001).to(cuda), 0.25, extra=(e1 * 0.125).to(cuda), sigmoid=True)
    torch.testing.assert_close(got.cpu(), want, atol=1e-6, rtol=1e-6)


def test_binding_rejects_malformed_arguments(cuda):
    c = xt.tail_case(*xt.CASES[3])  # 65 rows
    a = list(_gpu_args(c, cuda))
    ok = dict(extra=None, sigmoid=False)

    def bad(i, v, **kw):
        b = list(a)
        b[i] = v
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            ops.mlp_tail_fp8(*b, **{**ok, **kw})
            torch.cuda.synchronize()

    bad(0, a[0].float())                                    # dtype
    bad(0, torch.zeros(4, 512, dtype=torch.bfloat16, device=cuda))  # K1
    bad(0, torch.zeros(4, 2048, dtype=torch.bfloat16, device=cuda)[:, ::2])  # column stride
    bad(0, torch.zeros(4, 1028, dtype=torch.bfloat16, device=cuda)[:, :1024])  # rows not 16-byte multiples
    bad(0, torch.zeros(4, 1032, dtype=torch.bfloat16, device=cuda)[:, 4:1028])  # misaligned base
    bad(1, a[1].view(torch.uint8))                          # packed dtype
    bad(1, a[1].reshape(-1)[:-16])                          # packed size
    bad(1, a[1].cpu())                                      # device
    bad(5, a[5].reshape(-1)[::2])                           # contiguity / size
    bad(2, a[2][:-1])                                       # sw2 length
    bad(3, a[3].double())                                   # b2 dtype
    bad(6, torch.ones(512, device=cuda))                    # sw3 length
    bad(7, a[7][:128])                                      # b3 length
    bad(9, torch.ones(512, device=cuda))                    # hw length
    bad(4, "sigmoid")                                       # activation
    bad(0, a[0], extra=torch.zeros(2, c.M - 1, device=cuda))  # extra partials shorter than M
    bad(0, a[0], extra=torch.zeros(2, c.M + 4))            # extra on the host
    bad(0, a[0], extra=torch.zeros(c.M + 1, device=cuda))   # extra [M] length
    bad(0, a[0], extra=torch.zeros(2, c.M + 4, device=cuda).double())
    bad(0, a[0], out=torch.zeros(c.M + 1, device=cuda))     # out length
    bad(0, a[0], out=torch.zeros(c.M))                      # out neither device nor pinned
    # a row view with a 16-byte-multiple pitch is fine
    wide = torch.zeros(c.M, 1040, dtype=torch.bfloat16, device=cuda)
    wide[:, 8:1032] = a[0]
    y = ops.mlp_tail_fp8(wide[:, 8:1032], *a[1:], extra=c.extra.to(cuda), sigmoid=False)
    assert torch.equal(y.cpu(), c.ref)


def test_capturable_in_a_graph(cuda):
    c = xt.tail_case(*xt.CASES[4])
    args = _gpu_args(c, cuda)
    extra = c.extra.to(cuda)
    out = torch.zeros(c.M, device=cuda)
    ops.mlp_tail_fp8(*args, extra=extra, sigmoid=False, out=out)  # warm-up outside the capture
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mlp_tail_fp8(*args, extra=extra, sigmoid=False, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), c.ref)


# ------------------------------------------------------------------ random data
def _random_case(M, seed):
    """Xavier weights through Dense(..., fp8=True), x = relu(randn) as bf16."""
    gen = make_generator(seed, "cpu")
    l2 = Dense(1024, 512, "relu", torch.bfloat16, "cpu", gen, fp8=True)
    l3 = Dense(512, 256, "relu", torch.bfloat16, "cpu", gen, fp8=True)
    x = torch.relu(torch.randn(M, 1024, generator=gen)).to(torch.bfloat16)
    hw = (torch.rand(256, generator=gen) * 0.1 - 0.05)
    return SimpleNamespace(M=M, x=x, W2q=l2.w_fp8, sw2=l2.w_scale, b2=l2.bias.data, act2="relu", W3q=l3.w_fp8,
                           sw3=l3.w_scale, b3=l3.bias.data, act3="relu", hw=hw, hbias=0.0,
                           extra=torch.zeros(1, M))


def _code_ulp(q: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 at the code's magnitude (float64): 2^(floor(log2 |q|) - 3), 2^-9 below 2^-6."""
    a = q.abs().clamp_min(2.0 ** -6)
    return torch.exp2(torch.floor(torch.log2(a)) - 3)


def _single_code_effect(c, r) -> torch.Tensor:
    """Per row: the largest change of the logit when one h2 e4m3 code moves one
    step, linearised through h3's ReLU mask: |d logit / d h2q| ulp(code) 2^e."""
    mask = (r.h3 > 0).double() if c.act3 == "relu" else torch.ones_like(r.h3)
    grad = (mask * c.hw.double() * c.sw3.double()) @ c.W3q.double()      # [M, 512]: d logit / d (h2q 2^e)
    scale = torch.exp2(r.e2.double()).repeat_interleave(xt.MX_BLOCK, dim=1)
    h2q = r.h2d / scale
    return (grad.abs() * _code_ulp(h2q) * scale).amax(dim=1)


def check_random(c, got: torch.Tensor, what: str):
    """atol 2e-3 + rtol 2e-3 against the float64 reference (the bf16 tail's own
    bound); a row may exceed it only within 2e-3 + 2 x its largest single-code
    effect (an fp32 h2 that rounds to the neighbouring e4m3 code), and at most
    1 row in 64 (minimum 1) may use that allowance."""
    r = xt.tail_ref(c, parts=True)
    err = (got.double() - r.y).abs()
    plain = 2e-3 + 2e-3 * r.y.abs()
    eff = _single_code_effect(c, r)
    outside = err > plain
    print(f"{what}: M={c.M} max err {err.max():.3e} rows outside plain bound {int(outside.sum())} "
          f"max single-code effect {eff.max():.3e}")
    assert bool((err <= torch.maximum(plain, 2e-3 + 2 * eff)).all()), (what, err.max().item())
    assert int(outside.sum()) <= max(1, c.M // 64), (what, int(outside.sum()))
    return int(outside.sum())


# Observed with these seeds (M = 1 / 65 / 130). The CPU form of the op (fp32)
# against the float64 reference: 0 rows outside the plain bound, worst
# difference 1.4e-7 (asserted below, no GPU kernel involved; 0 of 2048 rows
# too, worst 4.6e-4). The kernel on an MI355X: 0 / 0 / 0 rows outside, worst
# difference 4.8e-7 / 2.3e-3 / 5.9e-4 (the 2.3e-3 row is inside atol + rtol
# |ref|); largest single-code effect 0.012 / 0.027 / 0.037.
@pytest.mark.parametrize("M", [1, 65, 130])
def test_random_data(cuda, M):
    c = _random_case(M, 100 + M)
    cpu = ops.mlp_tail_fp8(c.x, c.W2q, c.sw2, c.b2, c.act2, c.W3q, c.sw3, c.b3, c.act3, c.hw, c.hbias, sigmoid=False)
    assert check_random(c, cpu, "cpu op") == 0
    y = ops.mlp_tail_fp8(*_gpu_args(c, cuda), sigmoid=False)
    check_random(c, y.cpu(), "gpu kernel")


# ------------------------------------------------------------------ model
def test_dcn_v2_fp8_tail_model(cuda):
    cfg = ModelConfig(family="dcn_v2", vocab_size=20000, num_fields=43, embed_dim=64, num_cross_layers=3,
                      mlp_dims=(1024, 512, 256), gemm_dtype="fp8", tail_dtype="fp8")
    m = build_model(cfg, "cpu")
    mg = copy.deepcopy(m).to(cuda)
    cb = copy.deepcopy(cfg)
    cb.tail_dtype = "bf16"
    mb = build_model(cb, "cpu").to(cuda)
    for a, b in zip(m.state_dict().values(), mb.state_dict().values()):
        assert torch.equal(a, b.cpu())
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 10**9, (256, 43), generator=g)
    wts = torch.rand(256, 43, generator=g)
    calls = []
    real = ops.mlp_tail_fp8
    ops.mlp_tail_fp8 = lambda *a, **k: (calls.append(a[0].is_cuda), real(*a, **k))[1]
    try:
        y = mg(ids.to(cuda), wts.to(cuda)).cpu()
        yc = m(ids, wts)
    finally:
        ops.mlp_tail_fp8 = real
    assert calls == [True, False]
    yb = mb(ids.to(cuda), wts.to(cuda)).cpu()
    print(f"fp8 tail GPU vs CPU {(y - yc).abs().max():.3e}, vs bf16 tail {(y - yb).abs().max():.3e}")
    assert (y - yc).abs().max().item() <= 0.05
    assert (y - yb).abs().max().item() <= 0.05


# ------------------------------------------------------------------ served
def test_served_fp8_tail_preset_matches_eager_forward():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.ops import native
    from distributed_tf_serving_amd.serving.server import ModelServer
    from distributed_tf_serving_amd.wire import schema as pb
    from distributed_tf_serving_amd.wire import tensor as T

    cfg = load_preset("dcn_v2_fp8_tail")
    cfg.model.vocab_size = 20000
    cfg.serving.max_batch_rows = 2048
    cfg.serving.allowed_batch_sizes = (256, 2048)
    srv = ModelServer(cfg, device="cuda:0")
    try:
        served = srv.registry.resolve("DCN")
        model = served.model
        assert model.mlp.tail_fp8
        synth = SyntheticRequests(fields=43, id_space=1 << 40, dist="zipf", seed=23)
        for rows in (1, 37, 300, 512):
            ids, wts = synth.arrays(rows)
            data = native().encode_predict_request("DCN", "serving_default", None,
                                                   [("feat_ids", torch.from_numpy(ids)),
                                                    ("feat_wts", torch.from_numpy(wts))], True)
            resp = srv.service.predict_bytes(data, 30.0)
            got = T.to_ndarray(pb.PredictResponse.FromString(resp).outputs["prediction_node"])
            want = model(torch.from_numpy(ids).cuda(), torch.from_numpy(wts).cuda()).float().cpu().numpy()
            print(f"served rows={rows} max diff {np.abs(got - want).max():.3e}")
            np.testing.assert_allclose(got, want, atol=2e-5)
        st = served.scheduler.stats()
        assert not st["broken"]
    finally:
        srv.stop()
