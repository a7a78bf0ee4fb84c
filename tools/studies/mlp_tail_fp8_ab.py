"""A/B of the fused MLP tail: bf16 (ops.mlp_tail) against MX-fp8 with in-kernel
quantisation (ops.mlp_tail_fp8), on the same h1 at 16384 x 1024, then the
DCN-v2 eager forward with tail_dtype bf16 against fp8. JSON lines.

    python -m tools.studies.mlp_tail_fp8_ab [--rows 16384] [--launches 400] [--out FILE]

Method: HIP events around ``launches`` back-to-back launches after a warm-up,
the two forms alternating in both orders (A B, then B A), several rounds; the
per-form figures are the median and the range over the rounds. Needs a GPU.
"""
import argparse
import copy
import json
import statistics

import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model
from distributed_tf_serving_amd.models.layers import Dense, make_generator


def _time_us(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def ab(forms, launches, rounds):
    """{name: [us per round]}; each round times the forms in order, the next round in reverse."""
    names = list(forms)
    us = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            us[n].append(_time_us(forms[n], launches))
    return us


def _line(what, name, v, **kw):
    return dict(study="mlp_tail_fp8_ab", what=what, form=name, us_median=round(statistics.median(v), 2),
                us_min=round(min(v), 2), us_max=round(max(v), 2), rounds=len(v), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_tail_fp8_ab measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    # ---- the tail kernels on the same h1
    gen = make_generator(7, "cpu")
    l2 = Dense(1024, 512, "relu", torch.bfloat16, "cpu", gen, fp8=True).to(dev)
    l3 = Dense(512, 256, "relu", torch.bfloat16, "cpu", gen, fp8=True).to(dev)
    h1 = torch.relu(torch.randn(a.rows, 1024, generator=gen)).to(torch.bfloat16).to(dev)
    hw = (torch.rand(256, generator=gen) * 0.1 - 0.05).to(dev)
    extra = torch.zeros(11, a.rows, device=dev)  # DCN-v2's partial cross logits
    out = torch.empty(a.rows, device=dev)
    w2p, w3p, w2q, w3q = l2.packed("16"), l3.packed("16"), l2.packed("16f8"), l3.packed("16f8")
    forms = {
        "bf16": lambda: ops.mlp_tail(h1, w2p, l2.bias, "relu", w3p, l3.bias, "relu", hw, 0.0, extra=extra, out=out),
        "fp8": lambda: ops.mlp_tail_fp8(h1, w2q, l2.w_scale, l2.bias, "relu", w3q, l3.w_scale, l3.bias, "relu", hw,
                                        0.0, extra=extra, out=out),
    }
    yb = forms["bf16"]().clone()
    y8 = forms["fp8"]().clone()
    torch.cuda.synchronize()
    flops = 2.0 * a.rows * (1024 * 512 + 512 * 256)
    us = ab(forms, a.launches, a.rounds)
    for n, v in us.items():
        emit(_line("tail_kernel", n, v, rows=a.rows, launches=a.launches,
                   tflops=round(flops / statistics.median(v) / 1e6, 1)))
    emit(dict(study="mlp_tail_fp8_ab", what="tail_kernel_outputs", rows=a.rows,
              max_abs_diff_fp8_vs_bf16=float((y8 - yb).abs().max()), mean_abs_score=float(yb.abs().mean())))

    # ---- DCN-v2 eager forward, same weights
    cfg = ModelConfig(family="dcn_v2", vocab_size=1_000_000, num_fields=43, embed_dim=64, num_cross_layers=3,
                      mlp_dims=(1024, 512, 256), gemm_dtype="fp8")
    c8 = copy.deepcopy(cfg)
    c8.tail_dtype = "fp8"
    mb, m8 = build_model(cfg, dev), build_model(c8, dev)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1 << 40, (a.rows, 43), generator=g).to(dev)
    wts = torch.rand(a.rows, 43, generator=g).to(dev)
    models = {"bf16": lambda: mb(ids, wts), "fp8": lambda: m8(ids, wts)}
    sb, s8 = models["bf16"]().float(), models["fp8"]().float()
    us = ab(models, max(50, a.launches // 4), a.rounds)
    for n, v in us.items():
        emit(_line("dcn_v2_eager_forward", n, v, rows=a.rows, launches=max(50, a.launches // 4)))
    emit(dict(study="mlp_tail_fp8_ab", what="dcn_v2_scores", rows=a.rows,
              max_abs_diff_fp8_vs_bf16=float((s8 - sb).abs().max())))
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
