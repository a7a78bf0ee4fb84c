"""A/B of one DCN-v2 cross layer at 16384 x 2752: the mixture-of-experts kernel
(ops.cross_mix, E = 4, r = 64) against the two-launch low-rank layer at
cross_rank = 256 (ops.linear + ops.cross_v2) and the full-rank fp8 layer
(ops.quant_rows_fp8 + ops.cross_gemm_fp8). JSON lines.

    python -m tools.studies.cross_mix_ab [--rows 16384] [--launches 2000] [--rounds 6] [--out FILE]

Method: HIP events around ``launches`` back-to-back layers after a warm-up,
the forms alternating in one process (A B C, then C B A), several rounds; the
figures are the median and the range over the rounds. FLOPs and bytes are
computed from the shapes (bytes: every operand and result once). The three
forms are different models: this compares what a layer costs, not results.
Needs a GPU.
"""
import argparse
import json
import statistics

import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.config import ModelConfig
from distributed_tf_serving_amd.models import build_model
from distributed_tf_serving_amd.models.layers import CrossMix, Dense, make_generator
from tools.studies.mlp_tail_fp8_ab import ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--d", type=int, default=2752)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cross_mix_ab measures on the GPU; none found")
    dev = torch.device("cuda:0")
    M, d, E, r, R2 = a.rows, a.d, 4, 64, 256
    gen = make_generator(7, "cpu")
    bf = torch.bfloat16
    x0 = torch.randn(M, d, generator=gen).to(bf).to(dev)
    xl = torch.randn(M, d, generator=gen).to(bf).to(dev)
    hw = (torch.randn(d, generator=gen) / d ** 0.5).to(dev)

    mix = CrossMix(d, E, r, bf, "cpu", gen).to(dev)
    packed, z_mix = mix.packed(), torch.empty(M, d, dtype=bf, device=dev)
    lv = Dense(d, R2, "none", bf, "cpu", gen).to(dev)
    lu = Dense(R2, d, "none", bf, "cpu", gen).to(dev)
    v_out = torch.empty(M, R2, dtype=bf, device=dev)
    full = Dense(d, d, "none", bf, "cpu", gen, fp8=True).to(dev)
    if not ops.cross_gemm_fits(M, d):
        raise SystemExit(f"the fused fp8 cross GEMM does not take {M} x {d}")

    def fp8_layer():
        q, sx = ops.quant_rows_fp8(xl, ops.FP8_K_PAD)
        return ops.cross_gemm_fp8(q, sx, full.w_fp8, full.w_scale, full.bias, x0, xl)

    forms = {
        "mix_e4_r64": lambda: ops.cross_mix(x0, xl, packed, mix.bias, out=z_mix),
        "mix_e4_r64_logit_only": lambda: ops.cross_mix(x0, xl, packed, mix.bias, want_z=False, head_w=hw),
        "low_rank_256_two_launch": lambda: ops.cross_v2(x0, xl, lu.weight, lu.bias,
                                                        a=ops.linear(xl, lv.weight, lv.bias, out=v_out)),
        "full_rank_fp8": fp8_layer,
    }
    act = 2 * M * d  # bytes of one bf16 [M, d]
    R = E * r
    shape = {
        "mix_e4_r64": (2.0 * M * (d * (2 * R + E) + E * r * r), 3 * act + 2 * (2 * R * d + E * d + E * r * r) + 4 * d),
        "mix_e4_r64_logit_only": (2.0 * M * (d * (2 * R + E) + E * r * r + d),
                                  2 * act + 2 * (2 * R * d + E * d + E * r * r) + 8 * d + 4 * M),
        "low_rank_256_two_launch": (2.0 * M * d * 2 * R2, 4 * act + 2 * 2 * M * R2 + 2 * 2 * R2 * d + 4 * (d + R2)),
        "full_rank_fp8": (2.0 * M * d * d, 4 * act + 2 * M * full.w_fp8.shape[1] + full.w_fp8.numel() + 8 * (M + d)),
    }
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    lines = []
    for name, v in ab(forms, a.launches, a.rounds).items():
        med = statistics.median(v)
        flops, nbytes = shape[name]
        lines.append(dict(study="cross_mix_ab", form=name, rows=M, d=d, launches=a.launches, rounds=len(v),
                          us_median=round(med, 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                          window_ms=round(med * a.launches / 1e3, 1), gflop=round(flops / 1e9, 2),
                          mbytes=round(nbytes / 1e6, 1), tflops=round(flops / med / 1e6, 1),
                          tbytes_per_s=round(nbytes / med / 1e6, 2)))
        print(json.dumps(lines[-1]), flush=True)
    # ---- the eager forward of the two served models (config 5's shape), 3 cross layers each
    base = dict(family="dcn_v2", vocab_size=1_000_000, num_fields=d // 64, embed_dim=64, num_cross_layers=3,
                mlp_dims=(1024, 512, 256))
    models = {"dcn_v2_mix_e4_r64": build_model(ModelConfig(cross_rank=r, cross_experts=E, **base), dev),
              "dcn_v2_fp8": build_model(ModelConfig(gemm_dtype="fp8", **base), dev)}
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1 << 40, (M, d // 64), generator=g).to(dev)
    wts = torch.rand(M, d // 64, generator=g).to(dev)
    fwd = {n: (lambda m=m: m(ids, wts)) for n, m in models.items()}
    for n, f in fwd.items():
        y = f()
        assert torch.isfinite(y).all(), n
    for name, v in ab(fwd, max(50, a.launches // 8), a.rounds).items():
        lines.append(dict(study="cross_mix_ab", what="eager_forward", form=name, rows=M,
                          launches=max(50, a.launches // 8), rounds=len(v), us_median=round(statistics.median(v), 1),
                          us_min=round(min(v), 1), us_max=round(max(v), 1),
                          mscores_per_s=round(M / statistics.median(v), 2)))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
