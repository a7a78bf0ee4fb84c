"""A/B of one xDeepFM CIN layer at B = 16384 for both layers of the xdeepfm_1gpu
preset (F = 43, D = 64, H = 128; layer 1: H_prev = 43, layer 2: H_prev = 128):
the fused kernel (ops.cin_layer, csrc/kernels/cin.hip) against the same math in
torch ops on the GPU, chunked over B so that the materialised outer product
[chunk, H_prev, F, 64] stays near 0.35 GB. JSON lines.

    python -m tools.studies.cin_ab [--rows 16384] [--launches 100] [--rounds 6] [--mfma-tflops X] [--out FILE]

Method: HIP events around ``launches`` back-to-back calls after a warm-up, the
two forms alternating in one process (A B, then B A), several rounds; the
figures are the median and the range over the rounds. Both forms compute the
same xk and logit (compared once before the timing). ``--mfma-tflops``: the
bf16 16x16x32 rate (random operands) that tools/native/mfma_rate.hip printed on
the same box; the fused kernel's FLOP/s is then also given as a fraction of it.
FLOP = 2 B 64 H_prev F H, the unpadded GEMM. Needs a GPU.
"""
import argparse
import json
import statistics

import torch

from distributed_tf_serving_amd import ops
from tools.studies.mlp_tail_fp8_ab import ab


def torch_form(x0, xp, W, bias, w_out, chunk):
    """ops.cin_layer's contract in torch ops: the bf16 product is the single rounding of Z."""
    B, F, D = x0.shape
    H, Hp, _ = W.shape
    Wm = W.reshape(H, Hp * F)
    xk = torch.empty(B, H, D, dtype=torch.bfloat16, device=x0.device)
    for s in range(0, B, chunk):
        z = (xp[s:s + chunk, :, None] * x0[s:s + chunk, None]).reshape(-1, Hp * F, D)
        xk[s:s + chunk] = (torch.matmul(Wm, z).float() + bias.view(1, -1, 1)).to(torch.bfloat16)
    return xk, xk.float().sum(2) @ w_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--mfma-tflops", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cin_ab measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, F, D, H = a.rows, 43, 64, 128
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, F, D, generator=g).bfloat16().to(dev)
    lines = []
    for layer, Hp in ((1, F), (2, H)):
        xp = x0 if layer == 1 else torch.randn(B, Hp, D, generator=g).bfloat16().to(dev)
        W = (torch.randn(H, Hp, F, generator=g) / (Hp * F) ** 0.5).bfloat16().to(dev)
        bias, w_out = (torch.randn(H, generator=g) * 0.1).to(dev), (torch.randn(H, generator=g) / H ** 0.5).to(dev)
        packed = ops.cin_pack(W)
        out = torch.empty(B, H, D, dtype=torch.bfloat16, device=dev)
        chunk = max(1, (350 << 20) // (Hp * F * D * 2))
        forms = {"fused": lambda: ops.cin_layer(x0, xp, packed, bias, w_out, out=out),
                 "torch_chunked": lambda: torch_form(x0, xp, W, bias, w_out, chunk)}
        (xa, la), (xb, lb) = forms["fused"](), forms["torch_chunked"]()
        torch.cuda.synchronize()
        diff = (xa.float() - xb.float()).abs().max().item()
        assert diff <= 2.0 ** -6 * xb.float().abs().max().item(), diff  # bf16 roundings of two summation orders
        ldiff = (la - lb).abs().max().item()
        flop = 2.0 * B * D * Hp * F * H
        for name, v in ab(forms, a.launches, a.rounds).items():
            med = statistics.median(v)
            d = dict(study="cin_ab", form=name, layer=layer, rows=B, F=F, H_prev=Hp, H=H, launches=a.launches,
                     rounds=len(v), us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                     tflops_median=round(flop / med / 1e6, 1), max_abs_diff_xk=diff, max_abs_diff_logit=ldiff)
            if a.mfma_tflops > 0:
                d["mfma_probe_tflops"] = a.mfma_tflops
                d["fraction_of_mfma_probe"] = round(flop / med / 1e6 / a.mfma_tflops, 3)
            lines.append(d)
            print(json.dumps(d), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
