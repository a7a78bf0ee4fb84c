"""A/B of the AutoInt interacting-layer stack at B = 16384, F = 43, D = 64,
heads = 2 (the autoint_1gpu preset's shape) for L = 1 and L = 3 layers: the
fused kernel (ops.autoint, csrc/kernels/autoint.hip, the whole stack in one
launch) against the same stack in torch ops on the GPU. JSON lines.

    python -m tools.studies.autoint_ab [--rows 16384] [--launches 100] [--rounds 6] [--mfma-tflops X] [--out FILE]

Forms: ``fused`` writes y^L and the logit; ``fused_logit_only`` is the model's
call (want_x=False); ``torch_matched`` is the op's contract in torch ops (bf16
matmuls for q, k, v, which round once; fp32 matmuls where the contract keeps
fp32: scores, P V, the residual); ``torch_bf16`` is the stack as plain bf16
torch ops (bf16 bmm outputs: more roundings than the contract, not compared).

Method: HIP events around ``launches`` back-to-back calls after a warm-up, the
forms alternating in one process (in order, then reversed), several rounds; the
figures are the median and the range over the rounds. ``fused`` and
``torch_matched`` are compared once before the timing. ``--mfma-tflops``: the
bf16 16x16x32 rate (random operands) that tools/native/mfma_rate.hip printed on
the same box; the fused kernel's FLOP/s is then also given as a fraction of it.
FLOP = L B 2 F 64 (4 x 64 + 2 F), the unpadded products; bytes = x read + y
written (2 B F 128, half for the logit-only form). Needs a GPU.
"""
import argparse
import json
import statistics

import torch

from distributed_tf_serving_amd import ops
from tools.studies.mlp_tail_fp8_ab import ab


def torch_form(x, layers, heads, w_out, matched=True):
    B, F, D = x.shape
    y = x
    for Wq, Wk, Wv, Wr in layers:
        q, k, v = ((y @ W).view(B, F, heads, D // heads).transpose(1, 2) for W in (Wq, Wk, Wv))
        if matched:
            s = torch.matmul(q.float(), k.float().transpose(-1, -2))
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = torch.matmul(e.bfloat16().float(), v.float()) / e.sum(dim=-1, keepdim=True)
            y = torch.relu(o.transpose(1, 2).reshape(B, F, D) + y.float() @ Wr.float()).bfloat16()
        else:
            p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)).float(), dim=-1).bfloat16()
            y = torch.relu(torch.matmul(p, v).transpose(1, 2).reshape(B, F, D) + y @ Wr)
    return y, (y.float() * w_out).sum(dim=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--mfma-tflops", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autoint_ab measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, F, D, heads = a.rows, 43, 64, 2
    g = torch.Generator().manual_seed(7)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = n(B, F, D).bfloat16().to(dev)
    w_out = (n(F, D) / (D * F) ** 0.5).to(dev)
    sqk = 1.2 / 8 * (D // heads) ** -0.25
    lines = []
    for L in (1, 3):
        layers = [tuple((n(D, D) * s).bfloat16().to(dev) for s in (sqk, sqk, 1 / 8, 1 / 8)) for _ in range(L)]
        packed = ops.autoint_pack(layers, w_out)
        out = torch.empty(B, F, D, dtype=torch.bfloat16, device=dev)
        forms = {"fused": lambda: ops.autoint(x, packed, heads, out=out),
                 "fused_logit_only": lambda: ops.autoint(x, packed, heads, want_x=False),
                 "torch_matched": lambda: torch_form(x, layers, heads, w_out),
                 "torch_bf16": lambda: torch_form(x, layers, heads, w_out, matched=False)}
        (ya, la), (yb, lb) = forms["fused"](), forms["torch_matched"]()
        torch.cuda.synchronize()
        diff = (ya.float() - yb.float()).abs().max().item()
        assert diff <= 2.0 ** -5 * yb.float().abs().max().item(), diff  # bf16 roundings of two summation orders
        ldiff = (la - lb).abs().max().item()
        flop = L * B * 2.0 * F * D * (4 * D + 2 * F)
        for name, v in ab(forms, a.launches, a.rounds).items():
            med = statistics.median(v)
            d = dict(study="autoint_ab", form=name, layers=L, rows=B, F=F, heads=heads, launches=a.launches,
                     rounds=len(v), us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                     tflops_median=round(flop / med / 1e6, 1), max_abs_diff_y=diff, max_abs_diff_logit=ldiff)
            if name.startswith("fused"):
                d["gbytes_per_s"] = round((1 if name == "fused_logit_only" else 2) * B * F * 128 / med / 1e3, 1)
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
