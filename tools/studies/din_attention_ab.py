"""A/B of the DIN target attention at B = 16384, P = 26, H = 16 and H = 50: the
fused kernel (ops.din_attention, csrc/kernels/din_attention.hip) against the
unfused composition, ops.embed into a [B, F, 64] buffer plus the attention
unit in torch ops on the GPU. JSON lines.

    python -m tools.studies.din_attention_ab [--rows 16384] [--launches 300] [--rounds 6] [--out FILE]

Method: HIP events around ``launches`` back-to-back calls after a warm-up, the
two forms alternating in one process (A B, then B A), several rounds; the
figures are the median and the range over the rounds. Both forms compute the
same x (compared once before the timing). Needs a GPU.
"""
import argparse
import json
import statistics

import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.models.layers import DinAttention, make_generator
from tools.studies.mlp_tail_fp8_ab import ab


def composition(table, ids, wts, P, H, att):
    """The contract of ops.din_attention in separate launches."""
    Wq, Wk, Wp, b1, al1, W2, b2, al2, w3, b3 = att.raw()
    B, bf = ids.shape[0], torch.bfloat16
    x, _ = ops.embed(table, ids, wts, modulo=table.shape[0], want_x=True)
    e = x.view(B, P + 1 + H, 64)
    q, k = e[:, P], e[:, P + 1:]
    p = (q.float().unsqueeze(1) * k.float()).to(bf)
    z1 = (torch.matmul(k, Wk.t()).float() + torch.matmul(p, Wp.t()).float()
          + (torch.matmul(q, Wq.t()).float() + b1).unsqueeze(1))
    a1 = torch.where(z1 > 0, z1, al1 * z1).to(bf)
    z2 = torch.matmul(a1, W2.t()).float() + b2
    s = torch.where(z2 > 0, z2, al2 * z2) @ w3 + b3
    v = (s.unsqueeze(-1) * k.float()).sum(1).to(bf)
    return torch.cat([x[:, :(P + 1) * 64], v], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("din_attention_ab measures on the GPU; none found")
    dev = torch.device("cuda:0")
    B, P, V = a.rows, 26, 1_000_000
    gen = make_generator(7, "cpu")
    table = (torch.randn(V, 64, generator=gen) * 0.125).bfloat16().to(dev)
    att = DinAttention(64, (80, 40), torch.bfloat16, "cpu", gen).to(dev)
    lines = []
    for H in (16, 50):
        F = P + 1 + H
        ids = torch.randint(0, 1 << 40, (B, F), generator=gen).to(dev)
        wts = torch.rand(B, F, generator=gen).to(dev)
        out = torch.empty(B, (P + 2) * 64, dtype=torch.bfloat16, device=dev)
        packed = att.packed()
        forms = {"fused": lambda: ops.din_attention(table, ids, wts, P, H, packed, out=out),
                 "embed_plus_torch_ops": lambda: composition(table, ids, wts, P, H, att)}
        xa, xb = forms["fused"]().float(), forms["embed_plus_torch_ops"]().float()
        torch.cuda.synchronize()
        diff = (xa - xb).abs().max().item()
        assert diff <= 2.0 ** -6 * xb.abs().max().item(), diff  # bf16 roundings of two summation orders
        moved = B * (F * 128 + F * 12 + (P + 2) * 128)  # rows, ids + weights, x: each once
        for name, v in ab(forms, a.launches, a.rounds).items():
            med = statistics.median(v)
            lines.append(dict(study="din_attention_ab", form=name, rows=B, P=P, H=H, launches=a.launches,
                              rounds=len(v), us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                              mbytes_min=round(moved / 1e6, 1), max_abs_diff=diff))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
