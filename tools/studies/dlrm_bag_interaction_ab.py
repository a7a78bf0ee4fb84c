"""A/B of the multi-hot DLRM lookup + interaction on one GPU: the fused
bag-interaction kernel (csrc/kernels/interaction_bag.hip) against the path it
replaces (pack_ids + weight copy + CSR offsets + bag kernel + dot_interaction,
issued as DLRM.lookup / interact_and_top issue them), in one process.

    python -m tools.studies.dlrm_bag_interaction_ab [--rows 20000000] [--out FILE.jsonl]

Shape: B = 16384 candidates, T = 30 tables of --rows rows (the
dlrm_multihot_1gpu preset), hot in {2, 4, 8}, bf16 and fp8 tables, seeded Zipf
ids. Per case: warm-up, then ROUNDS rounds alternating the two paths, each
round ITERS calls between two device events; reported are the median us per
call of each path, the spread of equal runs (max - min of a path's rounds),
the bytes a call moves (from the shapes) and the largest difference between
the two paths' outputs (reordered fp32 sums only). JSON lines. Needs a GPU.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

B, T, D, ND = 16384, 30, 64, 13
ROUNDS, ITERS, WARM = 7, 50, 10


def bytes_moved(hot: int, fp8: bool, out_cols: int) -> dict:
    """HBM bytes per call from the shapes (every table row counted as a miss)."""
    n = B * T * hot
    row = D * (1 if fp8 else 2)
    common = n * row + B * D * 2 + B * out_cols * 2  # table rows + dense in + interaction out
    fused = common + n * (8 + 4)  # int64 ids + fp32 weights, read in place
    # parent: pack_ids (8 in, 4 out), weight copy (4 in, 4 out), offsets (8 out, 8 in), bag (4 + 4 in), pooled out + in
    parent = common + n * (8 + 4 + 4 + 4 + 4 + 4) + 2 * (B * T + 1) * 8 + 2 * B * T * D * 2
    return {"fused": fused, "parent": parent}


def main() -> None:
    import torch

    from distributed_tf_serving_amd import ops
    from distributed_tf_serving_amd.client.synth import SyntheticRequests

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dlrm_bag_interaction_ab: needs a GPU")
    dev = torch.device("cuda:0")
    rows, V = a.rows, T * a.rows
    g = torch.Generator(device=dev).manual_seed(1)
    table = torch.empty(V, D, dtype=torch.bfloat16, device=dev)
    scale = ops.table_scale_fp8(torch.full((T,), 0.125)).to(dev)
    codes = torch.empty(V, D, dtype=torch.float8_e4m3fn, device=dev)
    chunk = 1 << 20
    for r0 in range(0, V, chunk):  # uniform +-1/8, quantised chunk by chunk
        n = min(chunk, V - r0)
        table[r0:r0 + n] = ((torch.rand(n, D, generator=g, device=dev) - 0.5) / 4).to(torch.bfloat16)
        codes[r0:r0 + n] = ops.quant_table_fp8(table[r0:r0 + n], float(scale[0]))
    mod = torch.full((T,), rows, dtype=torch.int64, device=dev)
    off = torch.arange(T, dtype=torch.int64, device=dev) * rows
    cols = ops.interaction_cols(T, D)
    dense = torch.randn(B, D, generator=g, device=dev).to(torch.bfloat16)
    lines = []
    for hot in (2, 4, 8):
        F = ND + T * hot
        ids_np, wts_np = SyntheticRequests(fields=F, id_space=100_000_000, dist="zipf", seed=7).arrays(B)
        ids, wts = torch.from_numpy(ids_np).to(dev), torch.from_numpy(wts_np).float().to(dev)
        col_mod, col_off = mod.repeat_interleave(hot), off.repeat_interleave(hot)
        for fp8 in (False, True):
            def fused():
                if fp8:
                    return ops.dot_interaction_bag_fp8(dense, codes, scale, ids[:, ND:], wts[:, ND:], hot, mod, off, cols)
                return ops.dot_interaction_bag(dense, table, ids[:, ND:], wts[:, ND:], hot, mod, off, cols)

            def parent():  # DLRM.lookup / _lookup_fp8 (int32 rows: V < 2^31) + interact_and_top
                r = ops.pack_ids(ids[:, ND:], modulo_f=col_mod, offset_f=col_off)
                w = wts[:, ND:].float().contiguous().view(-1)
                o = torch.arange(0, B * T * hot + 1, hot, dtype=torch.int64, device=dev)
                if fp8:
                    p = ops.embedding_bag_fp8(codes, scale, r.view(-1), o, per_sample_weights=w, out_bf16=True)
                else:
                    p = ops.embedding_bag(table, r.view(-1), o, per_sample_weights=w, out_bf16=True)
                return ops.dot_interaction(dense, p.view(B, T, D), cols)

            diff = float((fused().float() - parent().float()).abs().max())
            times = {"fused": [], "parent": []}
            for _ in range(WARM):
                fused(), parent()
            for _ in range(ROUNDS):
                for name, fn in (("fused", fused), ("parent", parent)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(ITERS):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / ITERS)
            rec = {"study": "dlrm_bag_interaction_ab", "B": B, "T": T, "rows": rows, "hot": hot,
                   "table": "fp8" if fp8 else "bf16", "max_abs_diff": diff, "bytes": bytes_moved(hot, fp8, cols)}
            for name, ts in times.items():
                ts = sorted(ts)
                rec[name + "_us"] = round(ts[len(ts) // 2], 2)
                rec[name + "_spread_us"] = round(ts[-1] - ts[0], 2)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
