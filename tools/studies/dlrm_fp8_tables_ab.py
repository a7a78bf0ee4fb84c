"""A/B of DLRM embedding storage through the live server: bf16 tables against
fp8 tables (ModelConfig.table_dtype), in the shape bench.py uses for DLRM on
one GPU - 16384-row steps of 32 x 512-candidate requests, 200 timed steps of
one continuous closed loop. JSON lines + a short table.

    python -m tools.studies.dlrm_fp8_tables_ab [--out profiles/dlrm_fp8_tables_ab.jsonl] [--md FILE]

Runs, each a fresh child process under its own ``timeout`` (the study stops at
the first one that fails):

    bf16 tables, 30 x 60M rows, twice (their difference is the run-to-run spread)
    fp8 tables,  30 x 60M rows
    fp8 tables,  30 x 100M rows (BASELINE config 4 on one GPU; bf16 does not fit)

Per run: scores/s and the step period, param_bytes, an fp32 check of one served
request (bf16: bench.py's fp32_check_dlrm_sparse; fp8: fp32 CPU math on the
model's own dequantised rows, only the rows the request references), and the
served scores of a few fixed requests, from which the parent takes the max
|fp8 - bf16| score difference at 60M rows. Needs a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

STUDY = "dlrm_fp8_tables_ab"
RUNS = [("bf16", 60_000_000, "bf16_60m_a"), ("bf16", 60_000_000, "bf16_60m_b"), ("fp8", 60_000_000, "fp8_60m"),
        ("fp8", 100_000_000, "fp8_100m")]


def fp32_check_fp8_sparse(cfg, model, live, request: bytes) -> dict:
    """The fp8 model against fp32 CPU math on its own dequantised rows: only
    the rows the request references leave the GPU (the tables are far too
    large for a CPU copy), the dense towers are copied, the reference math is
    the CPU path of the ops."""
    import torch

    from distributed_tf_serving_amd.models.ctr import DLRM
    from distributed_tf_serving_amd.wire import schema as pb
    from distributed_tf_serving_amd.wire import tensor as wt

    ref = DLRM(cfg, "cpu", materialize_tables=False).eval()
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("emb")},
                        strict=False)
    req = pb.PredictRequest.FromString(request)
    ids = torch.from_numpy(wt.to_ndarray(req.inputs["feat_ids"])).long()
    wts = torch.from_numpy(wt.to_ndarray(req.inputs["feat_wts"])).float()
    nd, Tn = cfg.num_dense, cfg.num_sparse
    B = ids.shape[0]
    rows = torch.remainder(ids[:, nd:], cfg.table_rows) + torch.arange(Tn).view(1, Tn) * cfg.table_rows
    e = model.dequant_rows(rows).cpu().view(B, Tn, cfg.embed_dim).to(torch.bfloat16)  # exact: the values are bf16
    with torch.no_grad():
        want = ref.interact_and_top(ref.bottom_out(wts), e).float()
    resp = pb.PredictResponse.FromString(live.predict_bytes(request, 30.0))
    got = torch.from_numpy(wt.to_ndarray(resp.outputs["prediction_node"]))
    diff = float((got - want).abs().max())
    tol = 2e-2
    return {"status": "ok" if diff <= tol else "MISMATCH", "max_abs_diff": round(diff, 6), "tol": tol,
            "rows": int(got.numel()), "reference": f"sparse: {B * Tn} referenced table rows dequantised from the store"}


def child(a) -> None:
    import numpy as np
    import torch

    import bench
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import ServingConfig, load_preset
    from distributed_tf_serving_amd.models import build_model
    from distributed_tf_serving_amd.parallel.dist import init_from_env, shutdown
    from distributed_tf_serving_amd.parallel.fanout import FanoutEngine
    from distributed_tf_serving_amd.serving.arena import ArenaLayout
    from distributed_tf_serving_amd.serving.executor import ShardExecutor
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.packing import PackedLayout
    from distributed_tf_serving_amd.utils.gc_tuning import tune_for_serving
    from distributed_tf_serving_amd.wire import schema as pb
    from distributed_tf_serving_amd.wire import tensor as wt

    os.environ.setdefault("DTFS_HOST_THREADS", "4")
    ctx = init_from_env()
    dev = ctx.device
    gpu = dev.type == "cuda"
    if not gpu and not a.tryout:  # a CPU run only tries the script out (--scale-rows): its times mean nothing
        raise SystemExit("dlrm_fp8_tables_ab measures on the GPU; none found")
    torch.manual_seed(1234)
    cfg = load_preset("dlrm_sharded8").model
    cfg.table_rows, cfg.table_dtype = a.table_rows, a.table_dtype
    model = build_model(cfg, dev)
    F, R, n_req, slots = cfg.num_fields, a.request_rows, a.requests_per_step, 4
    B = R * n_req
    buckets = sorted({2048, B})
    ex = ShardExecutor(model, PackedLayout(F), buckets, dev, use_graphs=True, slots=slots)
    eng = FanoutEngine(ex, ctx, mode="local", ingest="arena", arena=ArenaLayout(F, max_rows=B, gpu_varint=True))
    for b in buckets:
        eng.prepare(b)
    synth = SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=1000, weights="uniform")
    pool = [synth.serialized(R, raw=True) for _ in range(64)]
    sc = ServingConfig(max_batch_rows=B, allowed_batch_sizes=tuple(buckets), batch_timeout_us=200,
                       max_queued_rows=1 << 24, max_request_rows=1 << 20)
    live = LiveScheduler(eng, sc, buckets=buckets, depth=slots, step_timeout_s=a.step_timeout_s, narrow=True,
                         peer_timeout_s=a.step_timeout_s)
    tune_for_serving()
    if gpu:
        torch.cuda.synchronize(dev)
    r = live.run_load(pool, warmup=(a.prime_steps + a.warmup) * n_req, count=a.steps * n_req,
                      concurrency=(slots + 2) * n_req, threads=8, timeout_us=int(a.step_timeout_s * 1e6))
    window_s = r["window_us"] * 1e-6
    line = dict(study=STUDY, run=a.name, table_dtype=cfg.table_dtype, tables=cfg.num_sparse, table_rows=cfg.table_rows,
                step_rows=B, steps=a.steps, warmup=a.warmup, prime_steps=a.prime_steps, requests_failed=int(r["errors"]),
                param_bytes=int(model.param_bytes()), supports_arena=bool(model.supports_arena),
                device=torch.cuda.get_device_name(dev) if gpu else "cpu",
                hbm_allocated_bytes=int(torch.cuda.max_memory_allocated(dev)) if gpu else 0)
    if not r["errors"] and window_s > 0:
        line.update(scores_per_s=round(B * a.steps / window_s, 1), us_per_step=round(window_s / a.steps * 1e6, 2))
    if cfg.table_dtype == "fp8":
        line["fp32_check"] = fp32_check_fp8_sparse(cfg, model, live, pool[0])
    else:
        line["fp32_check"] = bench.fp32_check_dlrm_sparse(cfg, model, live, pool[0])
    scores = [wt.to_ndarray(pb.PredictResponse.FromString(live.predict_bytes(q, 30.0)).outputs["prediction_node"])
              for q in pool[:a.compare_requests]]
    np.save(a.scores, np.concatenate(scores).astype(np.float32))
    line["broken"] = bool(live.stats()["broken"])
    live.close()
    print(json.dumps(line), flush=True)
    shutdown()
    if r["errors"] or line["broken"] or line["fp32_check"]["status"] != "ok":
        raise SystemExit(3)


def table(lines) -> str:
    runs = {d["run"]: d for d in lines if "run" in d}
    out = ["# DLRM fp8 embedding tables vs bf16 (live server, 16384-row steps, one MI355X)", "",
           "Raw lines: `profiles/dlrm_fp8_tables_ab.jsonl` (`python -m tools.studies.dlrm_fp8_tables_ab`).", "",
           "| run | tables | param_bytes | scores/s | us/step | fp32 check (max abs diff) |", "|---|---|---|---|---|---|"]
    for d in runs.values():
        sps = f"{d['scores_per_s']:,}" if "scores_per_s" in d else "n/a"
        out.append(f"| {d['run']} | {d['tables']} x {d['table_rows']:,} {d['table_dtype']} | {d['param_bytes']:,} | "
                   f"{sps} | {d.get('us_per_step', 'n/a')} | "
                   f"{d['fp32_check']['status']} ({d['fp32_check']['max_abs_diff']}) |")
    out.append("")
    for d in lines:
        if d.get("what") == "summary":
            out += [f"- bf16 run-to-run spread at 60M rows: {d['bf16_spread_pct']} % of the step period.",
                    f"- fp8 vs bf16 at 60M rows: {d['fp8_vs_bf16_pct']:+} % scores/s"
                    + (" - slower than bf16 by more than the spread." if d["fp8_slower_than_spread"]
                       else " - not slower than bf16 beyond the spread."),
                    f"- max |fp8 - bf16| served score on the same {d['compared_scores']} candidates: "
                    f"{d['max_abs_score_diff_fp8_vs_bf16']:.2e} (the quantisation error of the tables; "
                    f"bf16 run a vs run b: {d['max_abs_score_diff_bf16_a_vs_b']:.2e})."]
            if "fp8_100m_param_bytes" in d:
                out.append(f"- 30 x 100M rows in fp8: param_bytes {d['fp8_100m_param_bytes']:,} "
                           f"({d['fp8_100m_param_bytes'] / 1e9:.1f} GB) on one GPU.")
    out += ["", "Method: one GPU, the runs back to back in fresh processes; each builds its tables, captures its steps and",
            "serves the priming, warm-up and timed steps (32 x 512-candidate requests per 16384-row step) in one closed",
            "loop. The fp8 step reads 64-byte rows where the bf16 step reads 128-byte ones; the rest of the step (bottom",
            "MLP, top MLP, head, the request copy) is the same code. `hbm_allocated_bytes` in the raw lines is the torch",
            "allocator's peak. bf16 tables at 100M rows (384 GB) do not fit one GPU, so that size has no bf16 row."]
    return "\n".join(out) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", STUDY + ".jsonl"))
    ap.add_argument("--md", default=os.path.join(REPO, "profiles", STUDY + ".md"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--prime-steps", type=int, default=1000)
    ap.add_argument("--request-rows", type=int, default=512)
    ap.add_argument("--requests-per-step", type=int, default=32)
    ap.add_argument("--compare-requests", type=int, default=8)
    ap.add_argument("--step-timeout-s", type=float, default=30.0)
    ap.add_argument("--run-timeout-s", type=int, default=420, help="wall limit of one run (a child process)")
    ap.add_argument("--runs", default=",".join(n for _, _, n in RUNS), help="subset of the runs, by name")
    ap.add_argument("--scale-rows", type=float, default=1.0, help="scale every run's table rows (a small try-out)")
    # child mode
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tryout", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--name", default="", help=argparse.SUPPRESS)
    ap.add_argument("--table-dtype", default="bf16", help=argparse.SUPPRESS)
    ap.add_argument("--table-rows", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--scores", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    import numpy as np

    lines, scores = [], {}
    want = set(a.runs.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, open(a.out, "w") as f:
        for dtype, rows, name in RUNS:
            if name not in want:
                continue
            path = os.path.join(tmp, name + ".npy")
            cmd = ["timeout", "-k", "10", str(a.run_timeout_s), sys.executable, "-m", "tools.studies." + STUDY, "--child",
                   "--name", name, "--table-dtype", dtype, "--table-rows", str(max(1000, int(rows * a.scale_rows))),
                   "--scores", path, "--steps", str(a.steps), "--warmup", str(a.warmup), "--prime-steps",
                   str(a.prime_steps), "--request-rows", str(a.request_rows), "--requests-per-step",
                   str(a.requests_per_step), "--compare-requests", str(a.compare_requests), "--step-timeout-s",
                   str(a.step_timeout_s)] + (["--tryout"] if a.scale_rows != 1.0 else [])
            p = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, text=True)
            got = [json.loads(s) for s in p.stdout.splitlines() if s.startswith("{")]
            for d in got:
                lines.append(d)
                f.write(json.dumps(d) + "\n")
                f.flush()
                print(json.dumps(d), flush=True)
            if p.returncode != 0 or not got:  # a failed, hung or faulted run: nothing more starts on the GPU
                d = dict(study=STUDY, what="stopped", run=name, exit_status=p.returncode)
                f.write(json.dumps(d) + "\n")
                print(json.dumps(d), flush=True)
                raise SystemExit(f"run {name} failed (exit status {p.returncode}); stopping")
            scores[name] = np.load(path)
        runs = {d["run"]: d for d in lines}
        if {"bf16_60m_a", "bf16_60m_b", "fp8_60m"} <= set(runs):
            ua, ub, u8 = (runs[n]["us_per_step"] for n in ("bf16_60m_a", "bf16_60m_b", "fp8_60m"))
            u16 = (ua + ub) / 2
            spread = abs(ua - ub) / u16 * 100
            delta = (u16 / u8 - 1) * 100
            d = dict(study=STUDY, what="summary", bf16_us_per_step=[ua, ub], fp8_us_per_step=u8,
                     bf16_spread_pct=round(spread, 2), fp8_vs_bf16_pct=round(delta, 2),
                     fp8_slower_than_spread=bool(u8 > max(ua, ub) and (u8 / u16 - 1) * 100 > spread),
                     compared_scores=int(scores["fp8_60m"].size),
                     max_abs_score_diff_fp8_vs_bf16=float(np.abs(scores["fp8_60m"] - scores["bf16_60m_a"]).max()),
                     max_abs_score_diff_bf16_a_vs_b=float(np.abs(scores["bf16_60m_b"] - scores["bf16_60m_a"]).max()))
            if "fp8_100m" in runs:
                d["fp8_100m_param_bytes"] = runs["fp8_100m"]["param_bytes"]
            lines.append(d)
            f.write(json.dumps(d) + "\n")
            print(json.dumps(d), flush=True)
    with open(a.md, "w") as f:
        f.write(table(lines))


if __name__ == "__main__":
    main()
