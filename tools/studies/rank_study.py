"""Cost of ranking in the served step (csrc/kernels/rank.hip, serving.rank_on_gpu).

    python -m tools.studies.rank_study kernel   # the kernel against what it replaces
    python -m tools.studies.rank_study step     # the served DeepFM step period with the flag off / on

kernel: ``ops.rank_segments`` on 32 x 512, 11 x 1500 and 1 x 16384 scores
against the only way to do each job without it - one ``ops.sort_scores`` launch
per segment, and ``torch.sort`` (``ops.sort_scores``' own path above 8192) for
the last. HIP events around ``--inner`` back-to-back calls, ``--reps`` such
windows per variant, the two variants alternating; every window is printed.

step: one 16384-row bucket of the served DeepFM, the native load generator
with the same seeded 512-candidate requests in every case, ``--steps`` timed
steps: flag off, flag on with no ranked request, flag on with every request
ranked, and flag off again (the run-to-run spread of the control).

One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def _windows(fn, inner: int) -> float:
    """Microseconds per call over `inner` back-to-back calls (HIP events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def kernel(a) -> None:
    from distributed_tf_serving_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    for S, n in ((32, 512), (11, 1500), (1, 16384)):
        scores = torch.rand(S * n, generator=g).to(dev)
        offsets = torch.arange(0, S * n + 1, n, dtype=torch.int64)
        vals = torch.empty(S * n, device=dev)
        idx = torch.empty(S * n, dtype=torch.int64, device=dev)

        def new():
            # offsets stay on the host (the op validates them there): what a caller pays
            ops.rank_segments(scores, offsets, False, -1, out=(vals, idx))

        if n <= ops.hip().sort_max_elems():
            base_name = f"{S} x ops.sort_scores"

            def base():
                for s in range(S):
                    ops.sort_scores(scores[s * n:(s + 1) * n])
        else:
            base_name = "torch.sort (ops.sort_scores above 8192)"

            def base():
                ops.sort_scores(scores)

        # same results first (faster and different is not faster)
        new()
        for s in range(S):
            v, p = ops.sort_scores(scores[s * n:(s + 1) * n])
            assert torch.equal(v, vals[s * n:(s + 1) * n]) and torch.equal(p, idx[s * n:(s + 1) * n])
        for fn in (new, base):
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        t = {"new": [], "base": []}
        for _ in range(a.reps):
            t["new"].append(_windows(new, a.inner))
            t["base"].append(_windows(base, a.inner))
        _emit(study="rank_kernel", segments=S, scores_per_segment=n, baseline=base_name, inner=a.inner,
              new_us=[round(x, 2) for x in t["new"]], base_us=[round(x, 2) for x in t["base"]],
              new_median_us=round(statistics.median(t["new"]), 2), base_median_us=round(statistics.median(t["base"]), 2))


def step(a) -> None:
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.ops import native
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.server import build_engine

    B, rows, F = 16384, 512, 43
    n_req = B // rows
    synth = SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=5)
    arrays = [synth.arrays(rows) for _ in range(4 * n_req)]

    def pool(flt):
        return [native().encode_predict_request(
            "DCN", "serving_default", None, [("feat_ids", torch.from_numpy(i)), ("feat_wts", torch.from_numpy(w))],
            True, flt) for i, w in arrays]

    plain, ranked = pool([]), pool(["prediction_node", "sorted_prediction", "sorted_index"])
    model = None
    for case, flag, reqs in (("flag_off", False, plain), ("flag_on_no_ranked", True, plain),
                             ("flag_on_all_ranked", True, ranked), ("flag_off_again", False, plain)):
        cfg = load_preset("deepfm_1gpu")
        cfg.serving.max_batch_rows = B
        cfg.serving.allowed_batch_sizes = (B,)
        cfg.serving.rank_on_gpu = flag
        eng = build_engine(cfg, torch.device("cuda", 0), a.slots, model=model)
        model = eng.ex.model  # the same weights in every case
        live = LiveScheduler(eng, cfg.serving, depth=a.slots)
        try:
            conc = (a.slots + 2) * n_req
            st0 = live.stats()
            r = live.run_load(reqs, warmup=a.warmup_steps * n_req, count=a.steps * n_req, concurrency=conc,
                              threads=a.threads, timeout_us=60_000_000)
            st = live.stats()
            steps = st["steps"] - st0["steps"]
            _emit(study="rank_step", case=case, rank_on_gpu=flag, ranks=bool(live.ranks), bucket=B,
                  requests_per_step=n_req, timed_requests=a.steps * n_req, errors=int(r["errors"]),
                  first_error=r["first_error"], window_us=round(r["window_us"], 1),
                  step_period_us=round(r["window_us"] / a.steps, 2),
                  scores_per_s=round(a.steps * B / (r["window_us"] * 1e-6)) if r["window_us"] else 0,
                  steps_total=steps, rows_total=st["rows"] - st0["rows"], ranked=st["ranked"] - st0["ranked"],
                  p50_request_us=round(statistics.median(r["latency_us"]), 1) if len(r["latency_us"]) else None,
                  encode_us_per_step=round((st["encode_us"] - st0["encode_us"]) / max(1, steps), 2),
                  wait_us_per_step=round((st["wait_us"] - st0["wait_us"]) / max(1, steps), 2))
        finally:
            live.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup-steps", type=int, default=40)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--threads", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_study measures on the GPU: none here")
    (kernel if a.what == "kernel" else step)(a)


if __name__ == "__main__":
    main()
