"""Cost of top-k outputs (csrc/kernels/topk.hip, served with serving.rank_on_gpu).

    python -m tools.studies.topk_study kernel   # selection against the full network
    python -m tools.studies.topk_study step     # the served DeepFM step: plain / sorted_* / top-k requests

kernel: ``ops.topk_segments`` against ``ops.rank_segments(descending=True, k)``
(the full network of csrc/kernels/rank.hip, the only way to the same k entries
before) on 32 x 512 (k = 50), 11 x 1500 (k = 100), 1 x 4097 and 1 x 8192
(k = 100: the shortest segments that are selected) and 1 x 16384 (k = 100 and
k = 1024) scores, uniform random and sigmoid-shaped. The first k entries of
every segment are checked equal before anything is timed. HIP events around
``--inner`` back-to-back calls, ``--reps`` such windows per variant, the two
variants alternating; every window is printed.

step: one 16384-row bucket of the served DeepFM, the native load generator
with the same seeded 512-candidate requests in every case, ``--steps`` timed
steps, rank_on_gpu on throughout: no ranked request (control), every request
asking for prediction_node + sorted_prediction + sorted_index, every request
asking for top_prediction + top_index with k = 50, and the control again (the
run-to-run spread).

One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from .rank_study import _windows


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def _scores(dist: str, n: int, g: torch.Generator) -> torch.Tensor:
    if dist == "uniform":
        return torch.rand(n, generator=g)
    return torch.sigmoid(torch.randn(n, generator=g) * 0.5 - 2.0)  # CTR-like: most scores near 0.1


def kernel(a) -> None:
    from distributed_tf_serving_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    for dist in ("uniform", "sigmoid"):
        for S, n, k in ((32, 512, 50), (11, 1500, 100), (1, 4097, 100), (1, 8192, 100), (1, 16384, 100),
                        (1, 16384, 1024)):
            scores = _scores(dist, S * n, g).to(dev)
            offsets = torch.arange(0, S * n + 1, n, dtype=torch.int64)
            ks = torch.full((S,), k, dtype=torch.int64)
            vals, idx = torch.empty(S * n, device=dev), torch.empty(S * n, dtype=torch.int64, device=dev)
            bvals, bidx = torch.empty(S * n, device=dev), torch.empty(S * n, dtype=torch.int64, device=dev)

            def new():
                # offsets and k stay on the host (the op validates them there): what a caller pays
                ops.topk_segments(scores, offsets, ks, out=(vals, idx))

            def base():
                ops.rank_segments(scores, offsets, True, k, out=(bvals, bidx))

            # same results first (faster and different is not faster)
            new()
            base()
            for s in range(S):
                assert torch.equal(idx[s * n:s * n + k], bidx[s * n:s * n + k])
                assert torch.equal(vals[s * n:s * n + k], bvals[s * n:s * n + k])
            for fn in (new, base):
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            t = {"new": [], "base": []}
            for _ in range(a.reps):
                t["new"].append(_windows(new, a.inner))
                t["base"].append(_windows(base, a.inner))
            _emit(study="topk_kernel", dist=dist, segments=S, scores_per_segment=n, k=k,
                  path="select" if n > ops.hip().topk_select_min() and k <= ops.hip().topk_select_max()
                  else "full network",
                  baseline="ops.rank_segments(descending, k)", inner=a.inner,
                  new_us=[round(x, 2) for x in t["new"]], base_us=[round(x, 2) for x in t["base"]],
                  new_median_us=round(statistics.median(t["new"]), 2),
                  base_median_us=round(statistics.median(t["base"]), 2))


def step(a) -> None:
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.config import load_preset
    from distributed_tf_serving_amd.ops import native
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.server import build_engine

    B, rows, F, K = 16384, 512, 43, 50
    n_req = B // rows
    synth = SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=5)
    arrays = [synth.arrays(rows) for _ in range(4 * n_req)]

    def pool(flt, k=None):
        extra = [("top_k", torch.tensor([k], dtype=torch.int64))] if k is not None else []
        return [native().encode_predict_request(
            "DCN", "serving_default", None,
            [("feat_ids", torch.from_numpy(i)), ("feat_wts", torch.from_numpy(w)), *extra], True, flt)
            for i, w in arrays]

    plain = pool([])
    ranked = pool(["prediction_node", "sorted_prediction", "sorted_index"])
    top = pool(["top_prediction", "top_index"], K)
    model = None
    for case, reqs in (("control", plain), ("all_sorted", ranked), ("all_top_k", top), ("control_again", plain)):
        cfg = load_preset("deepfm_1gpu")
        cfg.serving.max_batch_rows = B
        cfg.serving.allowed_batch_sizes = (B,)
        cfg.serving.rank_on_gpu = True
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
            _emit(study="topk_step", case=case, ranks=bool(live.ranks), bucket=B, k=K if reqs is top else None,
                  requests_per_step=n_req, timed_requests=a.steps * n_req, errors=int(r["errors"]),
                  first_error=r["first_error"], window_us=round(r["window_us"], 1),
                  step_period_us=round(r["window_us"] / a.steps, 2),
                  scores_per_s=round(a.steps * B / (r["window_us"] * 1e-6)) if r["window_us"] else 0,
                  steps_total=steps, rows_total=st["rows"] - st0["rows"], ranked=st["ranked"] - st0["ranked"],
                  topk=st["topk"] - st0["topk"],
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
        raise SystemExit("topk_study measures on the GPU: none here")
    (kernel if a.what == "kernel" else step)(a)


if __name__ == "__main__":
    main()
