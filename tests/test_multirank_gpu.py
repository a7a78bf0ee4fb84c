"""N > 1 rehearsal on a 1-GPU box: bench.py with 2 and 3 ranks sharing the one
GPU (DTFS_SHARE_GPU: each rank its own RCCL host id, socket transport). This
runs the native fan-out step (two RCCL communicators, ingress / egress
streams), the lockstep live servers and the bounded waits with more than one
rank on real hardware - the path the 8-GPU node runs over xGMI."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_errors(out) -> dict:
    """What tests/cluster_worker.py left behind on failure: each rank's Python
    traceback (rank<r>.err) and its faulthandler dump of every thread on a
    native abort (rank<r>.fault, empty when the rank exited cleanly)."""
    errs = {}
    for f in sorted(out.glob("rank*.err")) + sorted(out.glob("rank*.fault")):
        txt = f.read_text()
        if txt.strip():
            errs[f.name] = txt[-3000:]
    return errs


@pytest.mark.parametrize("n,mode,peer,scatter_path", [
    (2, "alltoall", 0, "shared"), (3, "alltoall", 0, "shared"), (2, "scatter", 0, "shared"),
    (3, "scatter", 0, "shared"), (2, "scatter", 0, "rccl"), (2, "local", 0, "shared"),
    (3, "alltoall", 262144, "shared"), (2, "scatter", 262144, "rccl")])
def test_bench_ranks_sharing_one_gpu(n, mode, peer, scatter_path):
    """peer > 0: the fan-out's exchanges of at most that many bytes per peer go
    through the one-shot peer kernel (csrc/kernels/peer.hip) instead of RCCL.
    Scatter runs both paths: rank 0's shared request arenas (each rank DMAs
    its share, runtime/shared_scatter.h) and the RCCL scatter fallback."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", str(n),
           "--steps", "20", "--warmup", "4", "--prime-steps", "10", "--requests-per-gpu", "4", "--request-rows", "96", "--mode", mode,
           "--pool", "8", "--client-threads", "2", "--qps", "500", "--qps-seconds", "0.4", "--small-buckets", "96",
           "--step-timeout-s", "20", "--scatter-path", scatter_path, "--full"]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100",
               DTFS_PEER_COMM=str(peer))
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == n and out["value"] > 0 and out.get("requests_failed", 0) == 0
    # the BASELINE's second metric at every N, and load-proportional stepping
    assert out["p50_at_fixed_qps_ms"] > 0 and out["fixed_qps"]["errors"] == 0, out.get("fixed_qps")
    assert out["config2_batch512"]["p50_ms"] > 0
    if mode != "local":
        assert out["server"]["idle_steps_per_s"] == 0, out["server"]
        assert "native C++ step" in out["config"]["parallelism"], out["config"]["parallelism"]
    if mode == "alltoall" or (mode == "scatter" and scatter_path == "rccl"):
        assert ("one-shot peer exchange" in out["config"]["parallelism"]) == (peer > 0), out["config"]["parallelism"]
    if mode == "scatter" and scatter_path == "shared":
        # every rank DMA'd only its share of rank 0's batch: 96-row requests, 4
        # per GPU -> each rank copies about the same bytes per step
        per = out["scatter"]["h2d_bytes_per_step_by_rank"]
        assert len(per) == n and min(per) > 0.5 * max(per), per


@pytest.mark.parametrize("n,peer", [(2, 0), (3, 0), (3, 262144)])
def test_bench_dcn_v2_alltoall_ranks_sharing_one_gpu(n, peer):
    """BASELINE config 5 through the candidate fan-out on hardware (verdict r5
    #1/#4): DCN-v2 with fp8 towers, alltoall over n ranks sharing the GPU. Each
    rank's rows cross to the others as narrow exchange rows and feed the fp8
    gather, the quant passes and the split cross path; every bucket's fan-out
    step scores exactly like a local forward at start-up, no request fails."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", str(n),
           "--model", "dcn_v2", "--mode", "alltoall", "--steps", "20", "--warmup", "4", "--prime-steps", "10",
           "--requests-per-gpu", "4", "--request-rows", "96", "--pool", "8", "--client-threads", "2",
           "--qps", "200", "--qps-seconds", "0.4", "--qps-sweep", "", "--small-buckets", "96",
           "--step-timeout-s", "20", "--full"]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100",
               DTFS_PEER_COMM=str(peer))
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == n and out["value"] > 0 and out.get("requests_failed", 0) == 0
    assert "native C++ step" in out["config"]["parallelism"], out["config"]["parallelism"]
    assert out["server"]["idle_steps_per_s"] == 0, out["server"]
    sc = out["self_check"]["buckets"]
    assert len(sc) == 2 and all(b["max_abs_diff"] <= 1e-5 for b in sc), sc


def test_bench_eight_ranks_sharing_one_gpu():
    """The 8-GPU node's world size on hardware (verdict r5 #5): 8 ranks share
    the box's GPU, an 8-rank RCCL communicator pair, the 8-rank step control
    and the alltoall fan-out; every bucket's fan-out step equals a local
    forward on every rank, no request fails, an idle cluster steps nothing.
    (scripts/gpu_rehearsal8.sh runs the scatter / peer-exchange DLRM / DCN-v2
    forms too: profiles/r06_rehearsal8_and_reference.log.)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "8",
           "--steps", "10", "--warmup", "2", "--prime-steps", "5", "--requests-per-gpu", "4", "--request-rows", "64",
           "--pool", "4", "--client-threads", "1", "--qps", "0", "--qps-sweep", "", "--small-buckets", "64",
           "--mode", "alltoall", "--step-timeout-s", "60", "--full"]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="1", DTFS_HANG_DUMP_S="140")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == 8 and out["value"] > 0 and out.get("requests_failed", 0) == 0
    assert "candidate-dp8" in out["config"]["parallelism"] and "native C++ step" in out["config"]["parallelism"]
    assert out["server"]["idle_steps_per_s"] == 0, out["server"]
    assert all(b["max_abs_diff"] <= 1e-5 for b in out["self_check"]["buckets"]), out["self_check"]


@pytest.mark.parametrize("n,peer", [(2, 0), (3, 0), (3, 1 << 20)])
def test_bench_sharded_dlrm_ranks_sharing_one_gpu(n, peer):
    """BASELINE config 4 shape on N ranks: DLRM tables sharded table-wise over
    the ranks, every step a native two-lane step program (ids all-to-all ->
    owner gather -> embeddings all-to-all on the aux lane, bottom MLP on the
    compute lane), checked against the eager forward before the run."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", str(n),
           "--model", "dlrm", "--table-rows", "1000000", "--steps", "20", "--warmup", "4", "--prime-steps", "10",
           "--requests-per-gpu", "4", "--request-rows", "96", "--pool", "8", "--client-threads", "2",
           "--qps", "0", "--step-timeout-s", "20", "--exchange", "alltoall"]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100",
               DTFS_PEER_COMM=str(peer))
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == n and out["value"] > 0 and out.get("requests_failed", 0) == 0
    par = out["config"]["parallelism"]
    assert f"embedding-mp{n}" in par and "native two-lane step program" in par, par
    assert ("one-shot peer exchange" in par) == (peer > 0), par


@pytest.mark.parametrize("n,hot", [(2, 1), (3, 1), (2, 3)])
def test_peer_exchange_ranks_sharing_one_gpu(n, hot):
    """Peer exchange (parallel/hot_cache.py) on N ranks: every rank maps the
    others' table stores by IPC and its lookups load remote rows directly (the
    8-GPU node does the same over xGMI); scores match the unsharded DLRM of the
    same seed through the eager forward and the arena step program, before
    and after the hot-row replica cache fills, and cached rows are hit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "-m", "tools.studies.peer_lookup_check",
           "--hot", str(hot)]
    env = dict(os.environ, DTFS_SHARE_GPU="1")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    ranks = json.loads(line[0])["ranks"]
    assert len(ranks) == n
    tol = 1e-6 if hot == 1 else 2e-3  # one-hot: the same fused kernel as the local model
    for r in ranks:
        assert r["remote_tables"] > 0
        for rnd in r["rounds"]:
            assert rnd["max_abs_diff"] <= tol and rnd["max_abs_diff_arena_program"] <= tol, r["rounds"]
        assert r["rounds"][0]["hits"] == 0 and r["rounds"][-1]["hits"] > 0, r["rounds"]


def test_bench_sharded_dlrm_peer_exchange_ranks_sharing_one_gpu():
    """bench.py --exchange peer on 2 ranks: no collective in the step (the
    ranks' live servers run independently), the replica cache installed
    before the clock, hit rate and xGMI bytes in the JSON."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2",
           "--model", "dlrm", "--table-rows", "1000000", "--steps", "20", "--warmup", "4", "--prime-steps", "10",
           "--requests-per-gpu", "4", "--request-rows", "96", "--pool", "8", "--client-threads", "2",
           "--qps", "0", "--step-timeout-s", "20", "--exchange", "peer", "--hot-cache-rows", "65536"]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    out = json.loads(line[-1])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out.get("requests_failed", 0) == 0
    assert "xGMI" in out["config"]["parallelism"], out["config"]["parallelism"]
    c = out["embedding_exchange"]["hot_row_cache"]
    assert c["hit_rate"] > 0.2 and c["xgmi_bytes_per_step_per_rank"] < out["embedding_exchange"]["bytes_per_step_per_rank"]


@pytest.mark.parametrize("n,mode", [(2, "scatter"), (3, "alltoall")])
def test_native_cluster_server_ranks_sharing_one_gpu(tmp_path, n, mode):
    """serving/cluster.py on N ranks over RCCL: every front door's concurrent
    requests (in-process and gRPC) score like a local forward of the same
    weights, every rank runs the same steps, and an idle cluster runs none."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "tests/cluster_worker.py",
           "--mode", mode, "--out", str(tmp_path), "--grpc-port", str(_port())]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    errs = _rank_errors(tmp_path)
    assert p.returncode == 0, (errs, p.stdout[-2000:], p.stderr[-2000:])
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(n)]
    fronts = [r for r in res if r["serves"]]
    assert len(fronts) == (n if mode == "alltoall" else 1)
    for r in fronts:
        assert r["max_diff"] < 1e-4 and r["grpc_max_diff"] < 1e-4, r
    for r in res:
        assert r["idle_steps"] == 0 and not r["broken"], r
    assert len({r["stats"]["steps"] for r in res}) == 1


def test_cluster_recovers_over_surviving_ranks_sharing_one_gpu(tmp_path):
    """SURVEY §5.3 on hardware: of 3 ranks (RCCL, one shared GPU) rank 2 dies
    after 3 steps; rank 0 answers the affected requests UNAVAILABLE, rebuilds
    the cluster over ranks 0-1 (new communicators, step control, fan-out; same
    processes and weights) and serves correct scores again."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_cluster_server import spawn_ranks  # direct processes: no agent tears the survivors down

    procs, outs = spawn_ranks(3, ["--out", str(tmp_path), "--kill-rank", "2", "--kill-after", "3"],
                              dict(DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100"), timeout=110)
    r0 = json.load(open(tmp_path / "rank0.json")) if (tmp_path / "rank0.json").exists() else None
    assert r0 is not None, [o[-3000:] for o in outs]
    assert procs[2].returncode == 17
    out = r0["outcomes"]
    assert out[0] == "ok" and "UNAVAILABLE" in out and out[-5:] == ["ok"] * 5, out
    assert r0["recoveries"] == 1 and r0["world_after"] == 2 and r0["max_diff"] < 1e-4, r0
    r1 = json.load(open(tmp_path / "rank1.json"))
    assert r1["recoveries"] == 1 and r1["world_after"] == 2, r1


@pytest.mark.parametrize("n", [2, 3])
def test_local_cluster_sharded_dlrm_ranks_sharing_one_gpu(tmp_path, n):
    """BASELINE config 4 served as a cluster on hardware: every rank is a front
    door over the sharded DLRM (tables read where they live through IPC-mapped
    stores, no collective in the step); in-process and gRPC scores equal the
    unsharded model's."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "tests/cluster_worker.py",
           "--mode", "local", "--preset", "dlrm", "--out", str(tmp_path), "--grpc-port", str(_port())]
    env = dict(os.environ, DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    errs = _rank_errors(tmp_path)
    written = sorted(f.name for f in tmp_path.glob("rank*.json"))  # how far the ranks got
    assert p.returncode == 0, (errs, written, p.stdout[-2000:], p.stderr[-4000:])
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(n)]
    for r in res:
        assert r["serves"] and r["max_diff"] < 1e-3 and r["grpc_max_diff"] < 1e-3, r
        assert r["idle_steps"] == 0 and not r["broken"], r
        assert r["threads_after_stop"] == [], r["threads_after_stop"]


def test_local_cluster_dead_table_owner_sharing_one_gpu(tmp_path):
    """A table owner of the peer exchange dies (rank 2 of 3, one shared GPU).
    Its IPC-exported stores stay valid for the importers (the dma-buf import
    holds its own reference to the memory: no GPU fault for the steps already
    in flight), the survivors see the process gone within one watcher period,
    answer UNAVAILABLE, re-plan the tables over ranks 0-1 and serve the
    unsharded model's scores again."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_cluster_server import spawn_launched

    procs, outs = spawn_launched(3, ["--mode", "local", "--preset", "dlrm", "--out", str(tmp_path), "--kill-rank",
                                     "2", "--kill-after", "3"],
                                 dict(DTFS_SHARE_GPU="1", DTFS_HOST_THREADS="2", DTFS_HANG_DUMP_S="100"), timeout=110)
    assert procs[2].returncode == 17, outs[2][-2000:]
    for r in (0, 1):
        f = tmp_path / f"rank{r}.json"
        assert f.exists(), outs[r][-3000:]
        res = json.load(open(f))
        out = res["outcomes"]
        assert "UNAVAILABLE" in out and out[-5:] == ["ok"] * 5, out
        assert res["recoveries"] == 1 and res["world_after"] == 2 and res["max_diff"] < 1e-3, res
