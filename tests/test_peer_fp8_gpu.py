"""The peer lookup on fp8 tables on the GPU (csrc/kernels/peer_lookup_fp8.hip):
two stores of e4m3 codes on one GPU stand in for two ranks (tests/
peer_fp8_cases.py). The fused kernel, the bags and the cache fill against the
local fp8 kernel on the concatenated store, the bf16 peer kernels on the
dequantised stores and the CPU twin - bit for bit wherever the format allows -
the arena form, refreshes under running lookups, the bindings' rejections and
two ranks sharing the GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_fp8_cases as pc  # noqa: E402

from distributed_tf_serving_amd import ops  # noqa: E402
from distributed_tf_serving_amd.parallel.hot_cache import KEY_SHIFT, HotRowCache  # noqa: E402

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 4096


def _bits(x):
    return x.cpu().view(torch.int16)


def _stores(T, seed=3):
    g = torch.Generator().manual_seed(seed + T)
    ts = pc.TwoStores(T, ROWS, pc.remote_half(T), g)
    planted = [(ts.remote[-1], ROWS - 1)]  # one remote row ..
    local = [t for t in range(T) if t not in ts.remote]
    if local:
        planted.append((local[-1], 517))  # .. and one local row hold every code extreme
    for t, r in planted:
        ts.plant(t, r, pc.EXTREMES.repeat(8))
    return ts, planted, g


@pytest.mark.parametrize("chunk_shift", [None, 9])
@pytest.mark.parametrize("T,B,ids64", [(1, 1, True), (1, 517, False), (6, 1, False), (6, 517, True), (31, 1, True),
                                       (31, 517, False)])
def test_fused_kernel(cuda, chunk_shift, T, B, ids64):
    """dot_interact_gather_peer_fp8_kernel == the local fp8 kernel on the
    concatenated code store == the bf16 peer kernel on the dequantised stores,
    bit for bit, before a refresh (all misses) and after (hits); counters, ring
    pushes, hot keys and the cached bytes are the CPU twin's."""
    ts, planted, g = _stores(T)
    col0 = 3
    full = pc.skewed(B, col0 + T, g, hot_ids=64)
    for i, (t, r) in enumerate(planted):  # negative ids onto the planted rows
        if i < B:
            full[i, col0 + t] = r - 7 * ROWS
    fi = full if ids64 else full.to(torch.int32)
    assert (fi < 0).any() or B == 1
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16)
    p8, p16, pcpu = ts.peer_fp8(chunk_shift, cuda), ts.peer_bf16(chunk_shift, cuda), ts.peer_fp8(chunk_shift)
    if chunk_shift:
        assert len(p8.stores[0]) == T * ROWS >> 9 and p8.stores[0][1].data_ptr() - p8.stores[0][0].data_ptr() == 64 << 9
    # capacity: 0.75 x 4096 slots hold every sampled key (<= 259 x 15), so the hot set has no ties to break
    c8, c16, cc = (HotRowCache(p, capacity=4096, ring_cap=1 << 14, sample_every=2) for p in (p8, p16, pcpu))
    assert c8.rows.dtype == F8 and c8.rows.is_cuda
    q, mod, off = ts.local()
    dc, ic = dense.to(cuda), fi.to(cuda)
    zl = ops.dot_interaction_gather_fp8(dc, q.to(cuda), ts.scale.to(cuda), ic[:, col0:], mod.to(cuda), off.to(cuda))
    used = 64 + (T + 1) * T // 2
    for rnd in range(2):
        for c in (c8, c16, cc):
            c.reset_counts()
        z8 = ops.dot_interaction_gather_peer(dc, ic, p8, c8, id_col0=col0)
        z16 = ops.dot_interaction_gather_peer(dc, ic, p16, c16, id_col0=col0)
        zr = ops.dot_interaction_gather_peer(dense, fi, pcpu, cc, id_col0=col0)
        torch.cuda.synchronize()
        assert z8.dtype == torch.bfloat16 and z8.shape == zl.shape == (B, ops.interaction_cols(T, 64))
        assert torch.equal(_bits(z8), _bits(zl)), f"round {rnd}: vs the local fp8 kernel"
        assert torch.equal(_bits(z8), _bits(z16)), f"round {rnd}: vs the bf16 peer kernel"
        assert (z8[:, used:] == 0).all() and torch.equal(z8[:, :64].cpu(), dense)
        assert (z8.float().cpu() - zr.float()).abs().max().item() < 2e-2 * max(1.0, zr.float().abs().max().item())
        assert c8.counts() == c16.counts() == cc.counts()
        assert sum(cc.counts()) == (B // 2) * len(ts.remote)  # every 2nd candidate counted
        assert int(c8.ring_ctr.sum()) == int(c16.ring_ctr.sum()) == int(cc.ring_ctr.sum()) == -(-B // 2) * len(ts.remote)
        if rnd == 0:
            assert c8.counts()[0] == 0
            assert c8.refresh() > 0 and c16.refresh() > 0 and cc.refresh() > 0
            assert torch.equal(c8.keys.cpu(), cc.keys) and c8.slots.unique().numel() == cc.keys.numel()
            # the fill: every cached row is its owner's 64 code bytes
            kt, kv = cc.keys >> KEY_SHIFT, cc.keys & ((1 << KEY_SHIFT) - 1)
            assert torch.equal(c8.rows.view(torch.uint8)[c8.slots.long()].cpu(), pcpu.row_cpu(kt, kv).view(torch.uint8))
            assert (ts.remote[-1] << KEY_SHIFT) + ROWS - 1 in cc.keys.tolist()  # the remote extremes row is cached
        elif B > 1:
            assert c8.counts()[0] > 0


@pytest.mark.parametrize("T", [5, 31])
def test_fused_kernel_exact_small_integers(cuda, T):
    """Rounding-free inputs (tests/test_peer_fp8_cpu.py shows they are): the
    output equals the fp32 CPU reference rounded to bf16, through the cache."""
    ts, dense, ids = pc.exact_probe(T)
    p8 = ts.peer_fp8(None, cuda)
    c8 = HotRowCache(p8, capacity=4096, ring_cap=1 << 14, sample_every=1)
    dc, ic = dense.to(cuda), ids.to(cuda)
    ops.dot_interaction_gather_peer(dc, ic, p8, c8)
    assert c8.refresh() > 0
    c8.reset_counts()
    z = ops.dot_interaction_gather_peer(dc, ic, p8, c8)
    torch.cuda.synchronize()
    zr = ops.dot_interaction_gather_peer(dense, ids, ts.peer_fp8(), None)
    assert torch.equal(zr, pc.probe_reference(ts, dense, ids, torch.float32).to(torch.bfloat16))
    assert torch.equal(z.cpu(), zr)
    h, m = c8.counts()
    assert h > 0 and h + m == 37 * (T // 2)


def test_arena_form_matches_row_view(cuda):
    """K0 fused: the fp8 peer lookups read ids (and bag weights) from the raw
    request bytes of a device arena; padding rows read id 0."""
    from distributed_tf_serving_amd.client.synth import SyntheticRequests
    from distributed_tf_serving_amd.serving.arena import ArenaLayout
    from distributed_tf_serving_amd.serving.packing import PackedLayout

    A, L = ArenaLayout(43, 2048), PackedLayout(43)
    ar = A.alloc()
    s = SyntheticRequests(dist="zipf", id_space=1 << 50, seed=9)
    reqs = [s.message(n, raw=r).SerializeToString() for n, r in ((3, True), (250, True), (17, False), (200, True))]
    ab = A.build(ar, A.place(ar, reqs))
    dev = ar.to(cuda)
    A.decode_varints(dev)
    B = 512  # > total_rows
    packed = A.unpack_cpu(ar, L.alloc(B))
    ids, wts = L.ids(packed), L.wts(packed)
    assert ab.total_rows == 470 and (ids[470:] == 0).all()
    g = torch.Generator().manual_seed(4)
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16).to(cuda)
    rows = ops.ArenaRows(dev, B, 43)
    for T, hot in ((30, 1), (10, 3)):
        ts, _, _ = _stores(T, seed=20)
        p8 = ts.peer_fp8(9, cuda)
        c8 = HotRowCache(p8, capacity=2048, ring_cap=1 << 14, sample_every=1)
        for rnd in range(2):
            if hot == 1:
                want = ops.dot_interaction_gather_peer(dense, ids.to(cuda), p8, c8, id_col0=13)
                got = ops.dot_interaction_gather_peer(dense, rows, p8, c8, id_col0=13)
                # padding rows: id 0 of every table
                zero = ops.dot_interaction_gather_peer(dense[470:], torch.zeros(B - 470, 43, dtype=torch.int64,
                                                                                  device=cuda), p8, None, id_col0=13)
                assert torch.equal(_bits(got[470:]), _bits(zero))
            else:
                want = ops.peer_bag(ids.to(cuda), wts.to(cuda), B, 13, hot, p8, c8)
                got = ops.peer_bag(rows, None, B, 13, hot, p8, c8)
            torch.cuda.synchronize()
            assert got.dtype == torch.bfloat16 and torch.equal(_bits(got), _bits(want)), (T, hot, rnd)
            c8.refresh()
        assert c8.counts()[0] > 0


@pytest.mark.parametrize("hot", [1, 3])
def test_bags(cuda, hot):
    """peer_bag_fp8_kernel vs the bf16 peer_bag kernel on the dequantised
    stores: the same fp32 sums in the same order, apart from FMA contraction
    before the one bf16 rounding - within one bf16 ulp, |a - b| <= 2^-7 |b|."""
    T, B, col0 = 6, 517, 3
    ts, _, g = _stores(T, seed=30)
    ids = pc.skewed(B, col0 + T * hot, g, hot_ids=64)
    wts = torch.rand(B, col0 + T * hot, generator=g)
    p8, p16, pcpu = ts.peer_fp8(9, cuda), ts.peer_bf16(9, cuda), ts.peer_fp8(9)
    c8, c16, cc = (HotRowCache(p, capacity=2048, ring_cap=1 << 14, sample_every=2) for p in (p8, p16, pcpu))
    for rnd in range(2):
        for c in (c8, c16, cc):
            c.reset_counts()
        a = ops.peer_bag(ids.to(cuda), wts.to(cuda), B, col0, hot, p8, c8)
        b = ops.peer_bag(ids.to(cuda), wts.to(cuda), B, col0, hot, p16, c16)
        r = ops.peer_bag(ids, wts, B, col0, hot, pcpu, cc)
        torch.cuda.synchronize()
        assert a.dtype == torch.bfloat16 and a.shape == (B, T, 64)
        af, bf = a.float().cpu(), b.float().cpu()
        assert torch.isfinite(bf).all()
        err = ((af - bf).abs() - 2.0 ** -7 * bf.abs()).max().item()
        print(f"hot {hot} round {rnd}: max (|a - b| - 2^-7 |b|) = {err:.3g}, differing {int((af != bf).sum())}")
        assert err <= 0
        assert (af - r.float()).abs().max().item() <= 2.0 ** -6 * r.float().abs().max().item()
        assert c8.counts() == c16.counts() == cc.counts() and sum(cc.counts()) == (B // 2) * 3 * hot
        assert int(c8.ring_ctr.sum()) == int(cc.ring_ctr.sum())
        if rnd == 0:
            assert c8.refresh() > 0 and c16.refresh() > 0 and cc.refresh() > 0
            assert torch.equal(c8.keys.cpu(), cc.keys)
        else:
            assert c8.counts()[0] > 0


@pytest.mark.parametrize("ids64", [True, False])
def test_bags_exact_small_integers(cuda, ids64):
    """Codes in [-2, 2], weights in {0, 1, 2}, scales 1 and 2^-3: every sum is
    exact in fp32 in any order and a bf16 value - the kernel must match the CPU."""
    ts, _, _ = pc.exact_probe(5)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(-(1 << 40), 1 << 40, (37, 15), generator=g)
    ids = ids if ids64 else ids.to(torch.int32)
    wts = torch.randint(0, 3, (37, 15), generator=g).float()
    p8 = ts.peer_fp8(None, cuda)
    c8 = HotRowCache(p8, capacity=4096, ring_cap=1 << 14, sample_every=1)
    want = ops.peer_bag(ids, wts, 37, 0, 3, ts.peer_fp8(), None)
    assert want.float().abs().max() <= 256
    for rnd in range(2):
        got = ops.peer_bag(ids.to(cuda), wts.to(cuda), 37, 0, 3, p8, c8)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want), rnd
        c8.refresh()
    assert c8.counts()[0] > 0


def test_refresh_while_lookups_run(cuda):
    """tests/test_hot_cache.py::test_refresh_while_lookups_run (ordered) on fp8
    tables: refreshes on the lookups' stream while four cached lookups are in
    flight; every lookup equals the uncached one through hot-set turnover."""
    import threading
    import time

    ts, _, g = _stores(6, seed=40)
    p = ts.peer_fp8(9, cuda)
    c = HotRowCache(p, capacity=1024, ring_cap=1 << 14, sample_every=2)
    B, T = 2048, p.T
    batches = [(pc.skewed(B, T, g, hot_ids=48) + 100 * k).to(cuda) for k in range(3)]
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16).to(cuda)
    want = [ops.dot_interaction_gather_peer(dense, ids, p, None) for ids in batches]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(cuda)
    c.set_step_stream(s.cuda_stream)
    stop, errs, done = threading.Event(), [], [0]

    def worker():
        k = 0
        with torch.cuda.stream(s):
            while not stop.is_set():
                zs = [(k + j, ops.dot_interaction_gather_peer(dense, batches[(k + j) % 3], p, c)) for j in range(4)]
                s.synchronize()
                errs.extend(i for i, z in zs if not torch.equal(z, want[i % 3]))
                k += 4
        done[0] = k

    t = threading.Thread(target=worker)
    t.start()
    try:
        for _ in range(12):
            time.sleep(0.02)
            c.refresh()
    finally:
        stop.set()
        t.join(timeout=60)
    assert not errs, errs[:5]
    assert done[0] > 12 and c.refreshes == 12 and c.keys.numel() > 0 and c._ordered
    assert c.counts()[0] > 0


def test_bindings_reject_mismatched_stores(cuda):
    """Wrong store / scale / cache dtypes raise a Python error; nothing is launched."""
    from distributed_tf_serving_amd.ops import hip

    ts, _, g = _stores(6, seed=50)
    p8, p16 = ts.peer_fp8(None, cuda), ts.peer_bf16(None, cuda)
    B = 8
    dense = torch.randn(B, 64, generator=g).to(torch.bfloat16).to(cuda)
    ids = pc.skewed(B, 6, g).to(cuda)
    wts = torch.rand(B, 6, generator=g).to(cuda)
    out = torch.empty(B, 6, 64, dtype=torch.bfloat16, device=cuda)
    k8, k16 = p8.kernel_args(), p16.kernel_args()
    keys = torch.tensor([(1 << KEY_SHIFT) + 5], device=cuda)
    slots = torch.zeros(1, dtype=torch.int32, device=cuda)
    rows8 = torch.zeros(4, 64, dtype=F8, device=cuda)
    # bf16 stores passed to the fp8 ops
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        hip().dot_interaction_gather_peer_fp8(dense, ids, None, 0, tscale=p8.scale, store=p16.mine, **k16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        hip().peer_bag_fp8(ids, wts, None, B, 0, 1, tscale=p8.scale, store=p16.mine, out=out, **k16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        hip().peer_cache_fill_fp8(keys, slots, tscale=p8.scale, store=p16.mine, rows=rows8, **k16)
    # a short tscale, a tscale of another dtype
    for bad in (p8.scale[:5].contiguous(), p8.scale.double()):
        kb = dict(k8, tscale=bad)
        with pytest.raises(RuntimeError, match="tscale"):
            hip().dot_interaction_gather_peer_fp8(dense, ids, None, 0, store=p8.mine, **kb)
        with pytest.raises(RuntimeError, match="tscale"):
            hip().peer_bag_fp8(ids, wts, None, B, 0, 1, store=p8.mine, out=out, **kb)
        with pytest.raises(RuntimeError, match="tscale"):
            hip().peer_cache_fill_fp8(keys, slots, store=p8.mine, rows=rows8, **kb)
    # a bf16 cache with fp8 stores
    with pytest.raises(RuntimeError, match="cache rows"):
        hip().peer_cache_fill_fp8(keys, slots, store=p8.mine, rows=torch.zeros(4, 64, dtype=torch.bfloat16, device=cuda),
                                  **k8)
    # .. and fp8 rows with the bf16 fill
    with pytest.raises(RuntimeError, match="bf16"):
        hip().peer_cache_fill(keys, slots, rows=rows8, **k16)
    # a float8 bag output is refused too
    with pytest.raises(RuntimeError, match="bf16"):
        hip().peer_bag_fp8(ids, wts, None, B, 0, 1, store=p8.mine, out=out.to(F8), **k8)
    torch.cuda.synchronize()
    # the well-formed call still runs: the uint8 view of the stores is accepted
    hip().peer_cache_fill_fp8(keys, slots, store=p8.mine.view(torch.uint8), rows=rows8.view(torch.uint8), **k8)
    torch.cuda.synchronize()
    assert torch.equal(rows8.view(torch.uint8)[0].cpu(), ts.codes[1].view(torch.uint8)[ROWS + 5])


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("hot", [1, 3])
def test_fp8_peer_exchange_ranks_sharing_one_gpu(hot):
    """tests/test_multirank_gpu.py::test_peer_exchange_ranks_sharing_one_gpu on
    fp8 tables: two ranks map each other's code stores by IPC; scores match the
    unsharded fp8 DLRM of the same seed through the eager forward and the
    arena step program, before and after the replica cache fills."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "-m", "tools.studies.peer_lookup_check",
           "--table-dtype", "fp8", "--rows", "5003", "--batch", "512", "--hot", str(hot)]
    env = dict(os.environ, DTFS_SHARE_GPU="1")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    ranks = json.loads(line[0])["ranks"]
    assert len(ranks) == 2
    tol = 1e-6 if hot == 1 else 2e-3  # one-hot: the same fused kernel math as the local fp8 model
    for r in ranks:
        assert r["remote_tables"] > 0 and r["table_dtype"] == "fp8"
        for rnd in r["rounds"]:
            assert rnd["max_abs_diff"] <= tol and rnd["max_abs_diff_arena_program"] <= tol, r["rounds"]
        assert r["rounds"][0]["hits"] == 0 and r["rounds"][-1]["hits"] > 0, r["rounds"]
