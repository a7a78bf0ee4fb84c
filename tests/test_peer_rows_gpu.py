"""The peer lookup on row-wise sharded tables on the GPU
(csrc/kernels/peer_lookup_rows.hip): three stores on one GPU stand in for
three ranks (tests/peer_rows_cases.py), seen from rank 0 and from rank 1 (whose
own range is the middle one). The fused kernel, the bags and the cache fill on
the row ranges against the merged table-wise peer kernels on stores holding
the same rows whole and against the local kernel on the concatenated store -
bit for bit: the same rows enter the same arithmetic - and against the CPU
twin's counters, ring, hot keys and cached bytes; the arena form, the
bindings' rejections and two ranks sharing the GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_rows_cases as rc  # noqa: E402

from distributed_tf_serving_amd import ops  # noqa: E402
from distributed_tf_serving_amd.parallel.hot_cache import KEY_SHIFT, HotRowCache, PeerTables  # noqa: E402

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return x.cpu().view(torch.int16)


def _bytes(x):
    return x.cpu().view(torch.uint8)


def _caches(*peers, sample_every=2):
    """A GPU cache and its CPU twin. 0.75 x the capacity holds every sampled
    key (<= 259 candidates x 31 tables), so the hot set has no ties to break.
    The index hashes bits 24.. of key x 0x9E37..15 (peer_lookup.h cache_hash),
    so the table number (key bits 40..) reaches only hash bits 16..: an index
    under 2^21 entries puts row v of EVERY table on one slot. The streams here
    share their hot rows between the tables and, cut by rows, all 31 tables
    have remote rows: chains of 31 equal hashes run past the kernels' 32
    probes, a cached row is then read from its owner and counted as a miss,
    and the CPU twin (an exact search) counts a hit. From 7 tables on the
    capacity is therefore 2^20 (2^21 entries: the 31 tables hash apart)."""
    cap = 16384 if peers[0].T <= 6 else 1 << 20
    return [HotRowCache(p, capacity=cap, ring_cap=1 << 14, sample_every=sample_every) for p in peers]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("chunk_shift", [None, 9])
@pytest.mark.parametrize("T,B,ids64", [(1, 1, True), (1, 517, False), (6, 1, False), (6, 517, True), (31, 1, True),
                                       (31, 517, False)])
def test_fused_kernel(cuda, fp8, chunk_shift, T, B, ids64):
    """Row ranges (pure and, for T > 1, mixed with whole tables) from rank 0
    and rank 1 == the table-wise peer kernel == the local kernel, bit for bit,
    before a refresh (all misses) and after (hits); counters, ring totals, hot
    keys and cached bytes are the CPU twin's."""
    col0 = 3
    for mixed in ((False, True) if T > 1 else (False,)):
        g = torch.Generator().manual_seed(100 * T + B + mixed)
        rs = rc.RowStores(T, g, mixed=mixed)
        full = rs.ids(B, col0, 1, g)
        fi = full if ids64 else full.to(torch.int32)
        assert (fi < 0).any()
        dense = torch.randn(B, 64, generator=g).to(torch.bfloat16)
        dc, ic = dense.to(cuda), fi.to(cuda)
        store, mod, off = rs.local(fp8)
        if fp8:
            zl = ops.dot_interaction_gather_fp8(dc, store.to(cuda), rs.scale.to(cuda), ic[:, col0:], mod.to(cuda),
                                                off.to(cuda))
        else:
            zl = ops.dot_interaction_gather(dc, store.to(cuda), ic[:, col0:], mod.to(cuda), off.to(cuda))
        pt = rs.peer_tables(0, fp8, chunk_shift, cuda)
        zt = ops.dot_interaction_gather_peer(dc, ic, pt, None, id_col0=col0)
        used = 64 + (T + 1) * T // 2
        for rank in (0, 1):
            pr, pcpu = rs.peer_rows(rank, fp8, chunk_shift, cuda), rs.peer_rows(rank, fp8, chunk_shift)
            assert pr.row_wise and pr.ranges_desc is not None and pr.rlo.is_cuda
            if chunk_shift:
                assert len(pr.stores[0]) == -(-rs.row_codes[0].shape[0] >> 9)
            cr, cc = _caches(pr, pcpu)
            for rnd in range(2):
                cr.reset_counts(), cc.reset_counts()
                z = ops.dot_interaction_gather_peer(dc, ic, pr, cr, id_col0=col0)
                zr = ops.dot_interaction_gather_peer(dense, fi, pcpu, cc, id_col0=col0)
                torch.cuda.synchronize()
                what = f"mixed {mixed} rank {rank} round {rnd}"
                assert z.dtype == torch.bfloat16 and z.shape == zl.shape == (B, ops.interaction_cols(T, 64))
                assert torch.equal(_bits(z), _bits(zt)), what + ": vs the table-wise peer kernel"
                assert torch.equal(_bits(z), _bits(zl)), what + ": vs the local kernel"
                assert (z[:, used:] == 0).all() and torch.equal(z[:, :64].cpu(), dense)
                assert (z.float().cpu() - zr.float()).abs().max().item() < 2e-2 * max(1.0, zr.float().abs().max().item())
                assert cr.counts() == cc.counts(), what
                assert int(cr.ring_ctr.sum()) == int(cc.ring_ctr.sum()), what
                if rnd == 0:
                    assert cr.counts()[0] == 0
                    n = cc.refresh()
                    assert cr.refresh() == n and (n > 0 or B == 1)
                    assert torch.equal(cr.keys.cpu(), cc.keys) and cr.slots.unique().numel() == cc.keys.numel()
                    kt, kv = cc.keys >> KEY_SHIFT, cc.keys & ((1 << KEY_SHIFT) - 1)
                    assert pcpu.remote_cpu(kt, kv).all()
                    # the fill: every cached row is its owner's row bytes
                    assert torch.equal(_bytes(cr.rows[cr.slots.long()]), pcpu.row_cpu(kt, kv).view(torch.uint8))
                elif B > 1:
                    assert cr.counts()[0] > 0, what


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("hot", [1, 3])
def test_bags(cuda, hot, fp8):
    """peer_bag_rows(_fp8)_kernel == the table-wise peer_bag(_fp8)_kernel on
    the whole-table stores == the same kernel on the one concatenated store,
    == the local bag kernel (ops.embedding_bag / embedding_bag_fp8) on that
    store, bit for bit: the same rows enter the same fp32 sums in the same
    order. One bag has its three ids on three different ranks."""
    T, B, col0 = 6, 517, 3
    for mixed in (False, True):
        g = torch.Generator().manual_seed(30 + hot + mixed)
        rs = rc.RowStores(T, g, mixed=mixed)
        ids = rs.ids(B, col0, hot, g)
        if hot == 3:
            ids[B - 1, col0 + 3:col0 + 6] = torch.tensor(rs.spread_bag(1))  # table 1's bag: three ranks
            assert {rs.owner_of(1, v) for v in rs.spread_bag(1)} == {0, 1, 2}
        wts = torch.rand(B, col0 + T * hot, generator=g)
        ic, wc = ids.to(cuda), wts.to(cuda)
        pt = rs.peer_tables(0, fp8, 9, cuda)
        bt = ops.peer_bag(ic, wc, B, col0, hot, pt, None)
        store, mod, off = rs.local(fp8)
        one = PeerTables([store.to(cuda)], [0] * T, off.tolist(), rs.rows, rank=0, scale=rs.scale if fp8 else None)
        bl = ops.peer_bag(ic, wc, B, col0, hot, one, None)
        # the local bag kernel over (c): rows resolved on the host
        t = torch.arange(T).repeat_interleave(hot)
        rows = (off[t] + torch.remainder(ids[:, col0:], mod[t])).reshape(-1).to(cuda)
        offs = torch.arange(0, B * T * hot + 1, hot, dtype=torch.int64, device=cuda)
        w = wc[:, col0:].contiguous().view(-1)
        if fp8:
            be = ops.embedding_bag_fp8(store.to(cuda), rs.scale.to(cuda), rows, offs, per_sample_weights=w,
                                       modulo=store.shape[0], out_bf16=True)
        else:
            be = ops.embedding_bag(store.to(cuda), rows, offs, per_sample_weights=w, modulo=store.shape[0], out_bf16=True)
        bef = be.float().cpu().view(B, T, 64)
        for rank in (0, 1):
            pr, pcpu = rs.peer_rows(rank, fp8, 9, cuda), rs.peer_rows(rank, fp8, 9)
            cr, cc = _caches(pr, pcpu)
            for rnd in range(2):
                cr.reset_counts(), cc.reset_counts()
                a = ops.peer_bag(ic, wc, B, col0, hot, pr, cr)
                r = ops.peer_bag(ids, wts, B, col0, hot, pcpu, cc)
                torch.cuda.synchronize()
                what = f"mixed {mixed} rank {rank} round {rnd}"
                assert a.dtype == torch.bfloat16 and a.shape == (B, T, 64)
                assert torch.equal(_bits(a), _bits(bt)), what + ": vs the table-wise peer bag kernel"
                assert torch.equal(_bits(a), _bits(bl)), what + ": vs the peer bag kernel on the local store"
                af = a.float().cpu()
                print(f"{what}: vs the local bag kernel {int((af != bef).sum())} values differ")
                assert torch.equal(_bits(a), _bits(be.view(B, T, 64))), what + ": vs the local bag kernel"
                assert (af - r.float()).abs().max().item() <= 2.0 ** -6 * r.float().abs().max().item()
                assert cr.counts() == cc.counts() and int(cr.ring_ctr.sum()) == int(cc.ring_ctr.sum()), what
                if rnd == 0:
                    assert cr.counts()[0] == 0 and cr.refresh() > 0 and cc.refresh() > 0
                    assert torch.equal(cr.keys.cpu(), cc.keys)
                else:
                    assert cr.counts()[0] > 0


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("chunk_shift", [None, 9])
def test_cache_fill(cuda, fp8, chunk_shift):
    """Every filled slot holds its owner's row bytes: every boundary row of
    every table and both rows of the 2-row table, local and remote alike."""
    g = torch.Generator().manual_seed(60)
    for mixed in (False, True):
        rs = rc.RowStores(7, g, mixed=mixed)
        logical = rs.codes if fp8 else rs.deq
        cases = [(t, v) for t in range(rs.T) for v in rs.boundaries(t)]
        assert {(rs.T - 1, 0), (rs.T - 1, 1)} <= set(cases)
        keys = torch.tensor([(t << KEY_SHIFT) | v for t, v in cases])
        slots = torch.randperm(64, generator=g)[:len(cases)].to(torch.int32)
        want = torch.stack([logical[t][v] for t, v in cases])
        for rank in (0, 1):
            pr = rs.peer_rows(rank, fp8, chunk_shift, cuda)
            c = HotRowCache(pr, capacity=64, ring_cap=64)
            c.rows.view(torch.uint8).fill_(0x5A)
            c._fill(keys.to(cuda), slots.to(cuda))
            torch.cuda.synchronize()
            assert torch.equal(_bytes(c.rows[slots.long().to(cuda)]), want.view(torch.uint8)), (mixed, rank)
            rest = torch.ones(64, dtype=torch.bool)
            rest[slots.long()] = False
            assert (_bytes(c.rows)[rest] == 0x5A).all()  # no other slot is written


def test_arena_form_matches_row_view(cuda):
    """K0 fused: the row-wise peer lookups read ids (and bag weights) from the
    raw request bytes of a device arena; padding rows read id 0."""
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
    for fp8 in (False, True):
        for T, hot in ((30, 1), (10, 3)):
            rs = rc.RowStores(T, g, mixed=True)
            pr = rs.peer_rows(1, fp8, 9, cuda)
            cr = HotRowCache(pr, capacity=4096, ring_cap=1 << 14, sample_every=1)
            for rnd in range(2):
                if hot == 1:
                    want = ops.dot_interaction_gather_peer(dense, ids.to(cuda), pr, cr, id_col0=13)
                    got = ops.dot_interaction_gather_peer(dense, rows, pr, cr, id_col0=13)
                    # padding rows: id 0 of every table
                    zero = ops.dot_interaction_gather_peer(dense[470:], torch.zeros(B - 470, 43, dtype=torch.int64,
                                                                                      device=cuda), pr, None, id_col0=13)
                    assert torch.equal(_bits(got[470:]), _bits(zero))
                else:
                    want = ops.peer_bag(ids.to(cuda), wts.to(cuda), B, 13, hot, pr, cr)
                    got = ops.peer_bag(rows, None, B, 13, hot, pr, cr)
                torch.cuda.synchronize()
                assert got.dtype == torch.bfloat16 and torch.equal(_bits(got), _bits(want)), (fp8, T, hot, rnd)
                cr.refresh()
            assert cr.counts()[0] > 0


def test_bindings_reject_malformed_descriptors(cuda):
    """Every malformed range descriptor raises a Python error before anything
    is launched; a well-formed call afterwards still gives the right rows."""
    from distributed_tf_serving_amd.ops import hip

    g = torch.Generator().manual_seed(50)
    rs = rc.RowStores(4, g)
    pr = rs.peer_rows(0, False, None, cuda)
    W, T = rc.S, rs.T
    rlo, roff, trows = pr.rlo_cpu, pr.roff_cpu, pr.trows_cpu
    store_rows = torch.tensor(pr.store_rows, dtype=torch.int64)

    def make(rlo=rlo, roff=roff, trows=trows, store_rows=store_rows, cbase=pr.cbase, rank=0, shift=pr.chunk_shift):
        return hip().peer_row_ranges(cbase, rlo, roff, trows, store_rows, rank, shift)

    def edited(x, t, r, val):
        y = x.clone()
        y[t, r] = val
        return y

    n2 = int(rlo[0, 3] - rlo[0, 2])
    bad = {
        "a gap in front (the first start is not 0)": dict(rlo=edited(rlo, 0, 0, 1)),
        "a decreasing start": dict(rlo=edited(rlo, 0, 2, int(rlo[0, 1]) - 1)),
        "a total that is not the table's rows": dict(rlo=edited(rlo, 0, 3, rc.ROWS - 1)),
        "a range past its store": dict(roff=edited(roff, 0, 2, pr.store_rows[2] - n2 + 1)),
        "a negative store offset": dict(roff=edited(roff, 1, 0, -1)),
        "a store row count too small": dict(store_rows=store_rows - 1),
        "rlo without its last column": dict(rlo=rlo[:, :W].contiguous()),
        "roff of another world": dict(roff=roff[:, :W - 1].contiguous()),
        "int32 boundaries": dict(rlo=rlo.to(torch.int32)),
        "boundaries on the device": dict(rlo=rlo.to(cuda)),
        "a table short": dict(trows=trows[:T - 1].contiguous()),
        "an empty table": dict(rlo=torch.cat([rlo[:3], torch.zeros(1, W + 1, dtype=torch.int64)]),
                               trows=torch.cat([trows[:3], torch.zeros(1, dtype=torch.int64)])),
        "cbase of two ranks": dict(cbase=pr.cbase[:2].contiguous()),
        "a rank outside the world": dict(rank=W),
        "an unmapped chunk": dict(cbase=torch.zeros_like(pr.cbase)),
        "a chunk size the stores do not have": dict(shift=4),
    }
    for what, kw in bad.items():
        with pytest.raises((RuntimeError, TypeError)):
            make(**kw)
            pytest.fail(what + " was accepted")
    # the kernels take only the checked object, and fp8 arguments go together
    dense = torch.randn(8, 64, generator=g).to(torch.bfloat16).to(cuda)
    ids = rs.ids(8, 0, 1, g).to(cuda)
    with pytest.raises(TypeError):
        hip().dot_interaction_gather_peer_rows(dense, ids, None, 0, pr.cbase)
    with pytest.raises(RuntimeError, match="together"):
        hip().dot_interaction_gather_peer_rows(dense, ids, None, 0, pr.ranges_desc, tscale=rs.scale.to(cuda))
    rows16 = torch.zeros(4, 64, dtype=torch.bfloat16, device=cuda)
    keys = torch.tensor([(0 << KEY_SHIFT) | int(rlo[0, 2]), (3 << KEY_SHIFT) | 1], device=cuda)
    slots = torch.tensor([2, 0], dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="bf16"):
        hip().peer_cache_fill_rows(keys, slots, pr.ranges_desc, rows=rows16.view(torch.uint8).view(F8)[:, :64].contiguous())
    torch.cuda.synchronize()
    # the well-formed call still runs
    d = make()
    assert d.world == W and d.rank == 0 and torch.equal(d.rlo.cpu(), rlo) and torch.equal(d.roff.cpu(), roff)
    hip().peer_cache_fill_rows(keys, slots, d, rows=rows16)
    torch.cuda.synchronize()
    assert torch.equal(_bits(rows16[2]), _bits(rs.deq[0][int(rlo[0, 2])])) and torch.equal(_bits(rows16[0]), _bits(rs.deq[3][1]))
    assert (rows16[1] == 0).all() and (rows16[3] == 0).all()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("table_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("hot", [1, 3])
def test_row_wise_peer_exchange_ranks_sharing_one_gpu(hot, table_dtype):
    """tests/test_multirank_gpu.py::test_peer_exchange_ranks_sharing_one_gpu and
    tests/test_peer_fp8_gpu.py's fp8 form with every table cut by rows: two
    ranks map each other's stores by IPC; scores match the unsharded DLRM of
    the same seed through the eager forward and the arena step program, before
    and after the replica cache fills."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), "-m", "tools.studies.peer_lookup_check",
           "--policy", "row", "--table-dtype", table_dtype, "--rows", "5003", "--batch", "512", "--hot", str(hot)]
    env = dict(os.environ, DTFS_SHARE_GPU="1")
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, p.stdout
    ranks = json.loads(line[0])["ranks"]
    assert len(ranks) == 2
    tol = 1e-6 if hot == 1 else 2e-3  # one-hot: the same fused kernel math as the local model
    for r in ranks:
        assert r["policy"] == "row" and r["remote_tables"] == 8 and r["table_dtype"] == table_dtype
        for rnd in r["rounds"]:
            assert rnd["max_abs_diff"] <= tol and rnd["max_abs_diff_arena_program"] <= tol, r["rounds"]
        assert r["rounds"][0]["hits"] == 0 and r["rounds"][-1]["hits"] > 0, r["rounds"]
