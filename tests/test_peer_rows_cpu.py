"""The peer lookup on row-wise sharded tables, CPU side: the range descriptor
of parallel/hot_cache.py PeerTables (round trip from the planner, the row
locator, per-lookup remoteness, malformed ranges), peer_gather_cpu on it
against the table-wise descriptor over the same rows, ShardedEmbedding /
ShardedDLRM with policy "row" behind the peer exchange, the preset, gloo ranks
against the unsharded model and a table-wise checkpoint loaded row-wise."""
import multiprocessing as mp
import os
import socket
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_fp8_cases as pc  # noqa: E402
import peer_rows_cases as rc  # noqa: E402

from distributed_tf_serving_amd.config import ModelConfig, load_preset  # noqa: E402
from distributed_tf_serving_amd.parallel.hot_cache import (KEY_SHIFT, HotRowCache, PeerTables, auto_capacity,  # noqa: E402
                                                           peer_gather_cpu)

F8 = torch.float8_e4m3fn


def _u8(x):
    return x.view(torch.uint8) if x.dtype == F8 else x.view(torch.int16)


# ------------------------------------------------------------------ descriptor
@pytest.mark.parametrize("policy", ["row", "mixed"])
def test_planner_ranges_round_trip(policy):
    """Placement.ranges of a row-wise (and a mixed) plan -> ShardedEmbedding's
    ranges -> PeerTables: rlo / roff hold exactly the plan's pieces at the
    layout's offsets, and every row is found where the layout put it."""
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import (Placement, ShardedEmbedding, ShardingPlan,
                                                                        TableSpec, plan_sharding)

    tables = [TableSpec(f"t{i}", n, 64) for i, n in enumerate((4099, 2, 4099, 301))]
    W = 3
    plan = plan_sharding(tables, W, policy="row")
    assert plan.row_wise() == [0, 1, 2, 3]
    assert [n for _, n in plan.placement(0).ranges] == [1367, 1366, 1366]
    assert [n for _, n in plan.placement(1).ranges] == [1, 1, 0]  # fewer rows than ranks: an empty range
    if policy == "mixed":  # tables 1 and 3 whole (on ranks 2 and 0), 0 and 2 by rows - with uneven pieces
        pl = [Placement(0, "row", ranges=[(0, 4000), (4000, 0), (4000, 99)]), Placement(1, "table", rank=2),
              plan.placement(2), Placement(3, "table", rank=0)]
        plan = ShardingPlan(tables, W, pl, plan.budget_bytes)
    # one process cannot hold three ranks' ShardedEmbedding; build the stores from each rank's layout instead
    embs = []
    for r in range(W):
        ctx = DistContext(device=torch.device("cpu"))
        ctx.rank, ctx.world = r, W
        e = ShardedEmbedding(plan, ctx, 7, 0.125, exchange="alltoall")  # the layout and the init are the exchange's own
        embs.append(e)
    ranges = []
    for t in range(len(tables)):
        p = plan.placement(t)
        if p.kind == "row":
            ranges.append([(*p.ranges[r], next(o for tt, _, _, o in embs[r].segments if tt == t)) for r in range(W)])
        else:
            off = next(o for tt, _, _, o in embs[p.rank].segments if tt == t)
            ranges.append([(0, tables[t].rows, off) if r == p.rank else (0 if r < p.rank else tables[t].rows, 0, 0)
                           for r in range(W)])
    stores = [e.store.data for e in embs]
    from distributed_tf_serving_amd.models.layers import hashed_uniform_rows_

    for rank in range(W):
        pt = PeerTables(stores, None, None, [t.rows for t in tables], rank=rank, ranges=ranges)
        assert pt.row_wise and pt.rlo.shape == (4, W + 1) and pt.roff.shape == (4, W)
        assert pt.rlo[:, 0].eq(0).all() and pt.rlo[:, -1].tolist() == [t.rows for t in tables]
        for t in range(4):
            p = plan.placement(t)
            want = [n for _, n in p.ranges] if p.kind == "row" else [tables[t].rows * (r == p.rank) for r in range(W)]
            assert (pt.rlo[t, 1:] - pt.rlo[t, :-1]).tolist() == want
            full = torch.empty(tables[t].rows, 64, dtype=torch.bfloat16)
            hashed_uniform_rows_(full, t, 0, 7, 0.125)  # the unsharded table
            v = torch.arange(tables[t].rows)
            tt = torch.full_like(v, t)
            assert torch.equal(pt.row_cpu(tt, v), full)
            own = torch.repeat_interleave(torch.arange(W), torch.tensor(want))
            assert torch.equal(pt.locate_cpu(tt, v)[0], own)
            assert torch.equal(pt.remote_cpu(tt, v), own != rank)
        assert pt.remote_rows == sum(t.rows for t in tables) - int((pt.rlo[:, rank + 1] - pt.rlo[:, rank]).sum())
        assert pt.remote_tables == sum(int(pt.rlo[t, rank + 1] - pt.rlo[t, rank]) < tables[t].rows for t in range(4))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
def test_row_cpu_and_remote_cpu(mixed, fp8):
    g = torch.Generator().manual_seed(1)
    rs = rc.RowStores(7, g, mixed=mixed)
    logical = rs.codes if fp8 else rs.deq
    for rank in (0, 1, 2):
        p = rs.peer_rows(rank, fp8, chunk_shift=9 if rank == 1 else None)
        assert p.row_wise and p.fp8 == fp8 and p.owner is None
        small = rs.T - 1
        cases = [(small, v) for v in range(rc.SMALL)] + [(t, v) for t in range(rs.T) for v in rs.boundaries(t)]
        t = torch.tensor([c[0] for c in cases])
        v = torch.tensor([c[1] for c in cases])
        got = p.row_cpu(t, v)
        want = torch.stack([logical[a][b] for a, b in cases])
        assert torch.equal(_u8(got), _u8(want))
        own = torch.tensor([rs.owner_of(a, b) for a, b in cases])
        assert torch.equal(p.locate_cpu(t, v)[0], own)
        assert torch.equal(p.remote_cpu(t, v), own != rank)  # true exactly outside the rank's range
        # the table-wise descriptor over the same rows agrees row for row
        assert torch.equal(_u8(rs.peer_tables(rank, fp8).row_cpu(t, v)), _u8(want))
    # rank 2 holds nothing of the 2-row table: all of it is remote there
    p2 = rs.peer_rows(2, fp8)
    assert rs.ranges[rs.T - 1][2][1] == 0 or mixed
    n_here = sum(rr[2][1] for rr in rs.ranges)
    assert p2.remote_rows == sum(rs.rows) - n_here
    assert abs(p2.remote_row_fraction - sum(1 - rr[2][1] / n for rr, n in zip(rs.ranges, rs.rows)) / rs.T) < 1e-12
    assert auto_capacity(p2, free_bytes=1 << 40) == p2.remote_rows


def test_table_wise_descriptor_keeps_its_attributes():
    g = torch.Generator().manual_seed(2)
    rs = rc.RowStores(5, g)
    p = rs.peer_tables(0, False)
    assert not p.row_wise and p.ranges_desc is None
    assert p.rows == rs.rows and p.owner == rs.tw_owner and p.off == rs.tw_off
    assert p.towner.tolist() == rs.tw_owner and p.toff.tolist() == rs.tw_off
    assert p.tremote_cpu.tolist() == [o != 0 for o in rs.tw_owner] and p.remote_tables == 3
    assert set(p.kernel_args()) == {"cbase", "towner", "toff", "trows", "tremote", "chunk_shift"}
    assert p.remote_rows == sum(n for n, o in zip(rs.rows, rs.tw_owner) if o != 0)
    assert p.remote_row_fraction == 3 / 5
    t, v = torch.tensor([0, 1, 4]), torch.tensor([5, 6, 1])
    assert p.remote_cpu(t, v).tolist() == [False, True, True]


def test_malformed_ranges_raise():
    g = torch.Generator().manual_seed(3)
    rs = rc.RowStores(4, g)
    bad = rc.bad_ranges(rs)
    assert [w for w, _ in bad] == ["gap", "decreasing", "total", "store"]
    for (what, ranges), match in zip(bad, ("gap", "decrease", "cover", "outside its store")):
        with pytest.raises(ValueError, match=match):
            PeerTables(rs.row_deq, None, None, rs.rows, rank=0, ranges=ranges)
    with pytest.raises(ValueError, match="per rank"):
        PeerTables(rs.row_deq, None, None, rs.rows, rank=0, ranges=[rr[:2] for rr in rs.ranges])
    with pytest.raises(ValueError, match="tables"):
        PeerTables(rs.row_deq, None, None, rs.rows, rank=0, ranges=rs.ranges[:-1])
    PeerTables(rs.row_deq, None, None, rs.rows, rank=0, ranges=rs.ranges)  # the well-formed one


# ------------------------------------------------------------ peer_gather_cpu
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("hot", [1, 3])
def test_gather_cpu_matches_the_table_wise_descriptor(hot, fp8, mixed):
    g = torch.Generator().manual_seed(10 + hot)
    T, B = 7, 61
    rs = rc.RowStores(T, g, mixed=mixed)
    ids = rs.ids(B, 0, hot, g)
    if hot == 3:
        ids[B - 1, 3:6] = torch.tensor(rs.spread_bag(1))  # table 1's bag: three ids on three ranks
    wts = torch.rand(B, T * hot, generator=g) if hot > 1 else None
    for rank in (0, 1):
        pr, pt = rs.peer_rows(rank, fp8), rs.peer_tables(rank, fp8)
        cr = HotRowCache(pr, capacity=4096, ring_cap=1 << 14, sample_every=2)
        want = peer_gather_cpu(pt, None, ids, wts, hot)
        t = torch.arange(T).repeat_interleave(hot).repeat(B)
        v = torch.remainder(ids.reshape(-1), torch.tensor(rs.rows)[t])
        b = torch.arange(B).repeat_interleave(T * hot)
        remote = torch.tensor([rs.owner_of(int(a), int(c)) != rank for a, c in zip(t, v)])
        for rnd in range(2):
            cr.reset_counts()
            ctr0 = int(cr.ring_ctr[0])
            got = peer_gather_cpu(pr, cr, ids, wts, hot)
            assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), rnd
            h, m = cr.counts()
            assert h + m == int((remote & (b % 2 == 1)).sum())  # the counted lookups with a remote owner
            keys = ((t << KEY_SHIFT) | v)[remote & (b % 2 == 0)]  # exactly the sampled remote keys
            assert int(cr.ring_ctr[0]) - ctr0 == keys.numel()
            assert torch.equal(cr.ring[ctr0:ctr0 + keys.numel()], keys)
            if rnd == 0:
                assert h == 0 and cr.refresh() > 0
                kt, kv = cr.keys >> KEY_SHIFT, cr.keys & ((1 << KEY_SHIFT) - 1)
                assert pr.remote_cpu(kt, kv).all()  # only remote rows are cached
                assert torch.equal(_u8(cr.rows[cr.slots.long()]), _u8(pr.row_cpu(kt, kv)))
            else:
                assert h > 0


# ------------------------------------------------- ShardedEmbedding / ShardedDLRM
def _cfg(hot=1, rows=997, **kw):
    kw.setdefault("embedding_exchange", "peer")
    return ModelConfig(family="dlrm", num_fields=5 + 5 * hot, num_dense=5, table_rows=rows, embed_dim=64,
                       bottom_mlp=(32, 64), mlp_dims=(64, 32), multi_hot=hot, hot_cache_rows=1024, **kw)


def test_row_policy_behind_the_peer_exchange_on_one_rank():
    from distributed_tf_serving_amd.models import build_model
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import (ShardedDLRM, ShardedEmbedding, TableSpec,
                                                                        build_parallel_model, plan_sharding)

    one = DistContext(device=torch.device("cpu"))
    tables = [TableSpec(f"t{i}", 40, 64) for i in range(3)]
    for hot in (1, 3):
        e = ShardedEmbedding(plan_sharding(tables, 1, policy="row"), one, 1, 0.125, exchange="peer", hot=hot)
        assert e.peer is not None and e.exchange_bytes(24) == 0
    cfg = _cfg(embedding_sharding="row")
    m = ShardedDLRM(cfg, one, policy="row")
    g = torch.Generator().manual_seed(4)
    ids, wts = pc.skewed(16, cfg.num_fields, g), torch.rand(16, cfg.num_fields, generator=g)
    assert (m(ids, wts) - build_model(cfg)(ids, wts)).abs().max().item() < 1e-5
    assert build_parallel_model(cfg, "cpu", shard_tables="on").emb.exchange == "peer"
    assert ModelConfig().embedding_sharding == "auto"  # a config written before the key existed loads with it


def test_row_wise_ranges_of_a_sharded_embedding(monkeypatch):
    """Rank 1 of 3, row-wise, fp8 and multi-hot behind the peer exchange: the
    constructor accepts the plan and hands PeerTables the plan's ranges at the
    layout's offsets (the peers' stores are stood in for by empty ones of their sizes)."""
    from distributed_tf_serving_amd.parallel import embedding_sharding as es, hot_cache
    from distributed_tf_serving_amd.parallel.dist import DistContext

    tables = [es.TableSpec(f"t{i}", n, 64, 1) for i, n in enumerate((4099, 2, 301))]
    plan = es.plan_sharding(tables, 3, policy="row")
    ctx = DistContext(device=torch.device("cpu"))
    ctx.rank, ctx.world = 1, 3
    monkeypatch.setattr(es.dist, "all_gather_object", lambda out, obj, group=None: out.__setitem__(slice(None), [obj] * 3))
    held = [sum(plan.placement(t).ranges[r][1] for t in range(3)) for r in range(3)]
    monkeypatch.setattr(hot_cache, "open_peer_stores", lambda mine, group, tag: [
        list(mine) if r == 1 else [torch.zeros(held[r], 64).to(mine[0].dtype)] for r in range(3)])
    e = es.ShardedEmbedding(plan, ctx, 7, 0.125, exchange="peer", hot=3, table_dtype="fp8", cache_rows=64)
    p = e.peer
    assert p.row_wise and p.fp8 and p.rank == 1 and e.cache is not None
    assert [[(lo, n) for lo, n, _ in rr] for rr in p.ranges] == [plan.placement(t).ranges for t in range(3)]
    assert [rr[1][2] for rr in p.ranges] == [o for _, _, _, o in e.segments]
    assert p.remote_tables == 3 and 0 < e.exchange_bytes(24) < 24 * 3 * 3 * 64
    # the fp8 hashed init starts at each segment's global lo: the shard holds the unsharded fp8 model's rows
    from distributed_tf_serving_amd import ops
    from distributed_tf_serving_amd.models.layers import hashed_uniform_rows_

    for t, lo, n, off in e.segments:
        full = torch.empty(tables[t].rows, 64, dtype=torch.bfloat16)
        hashed_uniform_rows_(full, t, 0, 7, 0.125)
        q = ops.quant_table_fp8(full, float(e.emb_scale[t]))
        assert torch.equal(e.store.data.view(torch.uint8)[off:off + n], q.view(torch.uint8)[lo:lo + n]), t


def test_alltoall_keeps_its_rejections():
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import ShardedEmbedding, TableSpec, plan_sharding

    ctx = DistContext(device=torch.device("cpu"))
    ctx.rank, ctx.world = 0, 2
    tables = [TableSpec(f"t{i}", 40, 64) for i in range(3)]
    with pytest.raises(NotImplementedError, match="multi-hot"):
        ShardedEmbedding(plan_sharding(tables, 2, policy="row"), ctx, 1, 0.125, hot=3)
    for policy in ("row", "table"):
        with pytest.raises(ValueError, match="peer"):
            ShardedEmbedding(plan_sharding(tables, 2, policy=policy), ctx, 1, 0.125, table_dtype="fp8")


def test_preset_loads_and_only_places_row_wise():
    from distributed_tf_serving_amd.parallel.embedding_sharding import dlrm_tables, plan_sharding

    cfg = load_preset("dlrm_rowwise_sharded8")
    m = cfg.model
    assert m.embedding_exchange == "peer" and m.embedding_sharding == "row" and m.table_dtype == "bf16"
    assert m.num_sparse == 4 and m.table_rows == 2_000_000_000 < 2 ** 31 and cfg.client.backends == 8
    ref = load_preset("dlrm_sharded8").model
    assert (m.mlp_dims, m.bottom_mlp, m.num_dense, m.embed_dim) == (ref.mlp_dims, ref.bottom_mlp, ref.num_dense,
                                                                   ref.embed_dim)
    assert ref.embedding_sharding == "auto"  # a preset without the key
    tables = dlrm_tables(m)
    assert tables[0].bytes == 256 * 10 ** 9
    with pytest.raises(MemoryError):
        plan_sharding(tables, 8, policy="table")
    plan = plan_sharding(tables, 8, policy="row")
    assert plan.rank_bytes() == [128 * 10 ** 9] * 8


# ------------------------------------------------------------------ gloo ranks
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _store_bytes(emb):
    return torch.cat([_u8(c.data) for c in [emb.store, *emb.store_chunks]])


def _worker(rank, world, port, hot, table_dtype, path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from distributed_tf_serving_amd.models import build_model
    from distributed_tf_serving_amd.parallel.dist import init_from_env, shutdown
    from distributed_tf_serving_amd.parallel.embedding_sharding import ShardedDLRM, build_parallel_model
    from distributed_tf_serving_amd.utils.checkpoint import load_sharded, save_sharded

    try:
        ctx = init_from_env(device="cpu")
        cfg = _cfg(hot, table_dtype=table_dtype, embedding_sharding="row")
        m = build_parallel_model(cfg, "cpu", ctx)
        e = m.emb
        assert e.peer.row_wise and e.rw == list(range(5)) and not m.has_collectives and m.cache is not None
        assert e.peer.fp8 == (table_dtype == "fp8")
        ref = build_model(cfg)
        m.cache.sample_every = 1  # small batches: sample every candidate
        g = torch.Generator().manual_seed(11 + rank)
        errs, rates = [], []
        for it in range(3):
            B = 24
            # the skewed stream's 40 hot ids, spread over the 997 rows (0, 25 .. 975): every
            # rank's range holds some, so every rank has hot REMOTE rows to cache (unscaled they
            # are rows 0 .. 39, all in rank 0's range, where nothing hot would be remote)
            ids = pc.skewed(B, cfg.num_fields, g) * 25
            wts = torch.rand(B, cfg.num_fields, generator=g)
            m.cache.reset_counts()
            out = m(ids, wts)
            errs.append((out - ref(ids, wts)).abs().max().item())
            rates.append(m.cache.hit_rate())
            m.cache.refresh()
        ck = None
        if path is not None:
            # a table-wise peer model saves; a row-wise one of another seed loads it
            tw = ShardedDLRM(_cfg(hot, table_dtype=table_dtype), ctx)
            assert not tw.emb.peer.row_wise and not tw.emb.rw
            save_sharded(tw, path)
            m2 = ShardedDLRM(_cfg(hot, table_dtype=table_dtype, seed=2), ctx, policy="row")
            assert m2.emb.peer.row_wise and not torch.equal(_store_bytes(m2.emb), _store_bytes(e))
            load_sharded(m2, path)
            ck = (torch.equal(_store_bytes(m2.emb), _store_bytes(e)), torch.equal(m2(ids, wts), tw(ids, wts)),
                  (m2(ids, wts) - ref(ids, wts)).abs().max().item())
        q.put((rank, max(errs), rates, m.cache.describe(), m.exchange_bytes(24), ck))
        shutdown()
    except Exception:  # pragma: no cover - surfaced by the assertion below
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def _run(world, hot, table_dtype, path=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, hot, table_dtype, path, q)) for r in range(world)]
    [p.start() for p in procs]
    res = {}
    for _ in range(world):
        r, *rest = q.get(timeout=240)
        res[r] = rest
    [p.join(timeout=60) for p in procs]
    for r in range(world):
        assert isinstance(res[r][0], float), f"rank {r} failed: {res[r][0]}"
    return res


@pytest.mark.slow
@pytest.mark.parametrize("table_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("world,hot", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_row_wise_peer_exchange_matches_unsharded(world, hot, table_dtype):
    for r, (err, rates, desc, xb, _) in _run(world, hot, table_dtype).items():
        assert err < 1e-5, f"rank {r}: row-wise peer-exchange scores differ by {err}"
        assert rates[0] == 0.0  # nothing cached before the first refresh
        assert rates[-1] > 0.3, rates  # the hot ids are served from the replica
        assert desc["hot_rows"] > 0 and desc["refreshes"] == 3
        assert xb > 0


@pytest.mark.slow
@pytest.mark.parametrize("table_dtype", ["bf16", "fp8"])
def test_table_wise_checkpoint_loads_row_wise(tmp_path, table_dtype):
    for r, (err, _, _, _, ck) in _run(2, 1, table_dtype, str(tmp_path / "ckpt")).items():
        same_rows, same_scores, err2 = ck
        assert same_rows and same_scores and err2 < 1e-5, (r, ck)
