"""fp8 tables across ranks on the CPU (parallel/hot_cache.py PeerTables with
scales, ShardedEmbedding table_dtype fp8, sharded checkpoints): the fp8 peer
lookup is the bf16 one on the dequantised stores, exactly; two gloo ranks
score like the unsharded fp8 DLRM and hold its code rows byte for byte; the
checkpoint round-trips codes and scales at the same and at another world
size; every other fp8 combination is still rejected; and the GPU test's exact
probe is shown rounding-free before a GPU is asked."""
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_fp8_cases as pc  # noqa: E402

from distributed_tf_serving_amd import ops  # noqa: E402
from distributed_tf_serving_amd.config import ModelConfig, load_preset  # noqa: E402
from distributed_tf_serving_amd.parallel.hot_cache import (KEY_SHIFT, HotRowCache, PeerTables,  # noqa: E402
                                                           auto_capacity, peer_gather_cpu)

F8 = torch.float8_e4m3fn


def _u8(x):
    return x.view(torch.uint8)


# ------------------------------------------------------- lookup, cache, counters
@pytest.mark.parametrize("chunk_shift", [None, 4])
def test_fp8_peer_gather_is_the_bf16_gather_on_dequantised_stores(chunk_shift):
    g = torch.Generator().manual_seed(0)
    ts = pc.TwoStores(4, 50, (1, 3), g)
    assert ts.scale.unique().numel() == 4
    ts.plant(1, 7, pc.EXTREMES.repeat(8))
    p8, p16 = ts.peer_fp8(chunk_shift), ts.peer_bf16(chunk_shift)
    assert p8.fp8 and p8.dtype == F8 and not p16.fp8 and "tscale" in p8.kernel_args() and "tscale" not in p16.kernel_args()
    if chunk_shift:
        assert p8.chunk_shift == 4 and len(p8.stores[1]) == 13
    # raw rows come back in the store dtype
    t, v = torch.tensor([1, 0]), torch.tensor([7, 3])
    raw = p8.row_cpu(t, v)
    assert raw.dtype == F8 and torch.equal(_u8(raw)[0], pc.EXTREMES.repeat(8))
    assert torch.equal(_u8(raw)[1], _u8(ts.codes[0])[3])
    c8 = HotRowCache(p8, capacity=8, ring_cap=64, sample_every=1, fill=0.75)
    c16 = HotRowCache(p16, capacity=8, ring_cap=64, sample_every=1, fill=0.75)
    assert c8.rows.dtype == F8 and c16.rows.dtype == torch.bfloat16
    ids = torch.tensor([[r % 6 if i % 3 else r % 10 for i in range(4)] for r in range(30)])
    ids[3] -= 50 * 11  # negative ids
    ids[:, 1] = torch.where(torch.arange(30) % 2 == 0, 7, ids[:, 1])  # the planted row is hot
    bag_ids = torch.cat([ids, ids + 1, ids * 3], 1)[:, [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]]
    wts = torch.rand(30, 12, generator=g)
    for rnd in range(2):  # before a refresh (all misses) and after (hits)
        for c in (c8, c16):
            c.reset_counts()
        a = peer_gather_cpu(p8, c8, ids, None, 1)
        b = peer_gather_cpu(p16, c16, ids, None, 1)
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
        assert torch.equal(a, peer_gather_cpu(p8, None, ids, None, 1))
        a3 = peer_gather_cpu(p8, c8, bag_ids, wts, 3)
        assert a3.dtype == torch.bfloat16 and torch.equal(a3, peer_gather_cpu(p16, c16, bag_ids, wts, 3))
        assert torch.equal(a3, peer_gather_cpu(p8, None, bag_ids, wts, 3))
        # counters and ring pushes of the bf16 twin
        assert c8.counts() == c16.counts() and sum(c8.counts()) == 30 * 2 * 4
        assert (c8.counts()[0] == 0) == (rnd == 0)
        assert torch.equal(c8.ring_ctr, c16.ring_ctr) and torch.equal(c8.ring, c16.ring)
        n8, n16 = c8.refresh(), c16.refresh()
        assert n8 == n16 and torch.equal(c8.keys, c16.keys) and torch.equal(c8.slots, c16.slots)
        # a cached row is its owner's code bytes, verbatim
        kt, kv = c8.keys >> KEY_SHIFT, c8.keys & ((1 << KEY_SHIFT) - 1)
        assert c8.keys.numel() == 6
        assert torch.equal(_u8(c8.rows)[c8.slots.long()], _u8(p8.row_cpu(kt, kv)))
    assert (1 << KEY_SHIFT) + 7 in c8.keys.tolist()  # the extremes row went through the cache


def test_ops_dispatch_on_the_store_dtype_and_return_bf16():
    g = torch.Generator().manual_seed(1)
    ts = pc.TwoStores(4, 50, (1, 3), g)
    p8, p16 = ts.peer_fp8(), ts.peer_bf16()
    ids = pc.skewed(9, 3 + 8, g)
    wts = torch.rand(9, 3 + 8, generator=g)
    dense = torch.randn(9, 64, generator=g).to(torch.bfloat16)
    z8, z16 = (ops.dot_interaction_gather_peer(dense, ids, p, None, id_col0=3) for p in (p8, p16))
    assert z8.dtype == torch.bfloat16 and torch.equal(z8, z16)
    b8, b16 = (ops.peer_bag(ids, wts, 9, 3, 2, p, None) for p in (p8, p16))
    assert b8.dtype == torch.bfloat16 and b8.shape == (9, 4, 64) and torch.equal(b8, b16)


def test_auto_capacity_prices_fp8_rows_at_160_bytes():
    from distributed_tf_serving_amd.parallel.hot_cache import CACHE_BYTES_PER_ROW, cache_bytes_per_row

    assert CACHE_BYTES_PER_ROW == 224 == cache_bytes_per_row(torch.bfloat16) and cache_bytes_per_row(F8) == 160
    g = torch.Generator().manual_seed(2)
    ts = pc.TwoStores(2, 50, (1,), g)
    free = 10 ** 8
    for p, per in ((ts.peer_fp8(), 160), (ts.peer_bf16(), 224)):
        p.rows = [50, 10 ** 9]  # a billion-row remote table (the stores stay small: capacity math only)
        assert auto_capacity(p, free_bytes=free, fraction=1.0) == free // per
        assert auto_capacity(p, free_bytes=4 * free) == free // per  # the default quarter


# ------------------------------------------------------------------ rejections
def _cfg(hot=1, rows=997, **kw):
    kw.setdefault("table_dtype", "fp8")
    kw.setdefault("embedding_exchange", "peer")
    return ModelConfig(family="dlrm", num_fields=5 + 5 * hot, num_dense=5, table_rows=rows, embed_dim=64,
                       bottom_mlp=(32, 64), mlp_dims=(64, 32), multi_hot=hot, hot_cache_rows=1024, **kw)


def test_rejections():
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import (ShardedDLRM, ShardedEmbedding, TableSpec,
                                                                        _reject_fp8_tables, build_parallel_model,
                                                                        plan_sharding)

    one = DistContext(device=torch.device("cpu"))
    # one rank, even with the peer exchange asked for
    with pytest.raises(ValueError, match="single-rank.*embedding_exchange: peer"):
        ShardedDLRM(_cfg(), one, device="cpu")
    with pytest.raises(ValueError, match="single-rank"):
        build_parallel_model(_cfg(), "cpu", shard_tables="on")
    # more than one rank, any exchange but an explicit "peer"
    for ex in ("auto", "alltoall"):
        with pytest.raises(ValueError, match="single-rank"):
            _reject_fp8_tables(_cfg(embedding_exchange=ex), 2)
        with pytest.raises(ValueError, match="single-rank"):
            ShardedDLRM(_cfg(embedding_exchange=ex), one, device="cpu")
    _reject_fp8_tables(_cfg(), 2)  # the supported combination
    _reject_fp8_tables(_cfg(table_dtype="bf16", embedding_exchange="auto"), 1)
    # the embedding itself: fp8 stores only behind the peer exchange, table-wise
    tables = [TableSpec(f"t{i}", 40, 64, 1) for i in range(3)]
    with pytest.raises(ValueError, match="peer"):
        ShardedEmbedding(plan_sharding(tables, 1, policy="table"), one, 1, 0.125, table_dtype="fp8")
    with pytest.raises(ValueError, match="table_dtype"):
        ShardedEmbedding(plan_sharding(tables, 1, policy="table"), one, 1, 0.125, exchange="peer", table_dtype="int8")
    # PeerTables: codes and scale come together, one dtype on every rank
    g = torch.Generator().manual_seed(3)
    codes, bf = pc.random_codes(20, g), torch.zeros(20, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="scale"):
        PeerTables([codes], [0], [0], [20], rank=0)
    with pytest.raises(ValueError, match="scale"):
        PeerTables([bf], [0], [0], [20], rank=0, scale=torch.ones(1))
    with pytest.raises(ValueError, match="one dtype"):
        PeerTables([codes, bf], [0, 1], [0, 0], [20, 20], rank=0, scale=torch.ones(2))
    with pytest.raises(ValueError, match="per table"):
        PeerTables([codes], [0], [0], [20], rank=0, scale=torch.ones(2))


def test_preset_loads():
    cfg, ref = load_preset("dlrm_fp8_sharded8"), load_preset("dlrm_sharded8")
    assert cfg.model.table_dtype == "fp8" and cfg.model.embedding_exchange == "peer" and cfg.client.backends == 8
    import dataclasses

    a, b = dataclasses.asdict(cfg.model), dataclasses.asdict(ref.model)
    assert {k for k in a if a[k] != b[k]} == {"table_dtype", "embedding_exchange"}
    assert dataclasses.asdict(cfg.serving) == dataclasses.asdict(ref.serving)
    from distributed_tf_serving_amd.parallel.embedding_sharding import dlrm_tables, plan_sharding

    # a rank's shard of config 4: 24 GB of codes where bf16 rows take 48 GB
    fp8, bf16 = (max(plan_sharding(dlrm_tables(c.model), 8, policy="table").rank_bytes()) for c in (cfg, ref))
    assert fp8 * 2 == bf16 == 4 * 100_000_000 * 64 * 2


# -------------------------------------------------------------- two gloo ranks
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _store_bytes(emb):
    return torch.cat([_u8(c.data) for c in [emb.store, *emb.store_chunks]])


def _check_store(emb, ref_q):
    """Every row of this rank's store is the same row of the unsharded model's emb_q."""
    store, R = _store_bytes(emb), emb.plan.tables[0].rows
    for t, lo, n, off in emb.segments:
        assert torch.equal(store[off:off + n], _u8(ref_q)[t * R + lo:t * R + lo + n]), f"table {t}"


def _worker(rank, world, port, hot, chunk_shift, path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from distributed_tf_serving_amd.models import build_model
    from distributed_tf_serving_amd.parallel import hot_cache
    from distributed_tf_serving_amd.parallel.dist import init_from_env, shutdown
    from distributed_tf_serving_amd.parallel.embedding_sharding import ShardedDLRM
    from distributed_tf_serving_amd.utils.checkpoint import load_sharded, save_sharded

    try:
        if chunk_shift is not None:  # stores split into many small chunks
            hot_cache.CHUNK_SHIFT = chunk_shift
        ctx = init_from_env(device="cpu")
        cfg = _cfg(hot)
        m = ShardedDLRM(cfg, ctx)
        e = m.emb
        assert e.store.dtype == F8 and e.peer.fp8 and e.cache.rows.dtype == F8 and not m.has_collectives
        if chunk_shift is not None:
            assert e.peer.chunk_shift == chunk_shift and len(e.peer.stores[1 - rank]) > 10
        ref = build_model(cfg)
        assert ref.emb_q.dtype == F8 and torch.equal(e.emb_scale, ref.emb_scale)
        _check_store(e, ref.emb_q)
        # the bf16 twin: twice the bytes per local row, everything else the same
        mb = ShardedDLRM(_cfg(hot, table_dtype="bf16"), ctx)
        assert mb.param_bytes() - m.param_bytes() == e.rows_local * 64 == e.local_bytes()
        assert mb.emb.local_bytes() == 2 * e.local_bytes() and mb.exchange_bytes(24) == 2 * m.exchange_bytes(24) > 0
        assert m.alloc(24).get("emb_all", torch.zeros(1, dtype=torch.bfloat16)).dtype == torch.bfloat16
        m.cache.sample_every = 1  # small batches: sample every candidate
        g = torch.Generator().manual_seed(11 + rank)
        errs, rates, equal = [], [], True
        for it in range(3):
            B = 24
            ids = pc.skewed(B, cfg.num_fields, g)
            wts = torch.rand(B, cfg.num_fields, generator=g)
            m.cache.reset_counts()
            out, want = m(ids, wts), ref(ids, wts)
            equal = equal and torch.equal(out, want)
            errs.append((out - want).abs().max().item())
            rates.append(m.cache.hit_rate())
            m.cache.refresh()
        ck = None
        if path is not None:
            save_sharded(m, path)
            m2 = ShardedDLRM(_cfg(hot, seed=2), ctx)  # another init
            assert not torch.equal(_store_bytes(m2.emb), _store_bytes(e))
            m2.emb.set_table_scale(torch.full((e.T,), 4.0))
            load_sharded(m2, path)
            ck = (torch.equal(_store_bytes(m2.emb), _store_bytes(e)) and torch.equal(m2.emb.emb_scale, e.emb_scale)
                  and torch.equal(m2.emb.peer.scale, e.emb_scale) and torch.equal(m2.emb.peer.scale_cpu, e.emb_scale),
                  (m2(ids, wts) - ref(ids, wts)).abs().max().item())
            try:
                load_sharded(mb, path)
                ck += ("no error",)
            except ValueError as err:
                ck += (str(err),)
        q.put((rank, max(errs), equal, rates, m.cache.describe(), ck))
        shutdown()
    except Exception:  # pragma: no cover - surfaced by the assertion below
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def _run(hot, chunk_shift, path=None, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, hot, chunk_shift, path, q)) for r in range(world)]
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
@pytest.mark.parametrize("hot,chunk_shift", [(1, None), (3, None), (1, 6)])
def test_fp8_peer_exchange_matches_unsharded_fp8(hot, chunk_shift):
    for r, (err, equal, rates, desc, _) in _run(hot, chunk_shift).items():
        if hot == 1:  # the same CPU math on the same rows
            assert equal and err == 0.0, f"rank {r}: scores differ by {err}"
        else:
            assert err < 1e-5, f"rank {r}: peer-exchange scores differ by {err}"
        assert rates[0] == 0.0  # nothing cached before the first refresh
        assert rates[-1] > 0.3, rates  # the hot ids are served from the replica
        assert desc["hot_rows"] > 0 and desc["refreshes"] == 3


@pytest.mark.slow
def test_fp8_sharded_checkpoint_round_trips_and_reshards(tmp_path):
    """save_sharded at world 2 -> load_sharded at world 2 (in the workers) and
    into one rank holding every table: codes and scales come back byte-equal."""
    import json

    from distributed_tf_serving_amd.models import build_model
    from distributed_tf_serving_amd.models.ctr import DLRM
    from distributed_tf_serving_amd.parallel.dist import DistContext
    from distributed_tf_serving_amd.parallel.embedding_sharding import (ShardedDLRM, ShardedEmbedding, dlrm_tables,
                                                                        plan_sharding)
    from distributed_tf_serving_amd.utils.checkpoint import load_sharded

    path = str(tmp_path / "fp8_ckpt")
    for r, (err, equal, _, _, ck) in _run(1, None, path).items():
        same, err2, msg = ck
        assert same and err2 == 0.0, (r, ck)
        assert "fp8" in msg and "bf16" in msg, msg  # an fp8 checkpoint into a bf16 model
    with open(os.path.join(path, "manifest.json")) as f:
        man = json.load(f)
    cfg = _cfg()
    ref = build_model(cfg)
    assert man["world"] == 2 and man["model_config"]["table_dtype"] == "fp8"
    assert man["emb_scale"] == ref.emb_scale.tolist()
    from safetensors import safe_open

    with safe_open(os.path.join(path, "rank1.safetensors"), "pt") as f:
        assert all(f.get_tensor(k).dtype == torch.uint8 for k in f.keys() if k.startswith("table"))
    # one rank of the saved two: a ShardedDLRM refuses fp8 tables there, so the
    # target is its parts - the embedding with every table local + the towers
    one = DistContext(device=torch.device("cpu"))
    other = _cfg(seed=2)
    dense = DLRM(other, materialize_tables=False)
    emb = ShardedEmbedding(plan_sharding(dlrm_tables(other), 1, policy="table"), one, other.seed, dense.table_bound,
                           exchange="peer", col_base=other.num_dense, table_dtype="fp8")
    emb.set_table_scale(torch.full((emb.T,), 4.0))
    assert not torch.equal(_store_bytes(emb), _u8(ref.emb_q))
    load_sharded(SimpleNamespace(cfg=other, emb=emb, dense=dense), path)
    assert torch.equal(_store_bytes(emb), _u8(ref.emb_q)) and torch.equal(emb.emb_scale, ref.emb_scale)
    assert torch.equal(emb.peer.scale_cpu, ref.emb_scale)
    g = torch.Generator().manual_seed(5)
    ids = pc.skewed(16, cfg.num_fields, g)
    got = emb(ids)  # the eager lookup of the loaded rows
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref.lookup(ids, None).view(16, emb.T, 64))
    # and a bf16 checkpoint does not load into an fp8 model: covered by the message above in reverse
    with pytest.raises(ValueError, match="table_dtype"):
        load_sharded(SimpleNamespace(cfg=_cfg(table_dtype="bf16"), emb=emb, dense=dense), path)
    with pytest.raises(ValueError, match="single-rank"):
        ShardedDLRM(cfg, one)


# ------------------------------------------------------------------ exact probe
@pytest.mark.parametrize("T", [5, 31])
def test_exact_probe_is_rounding_free(T):
    """The GPU test's exact probe, before the GPU is asked: the fp32 reference
    equals a float64 computation, every magnitude is <= 256, and the CPU op
    (the GPU test's oracle) is that reference rounded to bf16."""
    ts, dense, ids = pc.exact_probe(T)
    assert len(ts.remote) == T // 2 and ts.scale.unique().tolist() == [0.125, 1.0]
    for c in ts.codes:
        assert torch.equal(c.float(), c.float().round()) and c.float().abs().max() == 2
    r32, r64 = pc.probe_reference(ts, dense, ids, torch.float32), pc.probe_reference(ts, dense, ids, torch.float64)
    assert torch.equal(r32.double(), r64)
    assert r64.abs().max() <= 256 and r64[:, 64:].abs().max() > 2
    assert torch.equal(r64 * 64, (r64 * 64).round())  # multiples of 2^-6
    z = ops.dot_interaction_gather_peer(dense, ids, ts.peer_fp8(), None)
    assert z.dtype == torch.bfloat16 and z.shape == r32.shape and torch.equal(z, r32.to(torch.bfloat16))
    assert torch.equal(z, ops.dot_interaction_gather_peer(dense, ids, ts.peer_bf16(), None))
    q, mod, off = ts.local()
    assert torch.equal(z, ops.dot_interaction_gather_fp8(dense, q, ts.scale, ids, mod, off))


def test_bag_probe_is_rounding_free():
    """The bag kernel's integer probe: codes in [-2, 2], weights in {0, 1, 2},
    scales 1 and 2^-3 - sums of at most 3 terms of magnitude <= 4, exact in any order."""
    ts, _, _ = pc.exact_probe(5)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(-(1 << 40), 1 << 40, (37, 15), generator=g)
    wts = torch.randint(0, 3, (37, 15), generator=g).float()
    a = peer_gather_cpu(ts.peer_fp8(), None, ids, wts, 3)
    v = torch.remainder(ids, ts.rows).view(37, 5, 3)
    want = torch.zeros(37, 5, 64, dtype=torch.float64)
    for t in range(5):
        rows = ts.codes[ts.owner[t]][ts.off[t] + v[:, t]].double() * ts.scale[t].double()  # [37, 3, 64]
        want[:, t] = (rows * wts.view(37, 5, 3)[:, t].double().unsqueeze(-1)).sum(1)
    assert want.abs().max() <= 256 and torch.equal(a.double(), want)
