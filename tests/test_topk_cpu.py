"""Top-k Predict outputs without a GPU: ops.topk_segments / topk_arena in their
CPU form, the arena's k table, the wire contract on the general path (bytes
and message entry points), the live server's CPU backend with rank_on_gpu, and
FanoutClient(top_k=N). The oracle is tests/rank_cases.py's reference order;
every comparison is exact."""
import concurrent.futures as cf
import os
import sys

import numpy as np
import pytest
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.client.backends import Backend, InProcessBackend
from distributed_tf_serving_amd.client.fanout_client import FanoutClient, RequestSpec
from distributed_tf_serving_amd.client.synth import SyntheticRequests
from distributed_tf_serving_amd.config import load_preset
from distributed_tf_serving_amd.ops import native
from distributed_tf_serving_amd.serving.arena import ArenaLayout
from distributed_tf_serving_amd.serving.errors import Code, ServingError
from distributed_tf_serving_amd.serving.server import ModelServer
from distributed_tf_serving_amd.wire import schema as pb
from distributed_tf_serving_amd.wire import tensor as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_cases as rc  # noqa: E402

F = 43
SV, SI = -7.5, -99
TOP = ["top_prediction", "top_index"]
ALL_TOP = ["prediction_node"] + TOP
ALL_SORTED = ["prediction_node", "sorted_prediction", "sorted_index"]


# ---------------------------------------------------------------- ops
def _expected(scores, segs, ks, into=None):
    vals, idx = into if into is not None else (np.full(scores.size, SV, dtype=np.float32),
                                               np.full(scores.size, SI, dtype=np.int64))
    for (a, b), k in zip(segs, ks):
        m = min(k, b - a)
        if m > 0:
            p = rc.ref_order(scores[a:b], True)[:m]
            vals[a:a + m] = scores[a:b][p]
            idx[a:a + m] = p
    return vals, idx


@pytest.mark.parametrize("rot", range(6))
def test_topk_segments_cpu_reference(rot):
    scores, offsets, segs = rc.make_buffer(rc.CPU_LENGTHS, seed=5)
    cyc = [lambda n: 0, lambda n: 1, lambda n: 10, lambda n: max(n - 1, 0), lambda n: n, lambda n: n + 5]
    ks = [cyc[(i + rot) % 6](b - a) for i, (a, b) in enumerate(segs)]
    vals, idx = torch.full((scores.size,), SV), torch.full((scores.size,), SI, dtype=torch.int64)
    s = torch.from_numpy(scores.copy())
    rv, ri = ops.topk_segments(s, offsets, ks, out=(vals, idx))
    assert rv is vals and ri is idx and np.array_equal(rc.bits(s), rc.bits(scores))
    want_v, want_i = _expected(scores, segs, ks)
    assert np.array_equal(idx.numpy(), want_i)  # sentinels past m and outside the segments included
    assert np.array_equal(rc.bits(vals), rc.bits(want_v))


def test_topk_segments_fresh_outputs_and_errors():
    scores, offsets, segs = rc.make_buffer((5, 0, 70), seed=2)
    v, i = ops.topk_segments(torch.from_numpy(scores), offsets, [2, 4, 100])
    want_v, want_i = _expected(scores, segs, [2, 4, 100],
                               into=(np.zeros(scores.size, np.float32), np.full(scores.size, -1, np.int64)))
    assert np.array_equal(i.numpy(), want_i) and np.array_equal(rc.bits(v), rc.bits(want_v))
    s = torch.zeros(100)
    for offsets, k in (([0, 50], [1, 1]), ([0, 50], [-1]), ([0, 50, 40], [1, 1]), ([0, 101], [1]), ([0, 50], [1.5])):
        with pytest.raises(ValueError):
            ops.topk_segments(s, offsets, k)


# ---------------------------------------------------------------- arena
def _req(rows, g, extra=(), flt=()):
    ids = torch.randint(0, 1 << 40, (rows, F), generator=g)
    wts = torch.rand(rows, F, generator=g)
    return native().encode_predict_request("DCN", "serving_default", None,
                                           [("feat_ids", ids), ("feat_wts", wts), *extra], True, list(flt))


def test_arena_without_topk_is_byte_identical():
    g = torch.Generator().manual_seed(1)
    A = ArenaLayout(F, 256)
    reqs = [_req(r, g) for r in (3, 17, 1, 40)]
    a0, a1, a2 = A.alloc(), A.alloc(), A.alloc()
    b0 = A.build(a0, A.place(a0, reqs), n_ranked=2)
    b1 = A.build(a1, A.place(a1, reqs), n_ranked=2, topk=())
    b2 = A.build(a2, A.place(a2, reqs), n_ranked=2, topk=[0, 0, 0, 0])
    assert b0.used_bytes == b1.used_bytes == b2.used_bytes
    assert torch.equal(a0, a1) and torch.equal(a0, a2)
    hdr = a2[:64].view(torch.int32)
    assert int(hdr[12]) == 0 and int(a2[56:64].view(torch.int64)[0]) == 0 and int(hdr[11]) == 2


def test_arena_k_table_and_header():
    g = torch.Generator().manual_seed(2)
    A = ArenaLayout(F, 256)
    reqs = [_req(r, g) for r in (3, 17, 1, 40)]
    plain, a = A.alloc(), A.alloc()
    b0 = A.build(plain, A.place(plain, reqs), n_ranked=1)
    b = A.build(a, A.place(a, reqs), n_ranked=1, topk=[5, 0, 2000, 7])
    hdr = a[:64].view(torch.int32)
    assert int(hdr[0]) == 4 and int(hdr[11]) == 1  # n_ranked keeps its meaning
    assert int(hdr[12]) == 3
    tab = int(a[56:64].view(torch.int64)[0])
    assert tab > 0 and tab % 64 == 0
    t0 = A.payload_off + tab
    assert a[t0:t0 + 16].view(torch.int32).tolist() == [5, 0, 2000, 7]
    assert b.used_bytes == t0 + 16 and b.used_bytes > b0.used_bytes
    # everything in front of the table, header words 48..63 aside, is the plain arena
    assert torch.equal(a[:48], plain[:48]) and torch.equal(a[64:b0.used_bytes], plain[64:b0.used_bytes])
    for bad in ([1, 2], [1, -1, 0, 0]):
        with pytest.raises(ValueError):
            A.build(a, A.place(a, reqs), topk=bad)


def test_arena_k_table_skips_a_request_without_descriptor():
    """A request the build rejects gets no descriptor: the table is per
    descriptor, as the kernel reads it."""
    g = torch.Generator().manual_seed(3)
    A = ArenaLayout(F, 256)
    reqs = [_req(4, g), b"\xff\xff\xff", _req(6, g)]
    a = A.alloc()
    b = A.build(a, A.place(a, reqs), topk=[3, 9, 2])
    assert b.errors[1] and b.n_valid == 2
    t0 = A.payload_off + int(a[56:64].view(torch.int64)[0])
    assert a[t0:t0 + 8].view(torch.int32).tolist() == [3, 2] and int(a[:64].view(torch.int32)[12]) == 2


def test_topk_arena_cpu_behind_rank_arena():
    g = torch.Generator().manual_seed(4)
    rows, ks = (1, 37, 50, 90), (5, 0, 50, 2000)
    B = 256
    A = ArenaLayout(F, B)
    reqs = [_req(r, g) for r in rows]
    rng = np.random.default_rng(9)
    scores = np.concatenate([rc.segment_scores(r, rng) for r in rows] + [rng.random(B - sum(rows), dtype=np.float32)])
    for topk, n_ranked in ((ks, 0), ((), 0), (ks, 1)):
        a = A.alloc()
        ab = A.build(a, A.place(a, reqs), n_ranked=n_ranked, topk=topk)
        segs = [(o, o + r) for o, r in zip(ab.offsets, ab.rows)]
        vals, idx = torch.full((B,), SV), torch.full((B,), SI, dtype=torch.int64)
        if n_ranked:
            ops.rank_arena(a, torch.from_numpy(scores), vals, idx)
        ops.topk_arena(a, torch.from_numpy(scores), vals, idx)
        want = rc.expected(scores, segs if n_ranked else [], False, -1, SV, SI)
        want_v, want_i = _expected(scores, segs, topk or [0] * 4, into=want)
        assert np.array_equal(idx.numpy(), want_i) and np.array_equal(rc.bits(vals), rc.bits(want_v))


# ---------------------------------------------------------------- general path
def _server(rank_on_gpu):
    cfg = load_preset("wdl_tiny_cpu")
    cfg.serving.max_batch_rows = 64
    cfg.serving.allowed_batch_sizes = (8, 64)
    cfg.serving.batch_timeout_us = 2000
    cfg.serving.rank_on_gpu = rank_on_gpu
    return ModelServer(cfg, device="cpu")


@pytest.fixture(scope="module")
def plain_server():
    """rank_on_gpu off: top-k requests take the general path."""
    srv = _server(False)
    yield srv
    srv.stop()


@pytest.fixture(scope="module")
def ranking_server():
    srv = _server(True)
    yield srv
    srv.stop()


def _arrays(rows, seed):
    return SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=seed).arrays(rows)


def _k_tensor(k, dtype=torch.int64, shape=(1,)):
    return ("top_k", torch.tensor(k, dtype=dtype).reshape(shape))


def _bytes_request(rows, seed, flt, k_input=None, raw=True):
    ids, wts = _arrays(rows, seed)
    t = [("feat_ids", torch.from_numpy(ids)), ("feat_wts", torch.from_numpy(wts))]
    if k_input is not None:
        t.append(k_input)
    return native().encode_predict_request("DCN", "serving_default", None, t, raw, list(flt))


def _message_request(rows, seed, flt, k_proto=None):
    ids, wts = _arrays(rows, seed)
    r = pb.PredictRequest()
    r.model_spec.name = "DCN"
    r.inputs["feat_ids"].CopyFrom(T.make_tensor_proto(ids))
    r.inputs["feat_wts"].CopyFrom(T.make_tensor_proto(wts))
    if k_proto is not None:
        r.inputs["top_k"].CopyFrom(k_proto)
    r.output_filter.extend(flt)
    return r


def _k_proto(k, dtype=None, shape=(), raw=False, values=None):
    dtype = pb.DT_INT64 if dtype is None else dtype
    p = pb.TensorProto()
    p.dtype = dtype
    p.tensor_shape.CopyFrom(T.make_shape(shape))
    vals = [k] if values is None else values
    if raw:
        p.tensor_content = np.asarray(vals, dtype="<i4" if dtype == pb.DT_INT32 else "<i8").tobytes()
    elif dtype == pb.DT_INT32:
        p.int_val.extend(vals)
    elif dtype == pb.DT_INT64:
        p.int64_val.extend(vals)
    else:
        p.float_val.extend(float(v) for v in vals)
    return p


def _outputs(resp):
    r = pb.PredictResponse.FromString(resp) if isinstance(resp, bytes) else resp
    return {k: T.to_ndarray(v) for k, v in r.outputs.items()}


def _wire_order(resp: bytes, keys):
    pos = [resp.index(k.encode() + b"\x12") for k in keys]  # map key, then the value field's tag
    return pos == sorted(pos)


def _check_top(out, rows, k):
    got = out["prediction_node"]
    assert got.shape == (rows,)
    head = rc.ref_order(got, True)[:min(k, rows)]
    assert out["top_index"].dtype == np.int64 and out["top_index"].shape == (min(k, rows),)
    assert np.array_equal(out["top_index"], head)
    assert out["top_prediction"].dtype == np.float32
    assert np.array_equal(rc.bits(out["top_prediction"]), rc.bits(got[head]))


@pytest.mark.parametrize("rows,k", [(40, 5), (40, 40), (40, 100), (1, 1), (0, 3)])
def test_general_path_bytes(plain_server, rows, k):
    data = _bytes_request(rows, 3, ALL_TOP, _k_tensor(k))
    out = _outputs(plain_server.service.predict_bytes(data, 10.0))
    assert set(out) == set(ALL_TOP)
    _check_top(out, rows, k)


@pytest.mark.parametrize("rows,k", [(40, 5), (40, 100), (0, 3)])
def test_general_path_message(plain_server, rows, k):
    resp = plain_server.service.predict(_message_request(rows, 4, ALL_TOP, _k_proto(k)), 10.0)
    out = _outputs(resp)
    assert set(out) == set(ALL_TOP)
    _check_top(out, rows, k)


def test_top_k_encodings_bytes_and_message(plain_server):
    """int32 / int64, [] / [1], tensor_content / typed field."""
    svc = plain_server.service
    want = None
    for dtype in (torch.int32, torch.int64):
        for shape in ((), (1,)):
            for raw in (False, True):
                data = _bytes_request(30, 8, ALL_TOP, _k_tensor(7, dtype, shape), raw=raw)
                out = _outputs(svc.predict_bytes(data, 10.0))
                _check_top(out, 30, 7)
                want = out if want is None else want
                assert np.array_equal(out["top_index"], want["top_index"])
    for dtype in (pb.DT_INT32, pb.DT_INT64):
        for shape in ((), (1,)):
            for raw in (False, True):
                out = _outputs(svc.predict(_message_request(30, 8, ALL_TOP, _k_proto(7, dtype, shape, raw)), 10.0))
                _check_top(out, 30, 7)
                assert np.array_equal(out["top_index"], want["top_index"])


def test_output_order_and_sorted_with_top(plain_server):
    flt = ["top_index", "sorted_index", "prediction_node", "top_prediction", "sorted_prediction"]  # any order asked
    data = _bytes_request(25, 9, flt, _k_tensor(4))
    resp = plain_server.service.predict_bytes(data, 10.0)
    out = _outputs(resp)
    assert set(out) == set(flt)
    assert _wire_order(resp, ["prediction_node", "sorted_prediction", "sorted_index", "top_prediction", "top_index"])
    _check_top(out, 25, 4)
    order = rc.ref_order(out["prediction_node"])
    assert np.array_equal(out["sorted_index"], order)
    assert np.array_equal(rc.bits(out["sorted_prediction"]), rc.bits(out["prediction_node"][order]))
    # the top outputs alone; an empty filter still returns prediction_node alone, top_k ignored
    only = _outputs(plain_server.service.predict_bytes(_bytes_request(25, 9, TOP, _k_tensor(4)), 10.0))
    assert set(only) == set(TOP) and np.array_equal(only["top_index"], out["top_index"])
    none = _outputs(plain_server.service.predict_bytes(_bytes_request(25, 9, [], _k_tensor(4)), 10.0))
    assert list(none) == ["prediction_node"]
    # a top_k nobody reads may be anything
    junk = _outputs(plain_server.service.predict_bytes(_bytes_request(25, 9, ALL_SORTED, _k_tensor(-3)), 10.0))
    assert set(junk) == set(ALL_SORTED)


BAD_K = [("missing", None), ("zero", _k_tensor(0)), ("negative", _k_tensor(-2)),
         ("float", ("top_k", torch.tensor([3.0]))), ("two_values", _k_tensor([3, 4], shape=(2,))),
         ("matrix", _k_tensor([3], shape=(1, 1)))]


@pytest.mark.parametrize("name,k_input", BAD_K, ids=[n for n, _ in BAD_K])
def test_errors_name_top_k_bytes(plain_server, ranking_server, name, k_input):
    data = _bytes_request(12, 2, ALL_TOP, k_input)
    for srv in (plain_server, ranking_server):  # the general path and the native server's admit
        with pytest.raises(ServingError) as e:
            srv.service.predict_bytes(data, 10.0)
        assert e.value.code == Code.INVALID_ARGUMENT and "top_k" in str(e.value)
    live = ranking_server.registry.resolve("DCN").scheduler
    code, msg, _ = live.predict_raw(data, 10.0)
    assert code == int(Code.INVALID_ARGUMENT) and "top_k" in msg


def test_errors_name_top_k_message(plain_server):
    bad = [None, _k_proto(0), _k_proto(-1), _k_proto(3, dtype=pb.DT_FLOAT), _k_proto(3, shape=(2,), values=[3, 4]),
           _k_proto(3, shape=(1, 1)), _k_proto(3, values=[3, 4]), _k_proto(3, raw=True, values=[3, 4]),
           _k_proto(3, values=[])]
    for k_proto in bad:
        with pytest.raises(ServingError) as e:
            plain_server.service.predict(_message_request(12, 2, ALL_TOP, k_proto), 10.0)
        assert e.value.code == Code.INVALID_ARGUMENT and "top_k" in str(e.value)
    # the same value problems through the bytes entry (typed field with two values / none)
    for k_proto in (_k_proto(3, values=[3, 4]), _k_proto(3, raw=True, values=[3, 4]), _k_proto(3, values=[])):
        data = _message_request(12, 2, ALL_TOP, k_proto).SerializeToString()
        with pytest.raises(ServingError) as e:
            plain_server.service.predict_bytes(data, 10.0)
        assert e.value.code == Code.INVALID_ARGUMENT and "top_k" in str(e.value)


def test_metadata_lists_top_k(plain_server):
    req = pb.GetModelMetadataRequest()
    req.model_spec.name = "DCN"
    req.metadata_field.append("signature_def")
    resp = plain_server.service.get_model_metadata(req)
    sdm = pb.SignatureDefMap()
    resp.metadata["signature_def"].Unpack(sdm)
    sd = sdm.signature_def["serving_default"]
    assert sd.inputs["top_k"].dtype == pb.DT_INT64 and len(sd.inputs["top_k"].tensor_shape.dim) == 0
    assert sd.outputs["top_prediction"].dtype == pb.DT_FLOAT and sd.outputs["top_index"].dtype == pb.DT_INT64
    assert {"feat_ids", "feat_wts"} <= set(sd.inputs) and {"prediction_node", "sorted_index"} <= set(sd.outputs)
    s = plain_server.registry.resolve("DCN")
    assert (s.ids_key, s.wts_key) == ("feat_ids", "feat_wts")


# ---------------------------------------------------------------- live server, CPU backend
def test_live_server_answers_top_k_itself(ranking_server, plain_server):
    live = ranking_server.registry.resolve("DCN").scheduler
    assert live.ranks
    before = live.stats()
    data = _bytes_request(40, 3, ALL_TOP, _k_tensor(6))
    code, msg, resp = live.predict_raw(data, 10.0)
    assert code == 0, msg  # CALLER_PATH without the feature
    out = _outputs(resp)
    assert set(out) == set(ALL_TOP) and _wire_order(resp, ALL_TOP)
    _check_top(out, 40, 6)
    # the native answer is the general path's, byte for byte in every output
    ref = _outputs(plain_server.service.predict_bytes(data, 10.0))
    for k in ALL_TOP:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape
    assert np.array_equal(out["top_index"], ref["top_index"])
    # rows = 0 and k > rows
    code, msg, resp = live.predict_raw(_bytes_request(0, 1, ALL_TOP, _k_tensor(3)), 10.0)
    assert code == 0, msg
    empty = _outputs(resp)
    assert set(empty) == set(ALL_TOP) and all(v.shape == (0,) for v in empty.values())
    assert empty["top_index"].dtype == np.int64
    code, msg, resp = live.predict_raw(_bytes_request(9, 1, ALL_TOP, _k_tensor(500)), 10.0)
    assert code == 0, msg
    _check_top(_outputs(resp), 9, 500)
    # sorted and top outputs together: the general path's
    both = ALL_SORTED + TOP
    data = _bytes_request(20, 6, both, _k_tensor(3))
    assert live.predict_raw(data, 10.0)[0] == live.CALLER_PATH
    out = _outputs(ranking_server.service.predict_bytes(data, 10.0))
    assert set(out) == set(both)
    _check_top(out, 20, 3)
    after = live.stats()
    assert after["topk"] - before["topk"] == 2 and after["ranked"] == before["ranked"]


def test_flag_off_keeps_the_caller_path(plain_server):
    live = plain_server.registry.resolve("DCN").scheduler
    assert not live.ranks
    code, msg, _ = live.predict_raw(_bytes_request(10, 3, ALL_TOP, _k_tensor(2)), 10.0)
    assert code == live.CALLER_PATH and live.stats()["topk"] == 0


def test_plain_sorted_and_top_requests_share_a_step():
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.server import build_engine

    cfg = load_preset("wdl_tiny_cpu")
    cfg.serving.max_batch_rows = 64
    cfg.serving.allowed_batch_sizes = (8, 64)
    cfg.serving.rank_on_gpu = True
    eng = build_engine(cfg, torch.device("cpu"), 3)
    live = LiveScheduler(eng, cfg.serving, start_paused=True)
    try:
        plan = [(5, ALL_TOP, 2), (8, [], None), (3, ALL_SORTED, None), (7, ["prediction_node", "top_index"], 100),
                (6, ALL_SORTED, None), (1, [], None), (4, ALL_TOP, 4), (2, ["top_prediction", "prediction_node"], 1)]
        reqs = [_bytes_request(rows, 10 + i, flt, None if k is None else _k_tensor(k))
                for i, (rows, flt, k) in enumerate(plan)]
        with cf.ThreadPoolExecutor(8) as pool:
            futs = [pool.submit(live.predict_raw, r, 20.0) for r in reqs]
            try:
                deadline = native().now_us() + 10_000_000
                st = live.stats()
                while st["submitted"] + st["rejected"] < len(reqs) and native().now_us() < deadline:
                    st = live.stats()
            finally:
                live.resume()  # whatever happened: the admitted requests' threads wait for a step
            outs = [f.result(timeout=30) for f in futs]
        assert st["submitted"] == len(reqs) and st["steps"] == 0, st
        for (rows, flt, k), (code, msg, resp) in zip(plan, outs):
            assert code == 0, msg
            out = _outputs(resp)
            assert set(out) == set(flt or ["prediction_node"])
            got = out["prediction_node"]
            if k is not None:
                head = rc.ref_order(got, True)[:min(k, rows)]
                if "top_index" in out:
                    assert np.array_equal(out["top_index"], head)
                if "top_prediction" in out:
                    assert np.array_equal(rc.bits(out["top_prediction"]), rc.bits(got[head]))
            elif flt:
                order = rc.ref_order(got)
                assert np.array_equal(out["sorted_index"], order)
                assert np.array_equal(rc.bits(out["sorted_prediction"]), rc.bits(got[order]))
        st = live.stats()
        assert st["topk"] == 4 and st["ranked"] == 2 and st["completed"] == 8 and st["steps"] == 1
    finally:
        live.close()


# ---------------------------------------------------------------- client
class _TableBackend(Backend):
    """Scores rows by a table: a row's first id is its global candidate index.
    Answers top_prediction / top_index in the reference order, like a server."""

    def __init__(self, table, name):
        self.table, self.name, self.calls = table, name, 0

    def predict(self, data, timeout_s=None):
        self.calls += 1
        req = pb.PredictRequest.FromString(data)
        assert list(req.output_filter) == TOP  # the client asks for nothing else
        k = int(T.to_ndarray(req.inputs["top_k"]).reshape(-1)[0])
        scores = self.table[T.to_ndarray(req.inputs["feat_ids"])[:, 0]]
        head = rc.ref_order(scores, True)[:k]
        resp = pb.PredictResponse()
        resp.outputs["top_prediction"].CopyFrom(T.make_tensor_proto(scores[head]))
        resp.outputs["top_index"].CopyFrom(T.make_tensor_proto(head.astype(np.int64)))
        return resp.SerializeToString()


class _DeadBackend(Backend):
    name = "dead"

    def predict(self, data, timeout_s=None):
        raise RuntimeError("down")


def _table(n, seed):
    """Few distinct values: ties inside every shard and across every boundary,
    with NaN, both zeros and the infinities among them."""
    rng = np.random.default_rng(seed)
    t = (rng.integers(0, 4, n).astype(np.float32) - 1) / 2
    t[rng.choice(n, 6, replace=False)] = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    return t


@pytest.mark.parametrize("n,shards,k,full_async", [(103, 4, 10, True), (103, 4, 60, False), (16, 5, 30, True),
                                                   (64, 3, 1, True), (7, 8, 3, True)])
def test_fanout_client_merges_the_global_top_n(n, shards, k, full_async):
    table = _table(n, n + k)
    ids = np.zeros((n, F), dtype=np.int64)
    ids[:, 0] = np.arange(n)
    backends = [_TableBackend(table, f"b{i}") for i in range(shards)]
    cl = FanoutClient(backends, RequestSpec(), top_k=k, full_async=full_async)
    try:
        res = cl.predict(ids, np.ones((n, F), np.float32))
    finally:
        cl.close()
    head = rc.ref_order(table, True)[:k]
    assert res.top_index.dtype == torch.int64 and np.array_equal(res.top_index.numpy(), head)
    assert np.array_equal(rc.bits(res.top_scores), rc.bits(table[head]))
    assert res.scores.numel() == 0 and res.sorted_scores is None


def test_fanout_client_top_k_with_failover_and_defaults():
    n, k = 90, 25
    table = _table(n, 1)
    ids = np.zeros((n, F), dtype=np.int64)
    ids[:, 0] = np.arange(n)
    cl = FanoutClient([_TableBackend(table, "a"), _DeadBackend(), _TableBackend(table, "c")], top_k=k, failover=True)
    try:
        res = cl.predict(ids, np.ones((n, F), np.float32))
        assert cl.failovers == 1
    finally:
        cl.close()
    head = rc.ref_order(table, True)[:k]
    assert np.array_equal(res.top_index.numpy(), head) and np.array_equal(rc.bits(res.top_scores), rc.bits(table[head]))
    with pytest.raises(ValueError):
        FanoutClient([_DeadBackend()], top_k=0)


def test_fanout_client_over_in_process_servers(plain_server):
    ids, wts = _arrays(50, 21)
    plain = FanoutClient([InProcessBackend(plain_server.service)] * 3, sort_scores=False)
    top = FanoutClient([InProcessBackend(plain_server.service)] * 3, top_k=8)
    try:
        scores = plain.predict(ids, wts)
        res = top.predict(ids, wts)
        assert scores.top_scores is None and scores.top_index is None  # default: today's result
    finally:
        plain.pool.shutdown(wait=True)
        top.pool.shutdown(wait=True)
    head = rc.ref_order(scores.scores.numpy(), True)[:8]
    assert np.array_equal(res.top_index.numpy(), head)
    assert np.array_equal(rc.bits(res.top_scores), rc.bits(scores.scores.numpy()[head]))


def test_simple_client_builds_a_top_k_request(plain_server):
    from distributed_tf_serving_amd.client.simple import build_request, top_entries

    assert "top_k" not in build_request().inputs and not build_request().output_filter
    req = build_request(top_k=1)
    resp = pb.PredictResponse.FromString(plain_server.service.predict_bytes(req.SerializeToString(), 10.0))
    out = _outputs(resp)
    _check_top(out, 2, 1)
    assert top_entries(resp) == [(int(out["top_index"][0]), float(out["top_prediction"][0]))]
