"""Ranked outputs from the live server itself (ServingConfig.rank_on_gpu) on the
CPU backend: the step ranks every request (ops.rank_arena's host form), admit
lets requests naming sorted_prediction / sorted_index in, and the completer
encodes them - instead of CALLER_PATH and the general path."""
import concurrent.futures as cf
import os
import sys

import numpy as np
import pytest
import torch

from distributed_tf_serving_amd.client.synth import SyntheticRequests
from distributed_tf_serving_amd.config import load_preset
from distributed_tf_serving_amd.ops import native
from distributed_tf_serving_amd.serving.server import ModelServer
from distributed_tf_serving_amd.wire import schema as pb
from distributed_tf_serving_amd.wire import tensor as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_cases as rc  # noqa: E402

F = 43
ALL = ["prediction_node", "sorted_prediction", "sorted_index"]


def _server(rank_on_gpu):
    cfg = load_preset("wdl_tiny_cpu")
    cfg.serving.max_batch_rows = 64
    cfg.serving.allowed_batch_sizes = (8, 64)
    cfg.serving.batch_timeout_us = 2000
    cfg.serving.rank_on_gpu = rank_on_gpu
    return ModelServer(cfg, device="cpu")


@pytest.fixture(scope="module")
def server():
    srv = _server(True)
    yield srv
    srv.stop()


def _request(rows, seed, flt):
    ids, wts = SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=seed).arrays(rows)
    t = [("feat_ids", torch.from_numpy(ids)), ("feat_wts", torch.from_numpy(wts))]
    return native().encode_predict_request("DCN", "serving_default", None, t, True, flt), ids, wts


def _outputs(resp: bytes):
    r = pb.PredictResponse.FromString(resp)
    return {k: T.to_ndarray(v) for k, v in r.outputs.items()}


def _check_ranked(out, rows):
    got = out["prediction_node"]
    assert got.shape == (rows,)
    order = rc.ref_order(got)
    if "sorted_index" in out:
        assert out["sorted_index"].dtype == np.int64 and np.array_equal(out["sorted_index"], order)
    if "sorted_prediction" in out:
        assert np.array_equal(rc.bits(out["sorted_prediction"]), rc.bits(got[order]))


def test_ranked_request_is_served_by_the_live_server(server):
    live = server.registry.resolve("DCN").scheduler
    assert live.ranks
    data, ids, wts = _request(40, 3, ALL)
    code, msg, resp = live.predict_raw(data, 10.0)
    assert code == 0, msg  # CALLER_PATH without the feature
    out = _outputs(resp)
    assert set(out) == set(ALL)
    _check_ranked(out, 40)
    m = server.registry.resolve("DCN").model
    want = m(torch.from_numpy(ids), torch.from_numpy(wts)).numpy()
    np.testing.assert_allclose(out["prediction_node"], want, atol=1e-5)
    # the wire carries them in the general path's order
    assert resp.index(b"prediction_node") < resp.index(b"sorted_prediction") < resp.index(b"sorted_index")


def test_filter_naming_only_the_index_returns_only_it(server):
    live = server.registry.resolve("DCN").scheduler
    data, ids, wts = _request(17, 5, ["sorted_index"])
    code, msg, resp = live.predict_raw(data, 10.0)
    assert code == 0, msg
    out = _outputs(resp)
    assert list(out) == ["sorted_index"]
    # its order is that of the scores the same server returns for the same rows
    code, msg, plain = live.predict_raw(_request(17, 5, [])[0], 10.0)
    assert code == 0, msg
    assert np.array_equal(out["sorted_index"], rc.ref_order(_outputs(plain)["prediction_node"]))


def test_empty_ranked_request(server):
    live = server.registry.resolve("DCN").scheduler
    code, msg, resp = live.predict_raw(_request(0, 1, ALL)[0], 10.0)
    assert code == 0, msg
    out = _outputs(resp)
    assert set(out) == set(ALL) and all(v.shape == (0,) for v in out.values())
    assert out["sorted_index"].dtype == np.int64


def test_ranked_and_plain_requests_share_a_step():
    """Eight requests, half of them ranked, admitted while the server is paused:
    they all run in one step, and each gets the outputs it asked for."""
    from distributed_tf_serving_amd.serving.live import LiveScheduler
    from distributed_tf_serving_amd.serving.server import build_engine

    cfg = load_preset("wdl_tiny_cpu")
    cfg.serving.max_batch_rows = 64
    cfg.serving.allowed_batch_sizes = (8, 64)
    cfg.serving.rank_on_gpu = True
    eng = build_engine(cfg, torch.device("cpu"), 3)
    live = LiveScheduler(eng, cfg.serving, start_paused=True)
    try:
        filters = [ALL, [], ["sorted_prediction"], ["prediction_node"], ["prediction_node", "sorted_index"], [], ALL,
                   []]
        reqs = [_request([5, 8, 3, 7, 6, 1, 4, 2][i], 10 + i, flt) for i, flt in enumerate(filters)]
        with cf.ThreadPoolExecutor(8) as pool:
            futs = [pool.submit(live.predict_raw, r[0], 20.0) for r in reqs]
            try:
                # every request admitted (or turned away: those have their answer already)
                deadline = native().now_us() + 10_000_000
                st = live.stats()
                while st["submitted"] + st["rejected"] < len(reqs) and native().now_us() < deadline:
                    st = live.stats()
            finally:
                live.resume()  # whatever happened: the admitted requests' threads wait for a step
            outs = [f.result(timeout=30) for f in futs]
        assert st["submitted"] == len(reqs) and st["steps"] == 0, st
        m = eng.ex.model
        for flt, (data, ids, wts), (code, msg, resp) in zip(filters, reqs, outs):
            assert code == 0, msg
            out = _outputs(resp)
            assert set(out) == set(flt or ["prediction_node"])
            want = m(torch.from_numpy(ids), torch.from_numpy(wts)).numpy()
            if "prediction_node" in out:
                np.testing.assert_allclose(out["prediction_node"], want, atol=1e-5)
                _check_ranked(out, ids.shape[0])
            else:  # sorted_prediction alone: the forward's scores, ranked
                np.testing.assert_allclose(out["sorted_prediction"], want[rc.ref_order(want)], atol=1e-5)
                assert np.all(np.diff(out["sorted_prediction"]) >= 0)
        st = live.stats()
        assert st["ranked"] == 4 and st["completed"] == 8 and st["steps"] == 1
    finally:
        live.close()


def test_service_answers_ranked_requests_from_the_fast_path(server):
    live = server.registry.resolve("DCN").scheduler
    before = live.stats()["ranked"]
    data, ids, wts = _request(33, 7, ALL)
    out = _outputs(server.service.predict_bytes(data, 10.0))
    _check_ranked(out, 33)
    assert live.stats()["ranked"] == before + 1


def test_flag_off_keeps_the_caller_path():
    srv = _server(False)
    try:
        live = srv.registry.resolve("DCN").scheduler
        assert not live.ranks
        data, ids, wts = _request(40, 3, ALL)
        code, msg, resp = live.predict_raw(data, 10.0)
        assert code == live.CALLER_PATH
        assert "ranked" in live.stats() and live.stats()["ranked"] == 0
        # ... and the service still serves it through the general path
        out = _outputs(srv.service.predict_bytes(data, 10.0))
        _check_ranked(out, 40)
    finally:
        srv.stop()
