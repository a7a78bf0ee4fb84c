"""Ranked outputs from the GPU live server's own step (ServingConfig.rank_on_gpu):
the captured step ends with the segmented rank kernel (csrc/kernels/rank.hip),
and requests naming sorted_prediction / sorted_index are answered by the native
server - same outputs as the general path of a server with the flag off."""
import concurrent.futures as cf
import os
import sys

import numpy as np
import pytest
import torch

from distributed_tf_serving_amd.client.synth import SyntheticRequests
from distributed_tf_serving_amd.config import load_preset
from distributed_tf_serving_amd.ops import native
from distributed_tf_serving_amd.wire import schema as pb
from distributed_tf_serving_amd.wire import tensor as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
F = 43
ALL = ["prediction_node", "sorted_prediction", "sorted_index"]


class _Served:
    """One servable behind a PredictionServiceImpl (what ModelServer sets up),
    built over a given model replica."""

    def __init__(self, rank_on_gpu, model=None):
        from distributed_tf_serving_amd.serving.registry import ModelRegistry
        from distributed_tf_serving_amd.serving.server import build_engine, build_servable
        from distributed_tf_serving_amd.serving.service import PredictionServiceImpl

        cfg = load_preset("deepfm_1gpu")
        cfg.model.vocab_size = 200_000
        cfg.serving.max_batch_rows = 2048
        cfg.serving.allowed_batch_sizes = (256, 2048)
        cfg.serving.rank_on_gpu = rank_on_gpu
        eng = build_engine(cfg, torch.device("cuda:0"), 3, model=model)
        self.registry = ModelRegistry()
        self.registry.load(build_servable(cfg, engine=eng))
        self.service = PredictionServiceImpl(self.registry, cfg.serving.request_timeout_s)
        self.model = eng.ex.model
        self.live = self.registry.resolve("DCN").scheduler

    def stop(self):
        self.live.close()


@pytest.fixture(scope="module")
def servers():
    """The server that ranks in its step and one with the flag off over the
    same weights."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    on = _Served(True)
    off = _Served(False, model=on.model)
    yield on, off
    on.stop()
    off.stop()


def _request(rows, seed, flt):
    ids, wts = SyntheticRequests(fields=F, id_space=1 << 40, dist="zipf", seed=seed).arrays(rows)
    t = [("feat_ids", torch.from_numpy(ids)), ("feat_wts", torch.from_numpy(wts))]
    return native().encode_predict_request("DCN", "serving_default", None, t, True, flt), ids, wts


def _outputs(resp: bytes):
    r = pb.PredictResponse.FromString(resp)
    return {k: T.to_ndarray(v) for k, v in r.outputs.items()}


def _check(out, rows):
    """sorted_index is the reference order of the returned prediction_node and
    sorted_prediction is prediction_node in that order, bit for bit."""
    got = out["prediction_node"]
    assert got.shape == (rows,)
    order = rc.ref_order(got)
    if "sorted_index" in out:
        assert out["sorted_index"].dtype == np.int64 and np.array_equal(out["sorted_index"], order)
    if "sorted_prediction" in out:
        assert np.array_equal(rc.bits(out["sorted_prediction"]), rc.bits(got[order]))


def test_ranked_requests_sharing_steps(servers):
    on, off = servers
    live, model = on.live, on.model
    assert live.ranks and type(live.srv).__module__.endswith("_hip")
    st0 = live.stats()
    filters = [ALL, [], ALL, ["sorted_index"], ALL, [], ["prediction_node", "sorted_prediction"], ALL, [], ALL, ALL, []]
    reqs = [_request([1, 512, 1500, 512, 1, 100, 1500, 512, 37, 1500, 512, 300][i], 40 + i, flt)
            for i, flt in enumerate(filters)]
    with cf.ThreadPoolExecutor(12) as pool:
        outs = list(pool.map(lambda r: live.predict_raw(r[0], 30.0), reqs))
    n_ranked = 0
    for flt, (data, ids, wts), (code, msg, resp) in zip(filters, reqs, outs):
        assert code == 0, msg  # CALLER_PATH for the ranked ones without the feature
        out = _outputs(resp)
        assert set(out) == set(flt or ["prediction_node"])
        want = model(torch.from_numpy(ids).cuda(), torch.from_numpy(wts).cuda()).float().cpu().numpy()
        if "prediction_node" in out:
            np.testing.assert_allclose(out["prediction_node"], want, atol=2e-5)  # as tests/test_live_gpu.py checks it
            _check(out, ids.shape[0])
        else:  # the index alone: a permutation that ranks the eager scores up to their 2e-5
            perm = out["sorted_index"]
            assert sorted(perm.tolist()) == list(range(ids.shape[0]))
            assert np.all(np.diff(want[perm]) >= -4e-5)
        n_ranked += any(k in flt for k in ALL[1:])
    st = live.stats()
    assert st["ranked"] - st0["ranked"] == n_ranked and not st["broken"]
    assert st["steps"] - st0["steps"] < len(reqs)


@pytest.mark.parametrize("rows", [1, 512, 1500])
def test_response_equals_the_general_path_of_a_server_without_the_flag(servers, rows):
    """The same bytes to both servers, one request per step on each (so both
    score the rows with the same kernels at the same place of the batch): every
    output the fast path encodes equals the general path's, dtype and bits."""
    on, off = servers
    data, ids, wts = _request(rows, 90 + rows, ALL)
    code, msg, resp = on.live.predict_raw(data, 30.0)
    assert code == 0, msg
    got = _outputs(resp)
    assert off.live.predict_raw(data, 30.0)[0] == off.live.CALLER_PATH
    ref = _outputs(off.service.predict_bytes(data, 30.0))
    assert set(ref) == set(got) == set(ALL)
    for k in ALL:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape == (rows,), k
        assert np.array_equal(got[k].view(np.uint32 if k != "sorted_index" else np.int64),
                              ref[k].view(np.uint32 if k != "sorted_index" else np.int64)), k
    _check(got, rows)
    assert off.live.stats()["ranked"] == 0


def test_plain_requests_and_the_service_entry(servers):
    on, off = servers
    data, ids, wts = _request(300, 77, [])
    a = _outputs(on.service.predict_bytes(data, 30.0))
    b = _outputs(off.service.predict_bytes(data, 30.0))
    assert list(a) == list(b) == ["prediction_node"]
    assert np.array_equal(rc.bits(a["prediction_node"]), rc.bits(b["prediction_node"]))
    before = on.live.stats()["ranked"]
    data, ids, wts = _request(1500, 78, ALL)
    _check(_outputs(on.service.predict_bytes(data, 30.0)), 1500)
    assert on.live.stats()["ranked"] == before + 1  # the service took the fast path
