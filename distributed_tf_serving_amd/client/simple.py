"""Smoke client (reference DCNClientSimple, DCNClientSimple.java:25-61).

Sends one Predict to host:port and prints the response. By default the request
is well-formed ([2, 43] with 86 ids/weights); ``--reference-shape`` reproduces
the reference exactly: shape [1500, 43] with only 87 ids and 86 weights, which
works only through TF's fill-with-last-value semantics (tensor.proto:24-29).
``--top-k N`` asks for the N best candidates (``top_prediction`` /
``top_index``, input ``top_k``) beside the scores and prints them.
"""
from __future__ import annotations

import argparse

from ..wire import schema as pb
from ..wire.tensor import make_shape
from .backends import GrpcBackend


def build_request(reference_shape: bool = False, fields: int = 43, model: str = "DCN",
                  signature: str = "serving_default", top_k: int = 0):
    r = pb.PredictRequest()
    r.model_spec.name = model
    r.model_spec.signature_name = signature
    rows = 1500 if reference_shape else 2
    for key, dt in (("feat_ids", pb.DT_INT64), ("feat_wts", pb.DT_FLOAT)):
        t = r.inputs[key]
        t.dtype = dt
        t.tensor_shape.CopyFrom(make_shape([rows, fields]))
    r.inputs["feat_ids"].int64_val.extend(list(range(1, fields + 1)) +
                                          list(range(fields, 2 * fields + (1 if reference_shape else 0))))
    r.inputs["feat_wts"].float_val.extend([1.0] * (2 * fields))
    if top_k > 0:
        r.inputs["top_k"].dtype = pb.DT_INT64
        r.inputs["top_k"].tensor_shape.CopyFrom(make_shape([]))
        r.inputs["top_k"].int64_val.append(int(top_k))
        r.output_filter.extend(["prediction_node", "top_prediction", "top_index"])
    return r


def top_entries(resp):
    """[(candidate index, score)] of a response's top-k outputs, best first."""
    return list(zip(resp.outputs["top_index"].int64_val, resp.outputs["top_prediction"].float_val))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=9999)
    ap.add_argument("--reference-shape", action="store_true")
    ap.add_argument("--top-k", type=int, default=0, help="also ask for the N best candidates and print them")
    a = ap.parse_args(argv)
    be = GrpcBackend(f"{a.host}:{a.port}")
    try:
        req = build_request(a.reference_shape, top_k=a.top_k)
        resp = pb.PredictResponse.FromString(be.predict(req.SerializeToString(), 30))
        print(resp)
        for rank, (idx, score) in enumerate(top_entries(resp) if a.top_k > 0 else ()):
            print(f"top {rank + 1}: candidate {idx} score {score:.6f}")
    finally:
        be.close()  # the reference never closes its channel (DCNClientSimple.java:54-60)


if __name__ == "__main__":
    main()
