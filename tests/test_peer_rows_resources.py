"""Compile-time resources of the row-wise peer-lookup kernels (CPU: hipcc
cross-compiles for gfx950), as tests/test_peer_fp8_resources.py checks their
table-wise twins: scratch-free like every kernel captured into the served
step's HIP graph, the fused kernels with the 8192 bytes of LDS of their twins
(4 waves x one output row), the bag and fill kernels with none."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kr.HIPCC), reason="hipcc not installed")

FUSED = ("dot_interact_gather_peer_rows_kernel", "dot_interact_gather_peer_rows_fp8_kernel")
OTHERS = ("peer_bag_rows_kernel", "peer_bag_rows_fp8_kernel", "peer_cache_fill_rows_kernel")


@pytest.fixture(scope="module")
def res():
    return kr._resources("peer_lookup_rows.hip")


def test_row_kernels_are_scratch_free(res):
    names = " ".join(res)
    for k in FUSED + OTHERS:
        assert k in names, (k, list(res))
    assert len(res) == 10, list(res)  # fused and bag, bf16 and fp8: int32 and int64 ids; the fill: bf16 and fp8 rows
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"


def test_lds_matches_the_table_wise_twins(res):
    fused = {n: r for n, r in res.items() if "dot_interact_gather_peer_rows" in n}
    assert len(fused) == 4
    for name, r in fused.items():
        assert r["lds"] == 8192, (name, r)
    for name, r in res.items():
        if name not in fused:
            assert r["lds"] == 0, (name, r)
