"""Compile-time resources of the fp8 peer-lookup kernels (CPU: hipcc
cross-compiles for gfx950): scratch-free like every kernel captured into the
served step's HIP graph (tests/test_kernel_resources.py), and the fused
kernel's LDS is the 8192 bytes of its twins (4 waves x one output row)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kr.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def res():
    return kr._resources("peer_lookup_fp8.hip")


def test_peer_fp8_kernels_are_scratch_free(res):
    names = " ".join(res)
    for k in ("dot_interact_gather_peer_fp8_kernel", "peer_bag_fp8_kernel", "peer_cache_fill_fp8_kernel"):
        assert k in names, (k, list(res))
    assert len(res) == 5, list(res)  # fused and bag: int32 and int64 ids; one fill
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"


def test_fused_kernel_lds_matches_its_twins(res):
    fused = {n: r for n, r in res.items() if "dot_interact_gather_peer_fp8_kernel" in n}
    assert len(fused) == 2
    for name, r in fused.items():
        assert r["lds"] == 8192, (name, r)
    for src, key in (("interaction_fp8.hip", "dot_interact_gather_fp8_kernel"),
                     ("interaction.hip", "dot_interact_gather_kernel")):
        twins = {n: r for n, r in kr._resources(src).items() if key in n}
        assert twins and all(r["lds"] == 8192 for r in twins.values()), twins
    for name, r in res.items():
        if name not in fused:
            assert r["lds"] == 0, (name, r)
