"""The DIN attention kernels (csrc/kernels/din_attention.hip) are captured into
the served step: no scratch (tests/test_kernel_resources.py tells why), and the
resident weights plus the per-wave slices fit the CU's LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import HIPCC, _resources  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_din_kernels_are_scratch_free():
    res = _resources("din_attention.hip")
    assert len(res) == 8, sorted(res)  # 1 .. 4 history blocks x int32 / int64 ids
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"
        assert r.get("lds", 0) <= 160 * 1024, f"{name} needs {r.get('lds')} bytes of LDS"
