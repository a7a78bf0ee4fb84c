"""The top-k kernels (csrc/kernels/topk.hip) and, since they share
rank_common.h with them, the rank kernels are captured into the served step:
none of them may use scratch (tests/test_kernel_resources.py tells why). The
same code-object resource query as there."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import HIPCC, _resources  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.mark.parametrize("src,kernels", [("topk.hip", 8), ("rank.hip", 6)])
def test_kernels_are_scratch_free(src, kernels):
    res = _resources(src)
    assert len(res) == kernels, sorted(res)
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{src}: {name} spills {r.get('scratch')} bytes/lane to scratch"
        assert r.get("lds", 0) <= 160 * 1024, f"{src}: {name} needs {r.get('lds')} bytes of LDS"
