"""Compile-only checks of csrc/kernels/autoint.hip: a candidate's whole stack
stays in registers (no scratch) and the resident weights fit the LDS."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import _resources  # noqa: E402


def test_autoint_kernels_fit_registers_and_lds():
    res = _resources("autoint.hip")
    assert len(res) == 12, sorted(res)  # 1 .. 4 row blocks x 1, 2, 4 heads
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"
        assert r["lds"] <= 160 * 1024, (name, r)
