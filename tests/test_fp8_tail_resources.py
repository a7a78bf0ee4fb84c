"""Compile-time resources of the MX-fp8 fused MLP tail (CPU: hipcc
cross-compiles for gfx950): scratch-free, like the other kernels captured into
the served step's HIP graph (tests/test_kernel_resources.py), inside the CU's
160 KiB of LDS, two waves per SIMD (512 threads on 4 SIMDs), and built on the
block-scaled 16x16x128 MFMA."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kr.HIPCC), reason="hipcc not installed")

SRC = "mlp_tail_fp8.hip"


def test_fp8_tail_is_scratch_free_and_fits_lds():
    res = kr._resources(SRC)
    assert len(res) == 1, res
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"
        assert 0 < r["lds"] <= 160 * 1024, (name, r)
        assert r["vgprs"] + r["agprs"] <= 256, (name, r)  # 8 waves per CU


def test_fp8_tail_isa(tmp_path):
    """The MFMA is the block-scaled one, and no instruction touches a register
    an inline-asm load is still filling (tools/isa_hazards.py)."""
    sys.path.insert(0, kr.REPO)
    from tools import isa_hazards

    path = os.path.join(kr.REPO, "csrc", "kernels", SRC)
    asm = str(tmp_path / "k.s")
    out = subprocess.run([kr.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", path,
                          "-o", asm, "-I" + os.path.join(kr.REPO, "csrc"), *kr._flags(path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(asm) as f:
        text = f.read()
    # both K loops are fully unrolled: GEMM2 8 tiles x 16, GEMM3 4 tiles x 8
    assert text.count("v_mfma_scale_f32_16x16x128_f8f6f4") == 8 * 16 + 4 * 8
    assert "v_mfma_f32_16x16x32" not in text
    kernels = isa_hazards.parse_kernels(text.splitlines())
    assert kernels
    bad = {name: isa_hazards.check(instrs)[:3] for name, instrs in kernels.items() if isa_hazards.check(instrs)}
    assert not bad, bad
