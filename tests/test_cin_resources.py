"""Compile-only checks of csrc/kernels/cin.hip: the accumulators of the whole
K loop stay in registers, and no instruction touches a register that one of
its inline-asm loads is still filling."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import HIPCC, REPO, _flags, _resources  # noqa: E402


def test_cin_kernels_fit_registers_and_lds():
    res = _resources("cin.hip")
    assert len(res) == 8, sorted(res)  # 1 .. 8 column blocks per pass
    for name, r in res.items():
        assert r.get("scratch") == 0, f"{name} spills {r.get('scratch')} bytes/lane to scratch"
        assert r["lds"] <= 160 * 1024, (name, r)


def test_cin_inline_asm_loads_have_no_register_hazards(tmp_path):
    sys.path.insert(0, REPO)
    from tools import isa_hazards

    path = os.path.join(REPO, "csrc", "kernels", "cin.hip")
    asm = str(tmp_path / "k.s")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", path,
                          "-o", asm, "-I" + os.path.join(REPO, "csrc"), *_flags(path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(asm) as f:
        kernels = isa_hazards.parse_kernels(f.read().splitlines())
    bad = {name: isa_hazards.check(instrs) for name, instrs in kernels.items()}
    bad = {k: v[:3] for k, v in bad.items() if v}
    assert any("cin_kernel" in k for k in kernels) and not bad, bad
