"""Exact small-integer cases for the MX-fp8 fused MLP tail (ops.mlp_tail_fp8,
csrc/kernels/mlp_tail_fp8.hip), in the manner of tests/exact_cases.py: seeded
generators that return CPU tensors plus a float64 reference written from the
op's contract with plain torch - nothing here imports distributed_tf_serving_amd -
and assert the conditions under which every step of the op is exact.

Contract (x bf16 [M, 1024], W2q e4m3 [512, 1024], W3q e4m3 [256, 512]):

    (xq, ex)  = MX(x)   per (row, 32 columns): e = smallest integer with
                        amax / 2^e <= 448 (0 for a zero block, clamped to
                        [-127, 127]), q = e4m3(x 2^-e), scale byte e + 127
    h2        = act2((xq 2^ex) W2q^T * sw2 + b2)
    (h2q, e2) = MX(h2)
    h3        = act3((h2q 2^e2) W3q^T * sw3 + b3)
    y         = h3 . hw + hbias + sum_e extra[e, :M]        (sigmoid off)

Family B (K / N indexing): x in {-1, 0, 1} with columns 32..63 zero (an
all-zero block in every row), W2q 12 entries of +-1 per row, sw2 in {1, 2},
b2 = sw2 * {-2..2}: |h2| <= 28 and every h2 is an integer of at most 4
significant bits, which e4m3 holds under any block scale. W3q 16 entries of
magnitude 1..3 per row, sw3 in {0.5, 1, 2}, integer b3 / hw, hbias 1.5, extra
[2, M + 37] integers.

Family A (x scale placement): x = {-1, 0, 1} 2^s with s in {0..3} drawn per
(row, block), so neighbouring blocks carry different scale bytes; W2q 2
entries of +-1 per row, sw2 = 1, b2 = 0: h2 = +-2^a +- 2^b spans <= 4 bits.
The rest as in family B.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

K1, N2, N3 = 1024, 512, 256
MX_BLOCK = 32
E4M3_MAX = 448.0
F32_EXACT = 1 << 24
EXTRA_PAD = 37

ROWS = (1, 63, 64, 65, 130)
ACT_PAIRS = (("relu", "relu"), ("none", "none"), ("relu", "none"))
CASES = [(fam, M) + ACT_PAIRS[(i + (fam == "A")) % 3] for fam in ("B", "A") for i, M in enumerate(ROWS)]


def _gen(*key) -> torch.Generator:
    seed = 0x51ED27
    for k in key:
        seed = (seed * 1000003 + int(k) + 977) % ((1 << 61) - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _sparse(g, n, k, nnz, mag):
    """float64 [n, k]: exactly nnz entries per row, magnitudes 1..mag, random signs."""
    pos = torch.rand(n, k, generator=g).topk(nnz, dim=1).indices
    val = torch.randint(1, mag + 1, (n, nnz), generator=g).double() * (torch.randint(0, 2, (n, nnz), generator=g) * 2 - 1)
    return torch.zeros(n, k, dtype=torch.float64).scatter_(1, pos, val)


def _act(x, act):
    assert act in ("none", "relu")
    return torch.relu(x) if act == "relu" else x


def mx_quant(x: torch.Tensor):
    """float64 [M, K] -> (e4m3 values as float64 [M, K], exponents int64 [M, K / 32])."""
    M, K = x.shape
    blk = x.view(M, K // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(dim=2)
    m, ex = torch.frexp(amax / E4M3_MAX)  # amax / 448 = m 2^ex, m in [0.5, 1)
    e = torch.where(m == 0.5, ex - 1, ex)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127).long()
    q = (blk * torch.exp2(-e.double())[:, :, None]).clamp(-E4M3_MAX, E4M3_MAX)
    q = q.to(torch.float32).to(torch.float8_e4m3fn).to(torch.float64)
    return q.view(M, K), e


def mx_dequant(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    return q * torch.exp2(e.double()).repeat_interleave(MX_BLOCK, dim=1)


def tail_ref(c, swap_x=None, shift_x_scale=False, swap_h2=None, shift_sw2=False, drop_k_tile=None,
             parts: bool = False):
    """float64 y [M] of the contract. The keyword arguments inject one fault each
    (tests/test_fp8_tail_cpu.py): e4m3 codes of two x columns swapped with the
    scales left in place, every x scale byte taken from the next block of its
    row, two h2 codes swapped, sw2 read one channel off, one 128-deep K tile
    of GEMM2 dropped."""
    xq, ex = mx_quant(c.x.double())
    if swap_x is not None:
        a, b = swap_x
        xq = xq.clone()
        xq[:, [a, b]] = xq[:, [b, a]]
    if shift_x_scale:
        ex = torch.roll(ex, -1, dims=1)
    xd = mx_dequant(xq, ex)
    if drop_k_tile is not None:
        xd = xd.clone()
        xd[:, 128 * drop_k_tile:128 * drop_k_tile + 128] = 0
    sw2 = torch.roll(c.sw2, 1) if shift_sw2 else c.sw2
    h2 = _act(xd @ c.W2q.double().t() * sw2.double() + c.b2.double(), c.act2)
    h2q, e2 = mx_quant(h2)
    if swap_h2 is not None:
        a, b = swap_h2
        h2q = h2q.clone()
        h2q[:, [a, b]] = h2q[:, [b, a]]
    h2d = mx_dequant(h2q, e2)
    h3 = _act(h2d @ c.W3q.double().t() * c.sw3.double() + c.b3.double(), c.act3)
    M = c.x.shape[0]
    y = h3 @ c.hw.double() + c.hbias + c.extra[:, :M].double().sum(0)
    if parts:
        return SimpleNamespace(y=y, xd=xd, ex=ex, h2=h2, h2d=h2d, e2=e2, h3=h3)
    return y


def f32(t: torch.Tensor) -> torch.Tensor:
    """float64 reference -> fp32, which must hold it exactly."""
    o = t.to(torch.float32)
    assert torch.equal(o.double(), t.double()), "reference is not an fp32 value"
    return o


def _e4m3(t: torch.Tensor) -> torch.Tensor:
    o = t.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(o.to(torch.float64), t.double()), "weight is not an e4m3 value"
    return o


def _bf16(t: torch.Tensor) -> torch.Tensor:
    o = t.to(torch.bfloat16)
    assert torch.equal(o.double(), t.double()), "x is not a bf16 value"
    return o


@functools.lru_cache(maxsize=None)
def tail_case(family: str, M: int, act2: str, act3: str):
    """One exact case: inputs as the op takes them (CPU), ``ref`` fp32 [M]."""
    assert family in ("A", "B")
    g = _gen(ord(family), M, len(act2), len(act3))
    if family == "B":
        x = _ints(g, -1, 1, (M, K1))
        x[:, 32:64] = 0
        W2 = _sparse(g, N2, K1, 12, 1)
        sw2 = _ints(g, 1, 2, (N2,))
        b2 = sw2 * _ints(g, -2, 2, (N2,))
    else:
        s = torch.randint(0, 4, (M, K1 // MX_BLOCK), generator=g).double()
        x = _ints(g, -1, 1, (M, K1)) * torch.exp2(s).repeat_interleave(MX_BLOCK, dim=1)
        W2 = _sparse(g, N2, K1, 2, 1)
        sw2 = torch.ones(N2, dtype=torch.float64)
        b2 = torch.zeros(N2, dtype=torch.float64)
    W3 = _sparse(g, N3, N2, 16, 3)
    sw3 = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (N3,), generator=g)]
    b3 = _ints(g, -3, 3, (N3,))
    hw = _ints(g, -3, 3, (N3,))
    extra = _ints(g, -4, 4, (2, M + EXTRA_PAD))
    c = SimpleNamespace(family=family, M=M, act2=act2, act3=act3, x=_bf16(x), W2q=_e4m3(W2), sw2=f32(sw2),
                        b2=f32(b2), W3q=_e4m3(W3), sw3=f32(sw3), b3=f32(b3), hw=f32(hw), hbias=1.5,
                        extra=f32(extra))
    r = tail_ref(c, parts=True)
    # exactness conditions (conditions on the inputs, not tolerances)
    assert torch.equal(r.xd, x), "the MX round trip of x is not the identity"
    assert torch.equal(r.h2d, r.h2), "the MX round trip of h2 is not the identity"
    # family A's h2 is sparse (2 weights per channel): one row's 16 blocks can share an exponent
    assert r.e2.unique().numel() >= (3 if family == "B" or M > 1 else 1), \
        f"only {r.e2.unique().tolist()} as h2 block exponents"
    if family == "A":
        assert r.ex.unique().numel() >= 4 and bool((r.ex[:, 1:] != r.ex[:, :-1]).any()), "x block scales do not vary"
    else:
        assert bool((r.ex[:, 1] == 0).all()) and r.h2.abs().max() <= 28
    # every partial sum, in any order, is a multiple of 0.5 below 2^24 units:
    # GEMM2 / GEMM3 accumulate before the channel scale, the head after it
    assert (x.abs() @ W2.abs().t()).max() < F32_EXACT
    assert (r.h2.abs() @ W3.abs().t()).max() < F32_EXACT
    h3_abs = (r.h2.abs() @ W3.abs().t()) * sw3 + b3.abs()
    tot = h3_abs @ hw.abs() + 1.5 + extra[:, :M].abs().sum(0)
    assert (tot / 0.5).max() < F32_EXACT, "head partial sums reach 2^24 units of 0.5"
    assert bool(((r.h3 * 2) == (r.h3 * 2).round()).all())
    c.ref = f32(r.y)
    c.h2 = r.h2
    return c
