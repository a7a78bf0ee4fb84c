"""Small-integer cases on which the MFMA kernels' arithmetic is exact, with
references that share no code with distributed_tf_serving_amd.ops.

Products and sums of small integers are exact in bf16 x bf16 -> fp32 MFMA
accumulation, integers of magnitude <= 256 survive rounding to bf16, and
power-of-two scales are exact in fp8 / MX. A single misplaced element, a
dropped K step or a stale ring slot then changes an integer, whatever order
the kernel accumulates in, and a torch.equal comparison sees it.

Every generator is seeded, returns CPU tensors plus a float64 / int64
reference computed with plain torch ops, and asserts the conditions under
which the kernel is exact (they are conditions on the inputs, not tolerances).
The parameter lists of tests/test_kernels_exact_gpu.py and
tests/test_gather_exact_gpu.py live here so that tests/test_exact_cases_cpu.py
checks the same cases without a GPU.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

BF16_EXACT = 256  # integers of magnitude <= 2^8 are bf16 values
F32_EXACT = 1 << 24  # integers of magnitude <= 2^24 are fp32 values
EDGE_IDS = (-(1 << 63), (1 << 63) - 1, -1, 0)


# ------------------------------------------------------------------ helpers
def _gen(*key) -> torch.Generator:
    seed = 0x9E3779B1
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % ((1 << 61) - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, shape, dtype=torch.float32):
    """Uniform integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def sparse_pm1(g, n, k, nnz) -> torch.Tensor:
    """fp32 [n, k] with exactly min(nnz, k) entries of +-1 per row at random positions."""
    nnz = min(nnz, k)
    pos = torch.rand(n, k, generator=g).topk(nnz, dim=1).indices
    sign = torch.randint(0, 2, (n, nnz), generator=g).float() * 2 - 1
    return torch.zeros(n, k).scatter_(1, pos, sign)


def py_mod_rows(ids: torch.Tensor, modulo: int, V: int) -> torch.Tensor:
    """clamp(python_mod(id, modulo), 0, V - 1) on Python integers."""
    flat = [min(max(int(i) % modulo, 0), V - 1) for i in ids.reshape(-1).tolist()]
    return torch.tensor(flat, dtype=torch.int64).view(ids.shape)


def _act(x, act):
    assert act in ("none", "relu")
    return torch.relu(x) if act == "relu" else x


def _is_int(t) -> bool:
    return bool((t == t.round()).all())


def _check_bf16_ints(t, what):
    m = t.abs().max().item() if t.numel() else 0
    assert _is_int(t) and m <= BF16_EXACT, f"{what}: max |value| {m} is not a bf16-exact integer"


def _check_f32_sum(abs_sum, what, unit=1.0):
    """Every partial sum, in any order, is a multiple of ``unit`` below 2^24 units."""
    m = float(abs_sum.max()) / unit if abs_sum.numel() else 0
    assert m < F32_EXACT, f"{what}: sum of magnitudes {m} units reaches 2^24"


def f32(t: torch.Tensor) -> torch.Tensor:
    """float64 reference -> fp32, which must hold it exactly."""
    o = t.to(torch.float32)
    assert torch.equal(o.double(), t.double()), "reference is not an fp32 value"
    return o


def bf16(t: torch.Tensor) -> torch.Tensor:
    o = t.to(torch.bfloat16)
    assert torch.equal(o.double(), t.double()), "reference is not a bf16 value"
    return o


# ------------------------------------------------------------------ gather inputs
def gather_inputs(B, F, V, modulo, seed, ids=None, wts=None, D=64):
    """Table {-2..2} bf16 [V, D], lin {-3..3}, weights {0, 1, 2} (the zeros
    matter: padding rows and zero-weight fields stay in), int64 ids over the
    whole range including -2^63, 2^63 - 1, -1 and 0."""
    g = _gen(1, B, F, V, seed) if D == 64 else _gen(1, B, F, V, seed, D)
    table = _ints(g, -2, 2, (V, D), torch.bfloat16)
    lin = _ints(g, -3, 3, (V,))
    if wts is None:
        wts = _ints(g, 0, 2, (B, F))
    if ids is None:
        ids = torch.randint(-(1 << 62), 1 << 62, (B, F), generator=g)
        edge = torch.tensor(EDGE_IDS, dtype=torch.int64)
        n = min(4, B * F)
        ids.view(-1)[-n:] = edge[:n]
        if B * F >= 8:  # and at the front, on non-zero weights
            ids.view(-1)[:4] = edge
            wts.view(-1)[:4] = torch.tensor([1.0, 2.0, 1.0, 2.0])
    rows = py_mod_rows(ids, modulo, V)
    return SimpleNamespace(B=B, F=F, V=V, modulo=modulo, table=table, lin=lin, ids=ids, wts=wts, rows=rows)


def embed_ref(c):
    """float64: e [B, F, D] = T[row] * w and the first-order sum."""
    e = c.table[c.rows].double() * c.wts.double()[..., None]
    first = (c.lin[c.rows].double() * c.wts.double()).sum(1)
    return e, first


def fm_term(e):
    return 0.5 * (e.sum(1).pow(2) - e.pow(2).sum(1)).sum(1)


def _check_gather(c, e, first):
    _check_bf16_ints(e, "x = T[row] * w")
    _check_f32_sum((c.lin[c.rows].abs() * c.wts).sum(1), "first-order term")
    s_abs = e.abs().sum(1)
    _check_f32_sum((s_abs.pow(2) + e.pow(2).sum(1)).sum(1), "FM term")


# ------------------------------------------------------------------ tower
TOWER_ACTS = [(True, "relu", "relu"), (False, "none", "none"), (False, "relu", "none")]
TOWER_B = [1, 63, 64, 65, 200]
TOWER_F = [1, 3, 4, 5, 43, 64]
TOWER_V = 5000
TOWER_MODULI = [TOWER_V, 1, 4096, (1 << 32) - 1, (1 << 32) + 3]
# Non-zeros per output row. h1 / h2 are stored as bf16, so both must stay <= 256
# (tower_ref asserts it): with 64 / 8 the cases below reach max |h1| = 106 and
# max |h2| = 236; 128 / 6 overflowed h2 (267), 128 / 4 left a swap of two h1
# columns visible in only 23 % of the rows of one case (each h1 column then
# feeds two h2 columns on average; with 8 it feeds four).
W1_NNZ, W2_NNZ, W3_NNZ = 64, 8, 16

# every B x F, the activation pattern cycling so each meets every B and every F
TOWER_CASES = [(B, F, TOWER_V) + TOWER_ACTS[(i + j) % 3] + (TOWER_V,)
               for i, B in enumerate(TOWER_B) for j, F in enumerate(TOWER_F)]
# every modulus with both kernels (fm on / off), one partial and one full workgroup
TOWER_MODULO_CASES = [(B, 43, TOWER_V) + TOWER_ACTS[k % 3] + (m,)
                      for k, m in enumerate(TOWER_MODULI) for B in (65,)] + \
                     [(200, 5, TOWER_V) + TOWER_ACTS[(k + 1) % 3] + (m,) for k, m in enumerate(TOWER_MODULI[1:])]
# the input forms (int32 rows, strided narrow rows, arena rows) run at these
TOWER_FORM_CASES = [(200, 43, TOWER_V) + TOWER_ACTS[0] + (TOWER_V,), (65, 4, TOWER_V) + TOWER_ACTS[2] + (TOWER_V,)]


@functools.lru_cache(maxsize=None)
def tower_weights(F, N1=1024, seed=0):
    """W1 / W2 / W3 with entries in {-1, 0, 1} (a fixed number of non-zeros per
    output row), small integer biases and head weights; half-integer scalars."""
    g = _gen(2, F, N1, seed)
    return SimpleNamespace(
        W1=sparse_pm1(g, N1, 64 * F, W1_NNZ), b1=_ints(g, -2, 2, (N1,)),
        W2=sparse_pm1(g, 512, 1024, W2_NNZ), b2=_ints(g, -2, 2, (512,)),
        W3=sparse_pm1(g, 256, 512, W3_NNZ), b3=_ints(g, -2, 2, (256,)),
        hw=_ints(g, -2, 2, (256,)), hbias=2.5, bias=-1.5)


def tower_ref(c, w, fm, act2, act3, e_hook=None, x_hook=None, h1_hook=None, check=True):
    """The tower of csrc/kernels/gather_mlp.hip's header comment in float64,
    sigmoid off. ``e_hook`` edits the gathered rows (MLP input and FM term, not
    the first-order term), ``x_hook`` the MLP input alone, ``h1_hook`` h1: the
    CPU tests' mutants. Returns h1, h2, h3, first, fm, logit."""
    e, first = embed_ref(c)
    if e_hook is not None:
        e = e_hook(e)
    x = e if x_hook is None else x_hook(e.clone())
    h1 = torch.relu(x.reshape(c.B, -1) @ w.W1.double().t() + w.b1.double())
    if h1_hook is not None:
        h1 = h1_hook(h1)
    h2 = _act(h1 @ w.W2.double().t() + w.b2.double(), act2)
    h3 = _act(h2 @ w.W3.double().t() + w.b3.double(), act3)
    fmv = fm_term(e) if fm else torch.zeros(c.B, dtype=torch.float64)
    logit = h3 @ w.hw.double() + w.hbias + w.bias + first + fmv
    if check:
        _check_gather(c, e, first)
        # stored as bf16 by the kernel: below 2^8 that rounding is the identity
        _check_bf16_ints(h1, "h1")
        _check_bf16_ints(h2, "h2")
        xa = x.abs().reshape(c.B, -1)
        _check_f32_sum(xa @ w.W1.abs().double().t() + w.b1.abs().double(), "h1 sums")
        _check_f32_sum(h1.abs() @ w.W2.abs().double().t() + w.b2.abs().double(), "h2 sums")
        h3a = h2.abs() @ w.W3.abs().double().t() + w.b3.abs().double()
        _check_f32_sum(h3a, "h3 sums")
        # the scalars are half-integers: every partial sum in units of 0.5
        total = h3a @ w.hw.abs().double() + abs(w.hbias) + abs(w.bias) + first.abs() + fmv.abs()
        _check_f32_sum(total, "logit", unit=0.5)
    return SimpleNamespace(h1=h1, h2=h2, h3=h3, first=first, fm=fmv, logit=logit)


def tower_case(B, F, V, fm, act2, act3, modulo, seed=0, ids=None, wts=None):
    c = gather_inputs(B, F, V, modulo, seed, ids=ids, wts=wts)
    w = tower_weights(F)
    r = tower_ref(c, w, fm, act2, act3)
    return c, w, r


# ------------------------------------------------------------------ gather-GEMM
GATHER_GEMM_B = [1, 255, 257, 600]
GATHER_GEMM_F = [1, 5, 7, 43]
GATHER_GEMM_NFM = [(1024, True), (1024, False), (512, False)]
GATHER_GEMM_V = 5000
GATHER_GEMM_CASES = [(B, F) + GATHER_GEMM_NFM[(i + j) % 3]
                     for i, B in enumerate(GATHER_GEMM_B) for j, F in enumerate(GATHER_GEMM_F)]


def gather_gemm_case(B, F, N, fm2, V=GATHER_GEMM_V, seed=0):
    """ops.embed_gemm: h = relu(x W^T + b) as bf16, parts[0] = bias + the
    first-order term, parts[1] = the FM term."""
    c = gather_inputs(B, F, V, V, seed + 7)
    w = tower_weights(F, N1=N, seed=1)
    e, first = embed_ref(c)
    _check_gather(c, e, first)
    h = torch.relu(e.reshape(B, -1) @ w.W1.double().t() + w.b1.double())
    _check_bf16_ints(h, "h")
    _check_f32_sum(e.abs().reshape(B, -1) @ w.W1.abs().double().t() + w.b1.abs().double(), "h sums")
    r = SimpleNamespace(h=h, part0=first + w.bias, part1=fm_term(e) if fm2 else None)
    return c, w, r


# ------------------------------------------------------------------ dense GEMMs
GEMM_VARIANTS = [0, 4, 8, 10, 14, 17, 18]
GEMM_SHAPES = [(1, 64, 64), (300, 200, 128), (513, 1024, 192), (130, 1020, 256)]  # N = 1020: register epilogue
GEMM_EPI_OUT = [("none", False), ("relu", False), ("none", True), ("relu", True)]  # (epilogue, bf16 output)
GEMM_NNZ = 64


def gemm_case(M, N, K, out_bf16, act="none", seed=0):
    """Integer A {-2..2}, sparse +-1 W, integer bias: sum |a||w| + |b| <= 256,
    so the bf16 output is exact too."""
    g = _gen(3, M, N, K, seed)
    A = _ints(g, -2, 2, (M, K), torch.bfloat16)
    W = sparse_pm1(g, N, K, GEMM_NNZ)
    b = _ints(g, -4, 4, (N,))
    bound = A.double().abs() @ W.double().abs().t() + b.double().abs()
    assert bound.max().item() <= BF16_EXACT
    y = _act(A.double() @ W.double().t() + b.double(), act)
    return SimpleNamespace(A=A, W=W.to(torch.bfloat16), b=b, y=bf16(y) if out_bf16 else f32(y))


MLP_M = [1, 130]
LINEAR_HEAD_NK = [(256, 512), (40, 64)]


def mlp_tail_case(M, act2, act3, seed=0):
    """ops.mlp_tail: 1024 -> 512 -> 256 -> score with [2, M + pad] partial logits."""
    g = _gen(4, M, seed)
    x = _ints(g, -2, 2, (M, 1024), torch.bfloat16)
    W2, b2 = sparse_pm1(g, 512, 1024, 32), _ints(g, -2, 2, (512,))
    W3, b3 = sparse_pm1(g, 256, 512, W3_NNZ), _ints(g, -2, 2, (256,))
    hw, hbias = _ints(g, -2, 2, (256,)), 1.5
    extra = _ints(g, -50, 50, (2, M + 37))
    h2 = _act(x.double() @ W2.double().t() + b2.double(), act2)
    _check_bf16_ints(h2, "h2")
    h3 = _act(h2 @ W3.double().t() + b3.double(), act3)
    h3a = h2.abs() @ W3.abs().double().t() + b3.abs().double()
    _check_f32_sum(h3a @ hw.abs().double() + hbias + extra[:, :M].abs().sum(0).double(), "logit", unit=0.5)
    y = h3 @ hw.double() + hbias + extra[:, :M].double().sum(0)
    return SimpleNamespace(x=x, W2=W2.to(torch.bfloat16), b2=b2, W3=W3.to(torch.bfloat16), b3=b3, hw=hw, hbias=hbias,
                           extra=extra, y=f32(y))


def linear_head_case(M, N, K, act, seed=0):
    """ops.linear_head: act(x W^T + b) . hw + hbias + extra, h kept in fp32."""
    g = _gen(5, M, N, K, seed)
    x = _ints(g, -2, 2, (M, K), torch.bfloat16)
    W, b = sparse_pm1(g, N, K, GEMM_NNZ), _ints(g, -4, 4, (N,))
    hw, hbias = _ints(g, -3, 3, (N,)), -0.5
    extra = _ints(g, -50, 50, (M,))
    ha = x.double().abs() @ W.abs().double().t() + b.abs().double()
    _check_f32_sum(ha @ hw.abs().double() + abs(hbias) + extra.abs().double(), "logit", unit=0.5)
    h = _act(x.double() @ W.double().t() + b.double(), act)
    y = h @ hw.double() + hbias + extra.double()
    return SimpleNamespace(x=x, W=W.to(torch.bfloat16), b=b, hw=hw, hbias=hbias, extra=extra, y=f32(y))


BOTTOM_MLP3_DIMS = (512, 256, 64)
BOTTOM_MLP3_NNZ = (16, 8, 4)


def bottom_mlp3_case(M, nd, seed=0):
    """ops.bottom_mlp3: fp32 feature columns [:nd] -> bf16, zero padded to 64,
    three ReLU layers, every activation stored as bf16. ``full`` is wider than
    nd: the op reads a row view."""
    g = _gen(6, M, nd, seed)
    full = _ints(g, -2, 2, (M, nd + 9))
    x = torch.zeros(M, 64, dtype=torch.float64)
    x[:, :nd] = full[:, :nd].double()
    layers, k = [], 64
    for n, nnz in zip(BOTTOM_MLP3_DIMS, BOTTOM_MLP3_NNZ):
        W, b = sparse_pm1(g, n, k, nnz), _ints(g, -2, 2, (n,))
        x = torch.relu(x @ W.double().t() + b.double())
        _check_bf16_ints(x, f"bottom MLP layer {n}")
        layers.append((W.to(torch.bfloat16), b))
        k = n
    return SimpleNamespace(full=full, nd=nd, layers=layers, y=bf16(x))


# ------------------------------------------------------------------ fp8 / MX
FP8_SHAPES = [(37, 256, 512), (130, 264, 256)]
FP8_VARIANT_SHAPE = (256, 256, 128)
MX_SHAPE = (100, 256, 512)
MX_MAX_K = 3072
CROSS_FP8_SHAPES = [(130, 264), (256, 512)]
CROSS_TILE = 256


def _pow2(g, lo, hi, shape):
    """2^randint(lo, hi)."""
    return torch.exp2(torch.randint(lo, hi, shape, generator=g).float())


def fp8_ref(q, sx, Wq, sw, b, act, sx_blk=None):
    """float64: act((q * block scales) Wq^T * sx * sw + b)."""
    a = q.double()
    if sx_blk is not None:
        a = a * torch.exp2(sx_blk.double() - 127).repeat_interleave(32, dim=1)
    y = a @ Wq.double().t()
    if sx is not None:
        y = y * sx.double()[:, None]
    return _act(y * sw.double()[None, :] + b.double(), act)


def fp8_case(M, N, K, act="none", mx=False, seed=0):
    """e4m3 integers in [-8, 8] for A and W, built directly (no quantiser);
    per-row scales 2^randint(-3, 4). ``mx``: an E8M0 exponent byte per (row,
    32-block) instead of the row scale, drawn independently per row AND per
    block from 127 + randint(-4, 5)."""
    g = _gen(7, M, N, K, int(mx), seed)
    q = _ints(g, -8, 8, (M, K))
    Wq = _ints(g, -8, 8, (N, K))
    sw = _pow2(g, -3, 4, (N,))
    b = _ints(g, -8, 8, (N,))
    sx = sx_blk = None
    if mx:
        assert K % 128 == 0 and K <= MX_MAX_K
        sx_blk = (127 + torch.randint(-4, 5, (M, K // 32), generator=g)).to(torch.uint8)
        blk = torch.exp2(sx_blk.double() - 127)
        unit = blk.min(dim=1).values[:, None] * sw.double()[None, :]
        mag = (q.abs().double() * blk.repeat_interleave(32, dim=1)) @ Wq.abs().double().t() * sw.double()[None, :]
    else:
        sx = _pow2(g, -3, 4, (M,))
        unit = sx.double()[:, None] * sw.double()[None, :]
        mag = q.abs().double() @ Wq.abs().double().t() * unit
    # every partial sum is a multiple of min(unit, 1) and stays below 2^24 of them
    unit = unit.clamp(max=1.0)
    _check_f32_sum((mag + b.abs().double()) / unit, "fp8 GEMM")
    y = f32(fp8_ref(q, sx, Wq, sw, b, act, sx_blk))
    e4 = torch.float8_e4m3fn
    assert torch.equal(q.to(e4).float(), q) and torch.equal(Wq.to(e4).float(), Wq)
    return SimpleNamespace(q=q.to(e4), sx=sx, sx_blk=sx_blk, Wq=Wq.to(e4), sw=sw, b=b, y=y, act=act)


def cross_fp8_case(M, N, seed=0):
    """ops.cross_gemm_fp8: y = bf16(q Wq^T sx sw + b), z = bf16(x0 y + xl), and
    the per-256-column partial dots z . head_w. q has 4 entries of +-1 per row
    and the scales are in {1, 2}, so |y| <= 4 * 8 * 4 + 4 and z is an integer
    of magnitude <= 256."""
    g = _gen(8, M, N, seed)
    K = -(-N // 128) * 128
    q = torch.zeros(M, K)
    q[:, :N] = sparse_pm1(g, M, N, 4)
    Wq = torch.zeros(N, K)
    Wq[:, :N] = _ints(g, -8, 8, (N, N))
    sx, sw = _pow2(g, 0, 2, (M,)), _pow2(g, 0, 2, (N,))
    b = _ints(g, -4, 4, (N,))
    x0, xl = _ints(g, -1, 1, (M, N)), _ints(g, -2, 2, (M, N))
    hw = _ints(g, -2, 2, (N,))
    y = fp8_ref(q, sx, Wq, sw, b, "none")
    _check_bf16_ints(y, "cross y")
    z = x0.double() * y + xl.double()
    _check_bf16_ints(z, "cross z")
    d = torch.stack([z[:, t:t + CROSS_TILE] @ hw[t:t + CROSS_TILE].double() for t in range(0, N, CROSS_TILE)])
    e4 = torch.float8_e4m3fn
    return SimpleNamespace(q=q.to(e4), sx=sx, Wq=Wq.to(e4), sw=sw, b=b, x0=x0.to(torch.bfloat16),
                           xl=xl.to(torch.bfloat16), hw=hw, z=bf16(z), d=f32(d))


# ------------------------------------------------------------------ interaction
INTERACTION_T = [1, 26, 31]
INTERACTION_B = 23


def interaction_ref(dense, emb):
    """[dense | strictly lower triangle of X X^T, row-major | zero pad to a
    multiple of 64], X = [dense; emb]."""
    B, T = emb.shape[0], emb.shape[1]
    X = torch.cat([dense.double()[:, None], emb.double()], dim=1)
    Z = X @ X.transpose(1, 2)
    pairs = [(i, j) for i in range(T + 1) for j in range(i)]
    cols = (64 + len(pairs) + 63) // 64 * 64
    out = torch.zeros(B, cols, dtype=torch.float64)
    out[:, :64] = dense.double()
    for n, (i, j) in enumerate(pairs):
        out[:, 64 + n] = Z[:, i, j]
    _check_bf16_ints(out, "interaction")
    return bf16(out)


def interaction_case(T, B=INTERACTION_B, seed=0):
    """Dense and embedding vectors in {-2..2}: every 64-long dot is <= 256."""
    g = _gen(9, T, B, seed)
    dense = _ints(g, -2, 2, (B, 64), torch.bfloat16)
    emb = _ints(g, -2, 2, (B, T, 64), torch.bfloat16)
    return SimpleNamespace(dense=dense, emb=emb, z=interaction_ref(dense, emb))


def interaction_gather_case(T, B=INTERACTION_B, rows=300, seed=0):
    """The same through per-table rows: row = offset_f + python_mod(id, modulo_f)."""
    g = _gen(10, T, B, seed)
    dense = _ints(g, -2, 2, (B, 64), torch.bfloat16)
    table = _ints(g, -2, 2, (T * rows, 64), torch.bfloat16)
    ids = torch.randint(-(1 << 62), 1 << 62, (B, T), generator=g)
    n = min(4, B * T)
    ids.view(-1)[:n] = torch.tensor(EDGE_IDS[:n], dtype=torch.int64)
    mod = torch.full((T,), rows, dtype=torch.int64)
    off = torch.arange(T, dtype=torch.int64) * rows
    r = py_mod_rows(ids, rows, rows) + off[None, :]
    return SimpleNamespace(dense=dense, table=table, ids=ids, mod=mod, off=off, z=interaction_ref(dense, table[r]))


# ------------------------------------------------------------------ address range
RANGE_V = 1 << 25
RANGE_ROWS = 2000


def range_positions(seed=0) -> torch.Tensor:
    """Sorted distinct table rows in [0, 2^25): both ends, both sides of 2^24
    (byte offset 2^31) and random rows in between."""
    g = _gen(11, seed)
    fixed = [0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, RANGE_V - 2, RANGE_V - 1]
    rnd = torch.randint(2, RANGE_V - 2, (RANGE_ROWS,), generator=g).tolist()
    pos = sorted(set(fixed + rnd))
    return torch.tensor(pos, dtype=torch.int64)


def range_case(B=200, F=43, seed=0):
    """A tower / gather case whose rows are the ``range_positions`` of a 2^25-row
    table: ``c`` indexes the compacted table (c.table[i] is table row pos[i]),
    ``ids`` = row + k V for random signed k are what the kernels get."""
    pos = range_positions(seed)
    n = pos.numel()
    g = _gen(12, B, F, seed)
    pick = torch.randint(0, n, (B, F), generator=g)
    pick.view(-1)[:7] = torch.tensor([0, 1, n - 1, n - 2, *[int((pos == p).nonzero()) for p in
                                                              ((1 << 24) - 1, 1 << 24, (1 << 24) + 1)]])
    c = gather_inputs(B, F, n, n, seed + 3, ids=pick)
    k = torch.randint(-(1 << 37), 1 << 37, (B, F), generator=g)
    ids = pos[pick] + k * RANGE_V
    assert torch.equal(py_mod_rows(ids, RANGE_V, RANGE_V), pos[pick])
    return c, pos, ids


# ------------------------------------------------------------------ the gather itself
# csrc/kernels/embedding.hip through ops.embed / embed_cross / embed_fp8 /
# embedding_bag: every embedding width, both gather kernels (one row per wave,
# and the pipelined walk with one or two rows in flight), arena rows.
GATHER_D = [8, 16, 32, 64, 128]
GATHER_F = [1, 5, 43, 64, 70]  # 64 fills the wave; 70 is embed_kernel's second chunk of fields
GATHER_B = [1, 2, 7, 67, 200]  # 7 / 67: half a pair of rows ends a two-row walk; 1 / 2: less than a block
GATHER_V = TOWER_V
GATHER_BIAS = -1.5
# every D x F; B and the modulus cycle so that each meets every D and every F
GATHER_CASES = [(GATHER_B[(i + j) % 5], F, D, TOWER_MODULI[(i + 2 * j) % 5])
                for i, D in enumerate(GATHER_D) for j, F in enumerate(GATHER_F)]
# (waves, rows in flight) of set_embed_wave_cap; 0 waves: the one-row-per-wave kernel
GATHER_GEOMETRY = [(0, 1), (4, 1), (4, 2), (8, 2), (4096, 1), (4096, 2)]
GATHER_GEOMETRY_SHAPES = [(B, 43, 64) for B in GATHER_B] + [(67, 43, D) for D in GATHER_D if D != 64]
GATHER_ARENA_D = [16, 64, 128]
GATHER_ARENA_GEOMETRY = [(0, 1), (4, 2), (4096, 1)]
GATHER_FIELD_GEOMETRY = [(4, 2), (0, 1)]


def gather_ref(c, bias=GATHER_BIAS):
    """What ops.embed returns for the inputs ``c`` (gather_inputs, or anything
    with table / lin / rows / wts), in float64 and then in the output types."""
    e, first = embed_ref(c)
    _check_gather(c, e, first)
    # the kernels add 0.5 (S_d^2 - sum e^2) per lane to the first-order term and
    # to the bias: every partial sum is a multiple of 0.5
    mag = (c.lin[c.rows].abs() * c.wts).sum(1).double() + abs(bias)
    _check_f32_sum(mag + 0.5 * (e.abs().sum(1).pow(2) + e.pow(2).sum(1)).sum(1), "fm logit", unit=0.5)
    B = e.shape[0]
    second = fm_term(e)
    return SimpleNamespace(e=e, first=first, second=second, bias=bias,
                           x=bf16(e.reshape(B, -1)),
                           fm_bias_only=f32(torch.full((B,), bias, dtype=torch.float64)),
                           fm_first=f32(bias + first),
                           fm_second=f32(bias + second),
                           fm_full=f32(bias + first + second))


@functools.lru_cache(maxsize=64)
def gather_case(B, F, D, modulo, seed=0, V=GATHER_V):
    assert F <= 70, "F = 130 at D = 128 can pass 2^24 in the FM term"
    c = gather_inputs(B, F, V, modulo, seed, D=D)
    return c, gather_ref(c)


def gather_case_from(ids, wts, D, V=GATHER_V, seed=0):
    """The same for given ids / weights (arena rows), modulo V."""
    B, F = ids.shape
    c = gather_inputs(B, F, V, V, seed, ids=ids, wts=wts, D=D)
    return c, gather_ref(c)


def pad_rows(c, n):
    """``c`` with rows n.. replaced by padding (id 0, weight 0): what an arena
    holding the first n rows gives for c.B rows."""
    ids, wts = c.ids.clone(), c.wts.clone()
    ids[n:], wts[n:] = 0, 0
    d = dict(vars(c))
    d.update(ids=ids, wts=wts, rows=py_mod_rows(ids, c.modulo, c.V))
    return SimpleNamespace(**d)


# per-field tables (modulo_f / offset_f) and row shards (shard_lo_f / shard_n_f)
GATHER_FIELD_CASES = [(67, 43, 64, True), (7, 5, 16, True), (67, 70, 128, True), (200, 64, 8, True),
                      (67, 43, 32, False), (2, 5, 128, False)]
_FIELD_MODULI = (1000, 1, 7, 300)


@functools.lru_cache(maxsize=None)
def gather_field_case(B, F, D, shards, seed=0):
    """Field f has its own table of m_f rows at offset_f. With ``shards`` this
    rank holds rows [lo_f, lo_f + n_f) of it - whole tables, middle halves,
    EMPTY shards and ONE-ROW shards cycle over the fields - and an id that
    hashes elsewhere contributes zero to x and to fm. Every third batch row
    is planted inside the shards so that the one-row shards are hit too."""
    g = _gen(13, B, F, D, int(shards), seed)
    m = torch.tensor([_FIELD_MODULI[f % 4] for f in range(F)], dtype=torch.int64)
    lo, n = torch.zeros(F, dtype=torch.int64), m.clone()
    if shards:
        for f in range(F):
            mf, pat = int(m[f]), (f // 4 + f) % 4
            if pat == 1:
                lo[f], n[f] = mf // 4, max(mf // 2, 1)
            elif pat == 2:
                lo[f], n[f] = mf // 2, 0
            elif pat == 3:
                lo[f], n[f] = mf - 1, 1
        assert (n == 0).any() and (n == 1).any()
    off = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int64), n[:-1]]), 0)
    V = int(n.sum()) + 1  # an empty shard at the end still points at a row
    table = _ints(g, -2, 2, (V, D), torch.bfloat16)
    lin = _ints(g, -3, 3, (V,))
    wts = _ints(g, 0, 2, (B, F))
    ids = torch.randint(-(1 << 62), 1 << 62, (B, F), generator=g)
    k = torch.randint(-(1 << 40), 1 << 40, (B, F), generator=g)
    r = (torch.rand(B, F, generator=g) * n).long()
    plant = (torch.arange(B) % 3 == 0)[:, None] & (n > 0)[None, :]
    ids = torch.where(plant, lo + r + k * m, ids)
    nedge = min(4, B * F)
    ids.view(-1)[-nedge:] = torch.tensor(EDGE_IDS[:nedge], dtype=torch.int64)
    h = torch.stack([py_mod_rows(ids[:, f], int(m[f]), int(m[f])) for f in range(F)], 1) - lo
    own = (h >= 0) & (h < n)
    rows = off + torch.where(own, h, torch.zeros_like(h))
    assert rows.min() >= 0 and rows.max() < V
    c = SimpleNamespace(B=B, F=F, V=V, table=table, lin=lin, ids=ids, wts_in=wts, wts=wts * own, rows=rows, own=own,
                        modulo_f=m, offset_f=off, shard_lo_f=lo if shards else None, shard_n_f=n if shards else None)
    if shards:
        live = own & (wts != 0)
        assert live[:, n == 1].any() and not own[:, n == 0].any() and (~own & (wts != 0)).any()
    return c, gather_ref(c)


# ------------------------------------------------------------------ cross network in the gather
GATHER_CROSS_DF = [(64, 43), (16, 43), (32, 64)]
GATHER_CROSS_L = [1, 3]
GATHER_CROSS_B = 67
CROSS_W_NNZ, CROSS_HEAD_NNZ = 8, 8
GATHER_CROSS_LDS = 160 * 1024


def cross_weights(F, D, L, seed=0):
    g = _gen(14, F, D, L, seed)
    d = F * D
    return SimpleNamespace(w=sparse_pm1(g, L, d, CROSS_W_NNZ), hw=sparse_pm1(g, 1, d, CROSS_HEAD_NNZ)[0],
                           b=_ints(g, -1, 1, (L, d)))


def gather_cross_ref(c, k):
    """ops.embed_cross on the gather inputs ``c`` with cross_weights ``k``:
    x0 = the gathered row, x_{l+1} = x0 (x_l . w_l) + b_l + x_l, logit = x_L .
    head_w, layer by layer in float64. The gather kernel folds the network
    into alpha_{l+1} = alpha_l + alpha_l s_l + c_l with s_l = x0 . w_l and
    c_l = (b_0 + .. + b_{l-1}) . w_l (ops.cross_v1_consts): those integers are
    asserted below 2^24 too, and to give the same logit."""
    w, hw, b = k.w, k.hw, k.b
    L, d = w.shape
    e, first = embed_ref(c)
    _check_gather(c, e, first)
    B = e.shape[0]
    x0 = e.reshape(B, d)
    xl = x0
    for l in range(L):
        _check_f32_sum(xl.abs() @ w[l].abs().double(), f"x_{l} . w_{l}")
        xl = x0 * (xl @ w[l].double())[:, None] + b[l].double() + xl
        _check_f32_sum(xl.abs(), f"x_{l + 1}")
    _check_f32_sum(xl.abs() @ hw.abs().double(), "x_L . head_w")
    logit = xl @ hw.double()
    # the kernel's own recurrence
    rows = torch.cat([w, hw[None]]).double()
    beta = torch.cumsum(torch.cat([torch.zeros(1, d), b]), 0).double()
    cc = (beta * rows).sum(1)
    dots = x0 @ rows.t()
    alpha = torch.ones(B, dtype=torch.float64)
    for l in range(L):
        for t in (alpha, alpha * dots[:, l], alpha * dots[:, l] + cc[l]):
            _check_f32_sum(t.abs(), f"alpha step {l}")
        alpha = alpha + alpha * dots[:, l] + cc[l]
    _check_f32_sum(alpha.abs(), "alpha_L")
    _check_f32_sum((alpha * dots[:, L]).abs() + cc[L].abs(), "alpha_L (x0 . head_w) + c_L")
    assert torch.equal(alpha * dots[:, L] + cc[L], logit)
    return SimpleNamespace(x=bf16(x0), logit=f32(logit))


@functools.lru_cache(maxsize=None)
def gather_cross_case(B, F, D, L, seed=0, V=GATHER_V):
    """w_l and head_w have 8 entries of +-1, b_l is in {-1, 0, 1}; with them the
    cases reach |logit| < 10^4 at L = 3."""
    assert (L + 1) * F * D * 4 <= GATHER_CROSS_LDS
    c = gather_inputs(B, F, V, V, seed + 11, D=D)
    k = cross_weights(F, D, L, seed)
    return c, k, gather_cross_ref(c, k)


# ------------------------------------------------------------------ fp8 copy of the gather, row quantisation
GATHER_FP8_CASES = [(67, 43, 64), (7, 43, 8), (200, 5, 16), (67, 64, 32), (2, 1, 128), (67, 21, 128)]
GATHER_FP8_K_PAD = 128
E4M3_MAX = 448.0


def quant_rows_ref(x, k_pad=1):
    """Per-row e4m3 quantisation of rows whose amax / 448 is a power of two and
    whose x / scale are e4m3 values (both asserted): codes uint8 [M, K padded
    with zeros to a multiple of k_pad], scale fp32 [M] (1 for an all-zero row)."""
    x = x.double()
    M, K = x.shape
    amax = x.abs().amax(1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    mant, _ = torch.frexp(scale)
    assert bool((mant == 0.5).all()), "a row's amax / 448 is not a power of two"
    y = x / scale[:, None]
    q = y.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(q.double(), y) and y.abs().max() <= E4M3_MAX, "x / scale is not an e4m3 value"
    Kq = -(-K // k_pad) * k_pad
    codes = torch.zeros(M, Kq, dtype=torch.uint8)
    codes[:, :K] = q.view(torch.uint8)
    return codes, f32(scale)


@functools.lru_cache(maxsize=None)
def gather_fp8_case(B, F, D, seed=0, V=GATHER_V):
    """ops.embed_fp8. Table row r holds 0 or +-7 * 2^(r mod 5); weights are in
    {0, 1, 2}. Batch row b draws its table rows from the classes j <= (2 b) mod 5
    with the top class always present, so neighbouring rows' scales differ by
    4x or more (a scale taken from the next row changes the codes); every
    fifth row from the end has all weights zero (scale 1, codes 0 - or 0x80:
    a negative entry times weight 0 is -0, in x and in its code)."""
    g = _gen(15, B, F, D, seed)
    cls = torch.arange(V) % 5
    table = (_ints(g, -1, 1, (V, D)) * 7 * torch.exp2(cls.float())[:, None]).to(torch.bfloat16)
    table[:, 0] = (7 * torch.exp2(cls.float())).to(torch.bfloat16)  # no all-zero table row
    cap = (2 * torch.arange(B)) % 5
    j = (torch.rand(B, F, generator=g) * (cap + 1)[:, None]).long()
    j[torch.arange(B), torch.arange(B) % F] = cap
    rows = j + 5 * torch.randint(0, V // 5, (B, F), generator=g)
    assert torch.equal(rows % 5, j) and rows.max() < V
    ids = rows + V * torch.randint(-(1 << 40), 1 << 40, (B, F), generator=g)
    assert torch.equal(py_mod_rows(ids, V, V), rows)
    wts = _ints(g, 0, 2, (B, F))
    wts[torch.arange(B), torch.arange(B) % F] = _ints(g, 1, 2, (B,))
    wts[torch.arange(B - 1, -1, -5)] = 0
    assert (wts == 0).all(1).any()
    c = SimpleNamespace(B=B, F=F, V=V, modulo=V, table=table, lin=None, ids=ids, wts=wts, rows=rows)
    return c, gather_fp8_ref(c)


def gather_fp8_ref(c):
    e = c.table[c.rows].double() * c.wts.double()[..., None]
    _check_bf16_ints(e, "x = T[row] * w")
    x = bf16(e.reshape(c.B, -1))
    codes, scale = quant_rows_ref(x, GATHER_FP8_K_PAD)
    assert codes.shape[1] % GATHER_FP8_K_PAD == 0 and not codes[:, c.F * e.shape[2]:].any()
    return SimpleNamespace(x=x, codes=codes, scale=scale)


def quant_rows_views(x):
    """Column ranges of x that ops.quant_rows_fp8 sends to quant_rows16_kernel
    (K a multiple of 16) and to quant_rows_kernel (K = 8 mod 16). The launcher:
    csrc/kernels/interaction.hip launch_quant_rows_fp8."""
    K = x.shape[1]
    k16 = K // 16 * 16
    k8 = K if K % 16 == 8 else (K - 8 if K >= 24 else 0)
    return [k for k in (k16, k8) if k > 0]


# ------------------------------------------------------------------ embedding bag
BAG_SUM_LENS = (0, 1, 3, 4, 5, 64, 65, 130)  # 65 and 130: past one wave pass (512 / D slots) for every D
BAG_MEAN_LENS = (0, 1, 2, 4, 64, 128)  # 1 / len is a power of two
BAG_V = 3000
BAG_CASES = [(D, idx64, mean, out_bf16) for D in GATHER_D for idx64 in (True, False) for mean in (False, True)
             for out_bf16 in (False, True)]


@functools.lru_cache(maxsize=None)
def bag_case(D, idx64, mean, out_bf16, seed=0, V=BAG_V):
    """ops.embedding_bag: three bags of every length in a shuffled order, table
    {-2..2}, per-sample weights {0, 1, 2} (sum pooling; mean takes none),
    indices over the whole int64 / int32 range. bf16 output: the pooled values
    themselves are asserted to be integers (mean: 8-bit integers / 2^k) of
    magnitude <= 256, which they are at every length used."""
    g = _gen(16, D, int(idx64), int(mean), int(out_bf16), seed)
    lens = torch.tensor((BAG_MEAN_LENS if mean else BAG_SUM_LENS) * 3)
    lens = lens[torch.randperm(lens.numel(), generator=g)]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    nnz = int(offsets[-1])
    table = _ints(g, -2, 2, (V, D), torch.bfloat16)
    bits = 62 if idx64 else 31
    idx = torch.randint(-(1 << bits), 1 << bits, (nnz,), generator=g)
    edge = EDGE_IDS if idx64 else (-(1 << 31), (1 << 31) - 1, -1, 0)
    idx[:4] = torch.tensor(edge, dtype=torch.int64)
    idx[-4:] = torch.tensor(edge, dtype=torch.int64)
    rows = py_mod_rows(idx, V, V)
    psw = None if mean else _ints(g, 0, 2, (nnz,))
    c = SimpleNamespace(D=D, table=table, idx=idx if idx64 else idx.to(torch.int32), offsets=offsets, psw=psw,
                        rows=rows, lens=lens, mean=mean, out_bf16=out_bf16, V=V)
    return c, bag_ref(c)


def bag_ref(c, keep=None):
    """float64 pooling; ``keep`` (bool [nnz]) drops elements: the CPU tests' mutant."""
    w = torch.ones(c.rows.numel(), dtype=torch.float64) if c.psw is None else c.psw.double()
    if keep is not None:
        w = w * keep
    v = c.table[c.rows].double() * w[:, None]
    out = torch.zeros(c.lens.numel(), c.D, dtype=torch.float64)
    mag = torch.zeros_like(out)
    bag = torch.repeat_interleave(torch.arange(c.lens.numel()), c.lens)
    out.index_add_(0, bag, v)
    mag.index_add_(0, bag, v.abs())
    _check_f32_sum(mag, "bag sums")
    if c.out_bf16:
        _check_bf16_ints(out, "bag sums as bf16")
    if c.mean:
        out = out / c.lens.clamp(min=1).double()[:, None]
    return bf16(out) if c.out_bf16 else f32(out)
