"""Exact small-integer probes of csrc/kernels/embedding.hip and the row
quantisation kernels: every embedding width, both gather kernels (one row per
wave; the pipelined walk with one and with two rows in flight), id tensors,
int32 rows, strided narrow rows and arena rows, the cross network and the
e4m3 copy inside the gather, and the embedding bag. The cases and their
float64 references are tests/exact_cases.py's; every assertion is torch.equal
or identical bits."""
import contextlib
import os
import sys

import pytest
import torch

from distributed_tf_serving_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cases as xc  # noqa: E402
from arena_cases import arena_case  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULT_GEOMETRY = (4096, 1)


@contextlib.contextmanager
def _geometry(waves, rows_in_flight):
    """The gather's grid is a process-global setting: always put it back."""
    h = ops.hip()
    try:
        h.set_embed_wave_cap(waves, rows_in_flight)
        yield
    finally:
        h.set_embed_wave_cap(4096)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t.contiguous().view(
        {2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _twice(fn):
    """Every launch runs twice and must repeat its bits; returns CPU tensors."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(_bits(u), _bits(v)), "two runs of the gather differ"
    return [None if u is None else u.cpu() for u in a]


def _check_embed(dev, c, r, ids, wts, what, **kw):
    """ops.embed with x / fm / the second-order term / lin on and off."""
    table, lin = c.table.to(dev), c.lin.to(dev)
    for lin_on, want_x, want_fm, fm2, fm_ref in ((True, True, True, True, r.fm_full),
                                                 (True, False, True, False, r.fm_first),
                                                 (False, True, True, True, r.fm_second),
                                                 (False, False, True, False, r.fm_bias_only),
                                                 (False, True, False, False, None)):
        x, fm = _twice(lambda: ops.embed(table, ids, wts, lin=lin if lin_on else None, bias=r.bias, want_x=want_x,
                                         want_fm=want_fm, fm2=fm2, **kw))
        tag = (what, lin_on, want_x, want_fm, fm2)
        assert (x is not None) == want_x and (fm is not None) == want_fm, tag
        if want_x:
            assert x.dtype == torch.bfloat16 and torch.equal(x, r.x), tag
        if want_fm:
            assert fm.dtype == torch.float32 and torch.equal(fm, fm_ref), tag


def _modulo_kw(c, dev):
    """The shared-table gather takes a modulus up to the table's rows; a larger
    one (rows clamp to V - 1) goes in as one per-field table per field."""
    if c.modulo <= c.V:
        return dict(modulo=c.modulo)
    return dict(modulo_f=torch.full((c.F,), c.modulo, dtype=torch.int64, device=dev),
                offset_f=torch.zeros(c.F, dtype=torch.int64, device=dev))


def _check_embed_forms(dev, c, r):
    """int64 ids, int32 rows (with fp32 and with bf16 weights), and the strided
    narrow rows of the candidate fan-out."""
    from distributed_tf_serving_amd.serving.packing import PackedLayout

    wts = c.wts.to(dev)
    _check_embed(dev, c, r, c.ids.to(dev), wts, "int64 ids", **_modulo_kw(c, dev))
    _check_embed(dev, c, r, c.rows.to(torch.int32).to(dev), wts, "int32 rows", modulo=c.V)
    _check_embed(dev, c, r, c.rows.to(torch.int32).to(dev), xc.bf16(c.wts).to(dev), "bf16 weights", modulo=c.V)
    L = PackedLayout(c.F, narrow_modulo=c.V)
    buf = L.pack(c.rows, c.wts).to(dev)
    iv, wv = L.ids(buf), L.wts(buf)
    assert iv.stride(0) > c.F and iv.dtype == torch.int32  # row views of the packed buffer
    _check_embed(dev, c, r, iv, wv, "narrow rows", modulo=c.V)


# ------------------------------------------------------------------ ops.embed
@pytest.mark.parametrize("case", xc.GATHER_CASES)
def test_embed_exact(cuda, case):
    """Every D with every F (70: embed_kernel's second chunk of fields), row
    counts below a block of waves and past it, every modulo path."""
    c, r = xc.gather_case(*case)
    with _geometry(*DEFAULT_GEOMETRY):
        _check_embed_forms(cuda, c, r)


@pytest.mark.parametrize("shape", xc.GATHER_GEOMETRY_SHAPES)
@pytest.mark.parametrize("geometry", xc.GATHER_GEOMETRY)
def test_embed_exact_geometry(cuda, geometry, shape):
    """The one-row-per-wave kernel (0 waves) and the pipelined walk with one
    and two rows in flight, few waves (many rows per wave, half a pair at the
    end) and many."""
    B, F, D = shape
    c, r = xc.gather_case(B, F, D, xc.GATHER_V)
    with _geometry(*geometry):
        _check_embed_forms(cuda, c, r)


@pytest.mark.parametrize("D", xc.GATHER_D)
@pytest.mark.parametrize("geometry", [(0, 1), (4, 2)])
def test_embed_exact_64_fields_no_pipeline(cuda, geometry, D):
    """F = 64 through embed_kernel's single full chunk, and through a two-row walk."""
    c, r = xc.gather_case(67, 64, D, xc.GATHER_V)
    with _geometry(*geometry):
        _check_embed_forms(cuda, c, r)


@pytest.mark.parametrize("case", xc.GATHER_FIELD_CASES)
@pytest.mark.parametrize("geometry", xc.GATHER_FIELD_GEOMETRY)
def test_embed_exact_field_tables_and_shards(cuda, geometry, case):
    """Per-field tables, and row shards with an empty and a one-row shard:
    rows of another shard give zero in x and in fm."""
    c, r = xc.gather_field_case(*case)
    kw = {k: getattr(c, k).to(cuda) for k in ("modulo_f", "offset_f", "shard_lo_f", "shard_n_f")
          if getattr(c, k) is not None}
    with _geometry(*geometry):
        _check_embed(cuda, c, r, c.ids.to(cuda), c.wts_in.to(cuda), "per-field", **kw)


def _arena_sizes(B):
    """A raw, a packed-varint and a one-row request, fewer rows than B."""
    return {200: [(3, True), (150, False), (1, True), (37, True)], 67: [(3, True), (40, False), (1, True), (20, True)],
            7: [(1, True), (4, False)], 2: [(1, False)]}[B]


def _arena(dev, F, B, seed, rows=None):
    A, ar, ids, wts = arena_case(F, _arena_sizes(B), B, seed, rows=rows)
    d = ar.to(dev)
    A.decode_varints(d)
    return ops.ArenaRows(d, B, F), ids, wts, sum(n for n, _ in _arena_sizes(B))


@pytest.mark.parametrize("B,F", [(200, 43), (67, 64), (7, 5)])
@pytest.mark.parametrize("D", xc.GATHER_ARENA_D)
def test_embed_exact_arena_rows(cuda, D, B, F):
    """The gather reading request bytes, padding rows past the requests."""
    rows, ids, wts, n = _arena(cuda, F, B, seed=31 + F)
    c, r = xc.gather_case_from(ids, wts, D)
    assert not r.x[n:].any() and torch.equal(r.fm_full[n:], r.fm_bias_only[n:])  # padding: zero x, fm = bias
    for geometry in xc.GATHER_ARENA_GEOMETRY:
        with _geometry(*geometry):
            _check_embed(cuda, c, r, rows, None, ("arena", geometry), modulo=c.V)


# ------------------------------------------------------------------ ops.embed_cross
@pytest.mark.parametrize("L", xc.GATHER_CROSS_L)
@pytest.mark.parametrize("D,F", xc.GATHER_CROSS_DF)
@pytest.mark.parametrize("geometry", [(4096, 1), (4, 2)])
def test_embed_cross_exact(cuda, geometry, D, F, L):
    """The cross network inside the gather, from ids and from arena rows."""
    B = xc.GATHER_CROSS_B
    c, k, r = xc.gather_cross_case(B, F, D, L)
    table, w, b, hw = (t.to(cuda) for t in (c.table, k.w, k.b, k.hw))
    ids, wts = c.ids.to(cuda), c.wts.to(cuda)
    rows, _, _, n = _arena(cuda, F, B, 0, rows=(c.ids, c.wts))
    ra = xc.gather_cross_ref(xc.pad_rows(c, n), k)
    with _geometry(*geometry):
        x, logit = _twice(lambda: ops.embed_cross(table, ids, wts, c.V, w, b, hw))
        xa, la = _twice(lambda: ops.embed_cross(table, rows, None, c.V, w, b, hw))
        x32, l32 = _twice(lambda: ops.embed_cross(table, c.rows.to(torch.int32).to(cuda), wts, c.V, w, b, hw))
    assert torch.equal(x, r.x) and torch.equal(logit, r.logit)
    assert torch.equal(x32, r.x) and torch.equal(l32, r.logit), "int32 rows"
    assert torch.equal(xa, ra.x) and torch.equal(la, ra.logit), "arena rows"


# ------------------------------------------------------------------ ops.embed_fp8, ops.quant_rows_fp8
@pytest.mark.parametrize("case", xc.GATHER_FP8_CASES)
@pytest.mark.parametrize("geometry", [(4096, 1), (4, 2)])
def test_embed_fp8_exact(cuda, geometry, case):
    """The gather's own e4m3 copy: codes, scales and the zero K padding."""
    B, F, D = case
    c, r = xc.gather_fp8_case(*case)
    table, ids, wts = c.table.to(cuda), c.ids.to(cuda), c.wts.to(cuda)
    rows, _, _, n = _arena(cuda, F, B, 0, rows=(c.ids, c.wts))
    ra = xc.gather_fp8_ref(xc.pad_rows(c, n))
    with _geometry(*geometry):
        got = _twice(lambda: ops.embed_fp8(table, ids, wts, c.V, xc.GATHER_FP8_K_PAD))
        gota = _twice(lambda: ops.embed_fp8(table, rows, None, c.V, xc.GATHER_FP8_K_PAD))
        got32 = _twice(lambda: ops.embed_fp8(table, c.rows.to(torch.int32).to(cuda), wts, c.V, xc.GATHER_FP8_K_PAD))
    for (x, q, sc), want, what in ((got, r, "ids"), (gota, ra, "arena rows"), (got32, r, "int32 rows")):
        assert q.dtype == torch.float8_e4m3fn and q.shape == want.codes.shape, what
        assert torch.equal(x, want.x), what
        assert torch.equal(sc, want.scale), what
        assert torch.equal(q.view(torch.uint8), want.codes), what


@pytest.mark.parametrize("case", xc.GATHER_FP8_CASES)
def test_quant_rows_fp8_exact(cuda, case):
    """quant_rows16_kernel (K a multiple of 16) and quant_rows_kernel (K = 8
    mod 16) on column ranges of the same rows (copied: the binding takes
    contiguous rows only)."""
    c, r = xc.gather_fp8_case(*case)
    x = r.x.to(cuda)
    ks = xc.quant_rows_views(r.x)
    assert ks
    for K in ks:
        codes, scale = xc.quant_rows_ref(r.x[:, :K], xc.GATHER_FP8_K_PAD)
        xk = x[:, :K].contiguous()
        q, sc = _twice(lambda: ops.quant_rows_fp8(xk, xc.GATHER_FP8_K_PAD))
        assert q.shape == codes.shape and torch.equal(sc, scale), K
        assert torch.equal(q.view(torch.uint8), codes), K


# ------------------------------------------------------------------ ops.embedding_bag
@pytest.mark.parametrize("case", xc.BAG_CASES)
def test_embedding_bag_exact(cuda, case):
    """Every D, int64 and int32 indices, sum (weighted) and mean pooling, fp32
    output and bf16 into an out= buffer; bags of more than one wave pass."""
    D, idx64, mean, out_bf16 = case
    c, want = xc.bag_case(*case)
    table, idx, off = c.table.to(cuda), c.idx.to(cuda), c.offsets.to(cuda)
    psw = None if c.psw is None else c.psw.to(cuda)
    nb = c.lens.numel()
    out = torch.full((nb, D), float("nan"), dtype=torch.bfloat16, device=cuda) if out_bf16 else None
    (y,) = _twice(lambda: (ops.embedding_bag(table, idx, off, psw, modulo=c.V, mean=mean, out_bf16=out_bf16,
                                             out=out),))
    assert y.dtype == want.dtype and y.shape == want.shape and torch.equal(y, want)
    if out_bf16:
        assert torch.equal(out.cpu(), want)
