"""The exact small-integer cases of tests/test_kernels_exact_gpu.py, checked
without a GPU: every parametrised case meets its exactness conditions, and
faults injected into the reference change its output - so the torch.equal
comparisons of the GPU file can fail."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_cases as xc  # noqa: E402


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", xc.TOWER_CASES + xc.TOWER_MODULO_CASES + xc.TOWER_FORM_CASES)
def test_tower_cases_are_exact(case):
    """The generator asserts max |h1|, max |h2| <= 256 and every fp32 sum below
    2^24; the float64 reference is then an fp32 value, and the edge ids are in."""
    c, w, r = xc.tower_case(*case)
    B, F, V, fm, act2, act3, modulo = case
    xc.f32(r.logit)
    assert r.h1.abs().max() <= 256 and r.h2.abs().max() <= 256
    assert c.rows.min() >= 0 and c.rows.max() <= V - 1
    have = set(c.ids.view(-1).tolist())
    assert set(xc.EDGE_IDS[:min(4, B * F)]) <= have
    assert (c.wts == 0).any() or B * F < 8
    if modulo > (1 << 32) - 2:  # rows past V clamp to V - 1
        assert (c.rows == V - 1).sum() > B * F // 2
    # the same reference evaluated in fp32 is bit-identical: nothing in it rounds
    e = c.table[c.rows].float() * c.wts[..., None]
    h1 = torch.relu(e.reshape(B, -1) @ w.W1.t() + w.b1)
    assert torch.equal(h1.double(), r.h1)


@pytest.mark.parametrize("case", xc.GATHER_GEMM_CASES)
def test_gather_gemm_cases_are_exact(case):
    c, w, r = xc.gather_gemm_case(*case)
    xc.bf16(r.h)
    xc.f32(r.part0)
    if r.part1 is not None:
        xc.f32(r.part1)


def test_dense_cases_are_exact():
    for M, N, K in xc.GEMM_SHAPES:
        for act, out_bf16 in xc.GEMM_EPI_OUT:
            xc.gemm_case(M, N, K, out_bf16, act)
    for M in xc.MLP_M:
        for act2, act3 in (("relu", "relu"), ("none", "none"), ("relu", "none")):
            xc.mlp_tail_case(M, act2, act3)
        for N, K in xc.LINEAR_HEAD_NK:
            for act in ("relu", "none"):
                xc.linear_head_case(M, N, K, act)
        for nd in (13, 64):
            xc.bottom_mlp3_case(M, nd)
    for T in xc.INTERACTION_T:
        xc.interaction_case(T)
        xc.interaction_gather_case(T)


def test_fp8_cases_are_exact():
    for M, N, K in xc.FP8_SHAPES + [xc.FP8_VARIANT_SHAPE]:
        for act in ("none", "relu"):
            xc.fp8_case(M, N, K, act)
    c = xc.fp8_case(*xc.MX_SHAPE, mx=True)
    # the exponents differ from row to row and from block to block
    assert (c.sx_blk[1:] != c.sx_blk[:-1]).any(dim=1).all() and (c.sx_blk[:, 1:] != c.sx_blk[:, :-1]).any(dim=1).all()
    for M, N in xc.CROSS_FP8_SHAPES:
        xc.cross_fp8_case(M, N)


def test_range_case_covers_both_halves():
    c, pos, ids = xc.range_case()
    assert pos[0] == 0 and pos[-1] == xc.RANGE_V - 1 and pos.numel() >= 1900
    rows = pos[c.rows]
    assert {0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, xc.RANGE_V - 2, xc.RANGE_V - 1} <= set(rows.view(-1).tolist())
    assert (rows * 128 >= 1 << 31).float().mean() > 0.3  # byte offsets a signed 32-bit reading would break
    assert (ids < 0).any() and (ids > 0).any()
    xc.f32(xc.tower_ref(c, xc.tower_weights(c.F), True, "relu", "relu").logit)


# ------------------------------------------------------------------ mutants
MUTANT_CASES = [(200, F, xc.TOWER_V) + acts + (xc.TOWER_V,) for F in (1, 7, 43, 64) for acts in xc.TOWER_ACTS]


def _differ(a, b):
    return (a != b).double().mean().item()


@pytest.mark.parametrize("case", MUTANT_CASES)
def test_mutant_wrong_row_of_one_field(case):
    """One field's table row replaced in every batch row, the first-order term
    intact (a wrong LDS-DMA source or a stale ring slot): at least 90 % of the
    rows whose weight for that field is non-zero change."""
    B, F, V, fm, act2, act3, modulo = case
    c, w, r = xc.tower_case(*case)
    f = F // 2
    wrong = c.table[(c.rows[:, f] + 1) % V].double() * c.wts[:, f].double()[:, None]

    def hook(e):
        e = e.clone()
        e[:, f] = wrong
        return e

    m = xc.tower_ref(c, w, fm, act2, act3, e_hook=hook, check=False)
    live = c.wts[:, f] != 0
    assert live.sum() > B // 2
    share = _differ(m.logit[live], r.logit[live])
    assert share >= 0.9, f"only {share:.2%} of the live rows changed"
    assert torch.equal(m.logit[~live], r.logit[~live])


@pytest.mark.parametrize("case", MUTANT_CASES)
def test_mutant_h1_layout(case):
    """h1 columns n and n + 1 swapped, and two 32-column blocks swapped (a
    fragment-order slip, an LDS chunk in the wrong place): at least 25 % of the
    rows change."""
    B, F, V, fm, act2, act3, modulo = case
    c, w, r = xc.tower_case(*case)

    def swap_cols(h1, n=5):
        h1 = h1.clone()
        h1[:, [n, n + 1]] = h1[:, [n + 1, n]]
        return h1

    def swap_blocks(h1, a=2, b=19):
        h1 = h1.clone()
        h1[:, 32 * a:32 * a + 32], h1[:, 32 * b:32 * b + 32] = r.h1[:, 32 * b:32 * b + 32], r.h1[:, 32 * a:32 * a + 32]
        return h1

    for name, hook in (("columns", swap_cols), ("blocks", swap_blocks)):
        m = xc.tower_ref(c, w, fm, act2, act3, h1_hook=hook, check=False)
        share = _differ(m.logit, r.logit)
        assert share >= 0.25, f"{name}: only {share:.2%} of the rows changed"


@pytest.mark.parametrize("case", MUTANT_CASES)
def test_mutant_dropped_k_step(case):
    """One 16-wide K step of one field's tile zeroed in the MLP input."""
    B, F, V, fm, act2, act3, modulo = case
    c, w, r = xc.tower_case(*case)

    def hook(x):
        x[:, F - 1, 32:48] = 0
        return x

    m = xc.tower_ref(c, w, fm, act2, act3, x_hook=hook, check=False)
    assert not torch.equal(m.logit, r.logit)
    assert not torch.equal(m.h1, r.h1)


def test_mutant_mx_scales():
    """MX block scales read from the next row, or from the next block."""
    c = xc.fp8_case(*xc.MX_SHAPE, mx=True)
    args = (c.q.float(), None, c.Wq.float(), c.sw, c.b, c.act)
    assert torch.equal(xc.fp8_ref(*args, sx_blk=c.sx_blk).float(), c.y)
    for dim in (0, 1):
        m = xc.fp8_ref(*args, sx_blk=torch.roll(c.sx_blk, -1, dims=dim))
        assert not torch.equal(m.float(), c.y)
        assert _differ(m.float(), c.y) > 0.5
    # with one exponent row shared by every row (how the tolerance test draws
    # them) the row mutant is invisible
    shared = c.sx_blk[:1].expand_as(c.sx_blk).contiguous()
    assert torch.equal(xc.fp8_ref(*args, sx_blk=shared), xc.fp8_ref(*args, sx_blk=torch.roll(shared, -1, dims=0)))


# ------------------------------------------------------------------ the finding
def test_tolerance_inputs_hide_a_wrong_row_without_fm():
    """Why the exact file exists. With the scalings of test_kernels_gpu.py's
    _gather_gemm_case (table +-0.1, W1 +-0.025: the MLP's logit is about 0.06)
    and the fp32 tower reference of test_gather_mlp_tower_vs_fp32 with
    fm=False, replacing one field's table row in EVERY batch row (first-order
    term intact) moves no score past that test's 2e-3 + 2e-3 |ref|: a stale
    ring slot or a wrong DMA source for one field passes it. A statement about
    those inputs, not about the kernel."""
    import test_kernels_gpu as tk  # its input scalings and its reference, as they stand

    B, F, V, bias, f = 2048, 43, 30_000, -0.25, 21
    table, lin, W1, b1, ids, wts = tk._gather_gemm_case(B, F=F, V=V, N=1024, seed=B + F)
    g = torch.Generator().manual_seed(B * 7 + F)
    W2 = (torch.randn(512, 1024, generator=g) / 32).to(torch.bfloat16)
    W3 = (torch.randn(256, 512, generator=g) / 512 ** 0.5).to(torch.bfloat16)
    b2, b3 = torch.randn(512, generator=g) * 0.1, torch.randn(256, generator=g) * 0.1
    hw = torch.randn(256, generator=g) * 0.05

    def score(ids_mlp):
        h1, _ = tk._gather_gemm_ref(table, lin, W1, b1, ids_mlp, wts, V, bias, False)
        _, first = tk._gather_gemm_ref(table, lin, W1, b1, ids, wts, V, bias, False)  # keeps the right rows
        return tk._mlp_tail_ref(h1.to(torch.bfloat16), W2, b2, "relu", W3, b3, "relu", hw, 0.2, first, True)

    ref = score(ids)
    wrong = ids.clone()
    wrong[:, f] += 1  # the next table row
    assert (table[torch.remainder(wrong[:, f], V)] != table[torch.remainder(ids[:, f], V)]).any(dim=1).all()
    err = (score(wrong) - ref).abs()
    assert err.max() > 0  # the mutant does change the scores ...
    over = (err > 2e-3 + 2e-3 * ref.abs()).sum().item()
    assert over == 0, f"{over} rows leave the tolerance"  # ... and none leaves the tolerance


# ------------------------------------------------------------------ the gather's own cases
# (tests/test_gather_exact_gpu.py) - conditions, the project's CPU paths, mutants
from distributed_tf_serving_amd import ops  # noqa: E402

GATHER_ALL = sorted(set(xc.GATHER_CASES + [(B, F, D, xc.GATHER_V) for B, F, D in xc.GATHER_GEOMETRY_SHAPES] +
                        [(67, 64, D, xc.GATHER_V) for D in xc.GATHER_D]))


def _cpu_embed_all(c, r, ids, wts, **kw):
    for lin, want_x, fm2, fm_ref in ((c.lin, True, True, r.fm_full), (c.lin, False, False, r.fm_first),
                                     (None, True, True, r.fm_second), (None, False, False, r.fm_bias_only)):
        x, fm = ops.embed(c.table, ids, wts, lin=lin, bias=r.bias, want_x=want_x, want_fm=True, fm2=fm2, **kw)
        assert (x is None) == (not want_x) and (x is None or torch.equal(x, r.x))
        assert fm.dtype == torch.float32 and torch.equal(fm, fm_ref)


@pytest.mark.parametrize("case", GATHER_ALL)
def test_gather_cases_are_exact(case):
    """Every D x F x modulus case meets its conditions (gather_ref asserts
    them), carries the edge ids and zero weights, and ops.embed's CPU path
    returns the reference exactly. That path takes a modulus up to the table's
    rows, so the larger moduli reach it as the rows they resolve to."""
    B, F, D, modulo = case
    c, r = xc.gather_case(*case)
    assert c.table.shape == (xc.GATHER_V, D) and r.x.shape == (B, F * D)
    assert c.rows.min() >= 0 and c.rows.max() <= c.V - 1
    assert set(xc.EDGE_IDS[:min(4, B * F)]) <= set(c.ids.view(-1).tolist())
    assert (c.wts == 0).any() or B * F < 8
    if modulo > c.V:
        assert (c.rows == c.V - 1).sum() > B * F // 2
        _cpu_embed_all(c, r, c.rows, c.wts, modulo=c.V)
    else:
        _cpu_embed_all(c, r, c.ids, c.wts, modulo=modulo)
    _cpu_embed_all(c, r, c.rows.to(torch.int32), c.wts, modulo=c.V)


def test_gather_d64_keeps_the_tower_inputs():
    """gather_inputs at the default width draws what it drew before it took D."""
    a = xc.gather_inputs(65, 43, xc.TOWER_V, xc.TOWER_V, 0)
    b = xc.gather_inputs(65, 43, xc.TOWER_V, xc.TOWER_V, 0, D=64)
    assert torch.equal(a.table, b.table) and torch.equal(a.ids, b.ids) and a.table.shape[1] == 64
    assert not torch.equal(a.ids, xc.gather_inputs(65, 43, xc.TOWER_V, xc.TOWER_V, 0, D=32).ids)


@pytest.mark.parametrize("case", xc.GATHER_FIELD_CASES)
def test_gather_field_cases_are_exact(case):
    B, F, D, shards = case
    c, r = xc.gather_field_case(*case)
    kw = {k: getattr(c, k) for k in ("modulo_f", "offset_f", "shard_lo_f", "shard_n_f") if getattr(c, k) is not None}
    _cpu_embed_all(c, r, c.ids, c.wts_in, **kw)
    if shards:  # rows of another shard: zero in x, nothing in fm
        e = r.x.view(B, F, D)
        assert not e[~c.own].any() and (c.shard_n_f == 0).any() and (c.shard_n_f == 1).any()
        assert e[:, c.shard_n_f == 1].any()


@pytest.mark.parametrize("L", xc.GATHER_CROSS_L)
@pytest.mark.parametrize("D,F", xc.GATHER_CROSS_DF)
def test_gather_cross_cases_are_exact(D, F, L):
    c, k, r = xc.gather_cross_case(xc.GATHER_CROSS_B, F, D, L)
    x, logit = ops.embed_cross(c.table, c.ids, c.wts, c.V, k.w, k.b, k.hw)
    assert torch.equal(x, r.x) and torch.equal(logit, r.logit)
    assert (r.logit != 0).float().mean() > 0.8
    rows, cc = ops.cross_v1_consts(k.w, k.b, k.hw)  # what the GPU kernel is handed: integers, exactly
    assert torch.equal(rows, torch.cat([k.w, k.hw[None]])) and xc._is_int(cc)
    p = xc.gather_cross_ref(xc.pad_rows(c, 40), k)  # padding rows: x0 = 0, logit = c_L
    assert not p.x[40:].any() and (p.logit[40:] == cc[-1]).all()


@pytest.mark.parametrize("case", xc.GATHER_FP8_CASES)
def test_gather_fp8_cases_are_exact(case):
    B, F, D = case
    c, r = xc.gather_fp8_case(*case)
    assert r.codes.dtype == torch.uint8 and r.codes.shape == (B, -(-F * D // 128) * 128)
    zero = (c.wts == 0).all(1)  # a negative entry times weight 0 is -0: code 0x80
    assert zero.any() and (r.scale[zero] == 1).all() and not (r.codes[zero] & 0x7F).any()
    x, q, s = ops.embed_fp8(c.table, c.ids, c.wts, c.V, xc.GATHER_FP8_K_PAD)
    assert torch.equal(x, r.x) and torch.equal(s, r.scale) and torch.equal(q.view(torch.uint8), r.codes)
    ks = xc.quant_rows_views(r.x)
    assert any(k % 16 == 0 for k in ks) and (any(k % 16 == 8 for k in ks) or F * D < 24)
    for K in ks:
        codes, scale = xc.quant_rows_ref(r.x[:, :K], xc.GATHER_FP8_K_PAD)
        q, s = ops.quant_rows_fp8(r.x[:, :K], xc.GATHER_FP8_K_PAD)
        assert torch.equal(s, scale) and torch.equal(q.view(torch.uint8), codes)


@pytest.mark.parametrize("case", xc.BAG_CASES)
def test_bag_cases_are_exact(case):
    D, idx64, mean, out_bf16 = case
    c, want = xc.bag_case(*case)
    assert c.idx.dtype == (torch.int64 if idx64 else torch.int32) and c.lens.max() > 512 // D
    lim = 63 if idx64 else 31
    assert {-(1 << lim), (1 << lim) - 1, -1, 0} <= set(c.idx.tolist())
    out = torch.full(want.shape, float("nan"), dtype=want.dtype)
    y = ops.embedding_bag(c.table, c.idx, c.offsets, c.psw, modulo=c.V, mean=mean, out_bf16=out_bf16, out=out)
    assert y.dtype == want.dtype and torch.equal(y, want) and torch.equal(out, want)


GATHER_MUTANT_CASES = [(200, F, D, xc.GATHER_V) for D in xc.GATHER_D for F in (5, 43)]
MUTANT_NWAVES = 4


def _share(a, b, live):
    d = (a != b).reshape(a.shape[0], -1).any(1)
    assert not d[~live].any(), "a row the mutant does not touch changed"
    return d[live].double().mean().item()


@pytest.mark.parametrize("case", GATHER_MUTANT_CASES)
def test_mutant_gather_pairs_the_wrong_row(case):
    """A two-row walk that resolves row b from the ids of row b + nwaves (its
    weights intact): x and fm change in at least 90 % of the rows with a
    non-zero weight."""
    c, r = xc.gather_case(*case)
    m = SimpleNamespace(**{**vars(c), "rows": torch.roll(c.rows, -MUTANT_NWAVES, 0)})
    e, first = xc.embed_ref(m)
    live = (c.wts != 0).any(1)
    assert live.sum() > c.B // 2
    assert _share(e.reshape(c.B, -1), r.e.reshape(c.B, -1), live) >= 0.9
    assert _share(r.bias + first + xc.fm_term(e), r.fm_full.double(), live) >= 0.9


@pytest.mark.parametrize("case", GATHER_MUTANT_CASES)
def test_mutant_fm_term(case):
    """One field's squares left out of sum e^2, and one group of 8 dimensions
    left out of S_d (every group: each D reduces them over other lanes)."""
    B, F, D, _ = case
    c, r = xc.gather_case(*case)
    f = F // 2
    live = c.wts[:, f] != 0
    assert live.sum() > B // 2
    fm = r.fm_full.double() + 0.5 * r.e[:, f].pow(2).sum(1)
    share = _share(fm, r.fm_full.double(), live)
    assert share >= 0.9, f"squares of field {f}: only {share:.2%} of the live rows changed"
    live = (c.wts != 0).any(1)
    q = r.e.pow(2).sum(1)
    for grp in range(D // 8):
        s = r.e.sum(1)
        s[:, 8 * grp:8 * grp + 8] = 0
        fm = r.bias + r.first + 0.5 * (s.pow(2) - q).sum(1)
        share = _share(fm, r.fm_full.double(), live)
        assert share >= 0.9, f"dimensions {8 * grp}..: only {share:.2%} of the live rows changed"


@pytest.mark.parametrize("case", GATHER_MUTANT_CASES)
def test_mutant_lin_of_one_field(case):
    """One field's first-order weight dropped. lin is in {-3..3}: a seventh of
    the rows would carry a zero there and hide it, so this case's ids of that
    field are moved onto rows with lin != 0 first."""
    B, F, D, V = case
    c0, _ = xc.gather_case(*case)
    f = F // 2
    nz = (c0.lin != 0).nonzero().view(-1)
    ids = c0.ids.clone()
    zero = c0.lin[c0.rows[:, f]] == 0
    ids[zero, f] = nz[torch.arange(B) % nz.numel()][zero]
    c, r = xc.gather_case_from(ids, c0.wts, D)
    assert torch.equal(c.lin, c0.lin) and torch.equal(c.table, c0.table) and (c.lin[c.rows[:, f]] != 0).all()
    live = c.wts[:, f] != 0
    assert live.sum() > B // 2
    fm = r.fm_full.double() - c.lin[c.rows[:, f]].double() * c.wts[:, f].double()
    assert _share(fm, r.fm_full.double(), live) >= 0.9


@pytest.mark.parametrize("D", xc.GATHER_D)
@pytest.mark.parametrize("mean", [False, True])
def test_mutant_bag_second_pass(D, mean):
    """A bag pooled from its first wave pass (512 / D slots) alone."""
    c, want = xc.bag_case(D, True, mean, False)
    pos = torch.arange(c.rows.numel()) - torch.repeat_interleave(c.offsets[:-1], c.lens)
    keep = pos < 512 // D
    w = torch.ones(c.rows.numel()) if c.psw is None else c.psw
    live = torch.zeros(c.lens.numel()).index_add_(0, torch.repeat_interleave(torch.arange(c.lens.numel()), c.lens),
                                                  (~keep).float() * w) > 0
    assert live.sum() >= 3
    share = _share(xc.bag_ref(c, keep), want, live)
    assert share >= 0.9, f"only {share:.2%} of the long bags changed"


@pytest.mark.parametrize("case", xc.GATHER_FP8_CASES)
def test_mutant_fp8_scale_of_the_next_row(case):
    """Codes computed with the neighbouring row's scale."""
    c, r = xc.gather_fp8_case(*case)
    wrong = torch.roll(r.scale, -1)
    y = (r.x.float() / wrong[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    live = r.x.float().abs().amax(1) > 0
    assert live.any()
    share = _share(y, r.codes[:, :y.shape[1]], live)
    assert share >= 0.9, f"only {share:.2%} of the live rows changed"
