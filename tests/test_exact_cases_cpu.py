"""The exact small-integer cases of tests/test_kernels_exact_gpu.py, checked
without a GPU: every parametrised case meets its exactness conditions, and
faults injected into the reference change its output - so the torch.equal
comparisons of the GPU file can fail."""
import os
import sys

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
