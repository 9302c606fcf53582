"""The cases of tests/smallgemm_cases.py are what they claim: exact in fp32 in any summation order, representable in bf16, rounded
and tied often enough that a bit-for-bit pass says something about the one fp32 -> bf16 rounding, and sensitive to the defects a
loose tolerance would hide — so that a pass of tests/test_smallgemm_exact_gpu.py means the kernels computed the right thing."""
import pytest
import torch

import smallgemm_cases as SC

CASES = SC.ALL
IDS = [SC.case_id(c) for c in CASES]


def _operands(c):
    return {"tn": SC.tn_operands, "nn": SC.nn_operands, "wgrad": SC.wgrad_operands}[c.kind](c)


def _refs(c):
    """every float64 reference the GPU test compares against for this case, by variant name"""
    if c.kind == "tn":
        x, w, b = SC.tn_operands(c)
        return {(bias, relu): SC.ref_tn(x, w, b if bias else None, relu) for bias in (False, True) for relu in (False, True)}
    if c.kind == "nn":
        dy, w, base, h = SC.nn_operands(c)
        return {(acc, mask): SC.ref_nn(dy, w, base if acc else None, h if mask else None) for acc in (False, True) for mask in (False, True)}
    dy, x = SC.wgrad_operands(c)
    return {"dw": SC.ref_wgrad(dy, x)}


def _one_element(c, j):
    """the contribution of contraction element j to the plain product"""
    if c.kind == "tn":
        x, w, _ = SC.tn_operands(c)
        return torch.outer(x[:, j].double(), w[:, j].double())
    if c.kind == "nn":
        dy, w, _, _ = SC.nn_operands(c)
        return torch.outer(dy[:, j].double(), w[j].double())
    dy, x = SC.wgrad_operands(c)
    return torch.outer(dy[j].double(), x[j].double())


def test_the_table_holds_the_shapes_that_reach_every_kernel_form():
    forms = {(c.kind, c.form) for c in CASES}
    assert forms >= {("tn", "k256"), ("tn", "chunked"), ("tn", "splitk"), ("nn", "n256"), ("nn", "chunked"), ("nn", "splitn"),
                     ("wgrad", "single"), ("wgrad", "split64"), ("wgrad", "split32"), ("wgrad", "grouped"), ("tn", "batched"), ("tn", "multi")}
    for c in CASES:                                            # the dispatch conditions of smallgemm.hip, restated
        n = SC.contraction(c)
        if c.form in ("k256", "n256", "batched", "multi"):
            assert n <= 256 and n % 64 == 0
        if c.form == "chunked":
            assert n > 256 and n % 64 == 0 and n % 256 != 0     # a multiple of 256 would go to the split form in functions/smallgemm.py
        if c.form in ("splitk", "splitn"):
            assert n >= 512 and n % 256 == 0
        if c.form == "split64":
            assert c.N % 64 == 0
        if c.form == "split32":
            assert c.N % 64 != 0
        assert c.N % 4 == 0 and c.K % 4 == 0
    assert {SC.contraction(c) // 64 % 2 for c in SC.TN if c.form == "chunked"} == {0, 1}     # an odd and an even chunk count
    assert len({c.seed for c in SC.TN + SC.NN + SC.WGRAD + SC.WGRAD_SPLIT + SC.GROUPED_SMALL + SC.BATCHED + SC.MULTI}) == \
        len(SC.TN + SC.NN + SC.WGRAD + SC.WGRAD_SPLIT + SC.GROUPED_SMALL + SC.BATCHED + SC.MULTI)
    assert len(SC.GROUPED_SMALL) == 130 and len(SC.MULTI) == 4


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_is_exact_in_fp32_and_its_operands_are_bf16(c):
    assert SC.magnitude(c) < SC.EXACT_LIMIT
    for t in _operands(c):
        assert t.dtype == torch.bfloat16
        assert torch.equal(t.double().bfloat16().double(), t.double()) and torch.equal(t.double(), t.double().round())
        assert not ((t != 0) & (t.double().abs() < 2.0 ** -126)).any()            # no subnormals
    for ref in _refs(c).values():                                                   # integers below 2^24: float() loses nothing
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max() if ref.numel() else 0) < SC.EXACT_LIMIT
        assert not (ref == 0).logical_and(torch.signbit(ref)).any()                # zeros are +0.0, like an accumulator that started there
    if c.kind == "nn":
        h = SC.nn_operands(c)[3]
        z = h == 0
        assert (z & torch.signbit(h)).any() and (z & ~torch.signbit(h)).any() and (h > 0).any() and (h < 0).any()


@pytest.mark.parametrize("c", [c for c in CASES if c.M > 0 and SC.contraction(c) >= 64 and (c.M, c.N, c.K) not in SC.INDEXING_ONLY],
                         ids=lambda c: SC.case_id(c))
def test_case_rounds_and_ties_often_enough(c):
    """at least 5 % of the outputs are changed by the rounding and at least 5 % are exact ties — of the plain product and of the product
    plus bias / base (the variants no ReLU or mask thins out)"""
    refs = _refs(c)
    for key in (["dw"] if c.kind == "wgrad" else [(False, False), (True, False)]):
        ref = refs[key]
        rounded, ties = SC.is_rounded(ref).double().mean().item(), SC.is_tie(ref).double().mean().item()
        print(f"{SC.case_id(c)} {key}: rounded {rounded:.3f} ties {ties:.3f}")
        assert rounded >= 0.05 and ties >= 0.05, (key, rounded, ties)


def _differs(a, b):
    return not torch.equal(SC.bits(a), SC.bits(b))


@pytest.mark.parametrize("c", [c for c in CASES if c.M > 0], ids=lambda c: SC.case_id(c))
def test_planted_defects_change_the_expected_bits(c):
    refs = _refs(c)
    plain = refs["dw"] if c.kind == "wgrad" else refs[(False, False)]
    want = SC.expected(plain)
    last = SC.contraction(c) - 1
    for j in (0, last):
        assert _differs(SC.expected(plain - _one_element(c, j)), want), f"dropping contraction element {j} goes unnoticed"
        assert _differs(SC.expected(plain + _one_element(c, j)), want), f"counting contraction element {j} twice goes unnoticed"
    if (c.M, c.N, c.K) not in SC.INDEXING_ONLY and SC.contraction(c) >= 64:
        for ref in refs.values():                              # every variant the GPU test runs has outputs that tell the roundings apart
            assert _differs(SC.truncated(ref), SC.expected(ref)), "truncation goes unnoticed"
            assert _differs(SC.half_away(ref), SC.expected(ref)), "round-half-away goes unnoticed"
    if c.kind == "tn":
        x, w, b = SC.tn_operands(c)
        for relu in (False, True):
            late = SC.expected(SC.expected(plain).double() + b.double())
            assert _differs(late.relu() if relu else late, SC.expected(refs[(True, relu)])), "a bias added after the rounding goes unnoticed"
    if c.kind == "nn":
        dy, w, base, h = SC.nn_operands(c)
        for acc in (False, True):
            assert _differs(SC.expected(SC.ref_nn(dy, w, base if acc else None, h, mask_ge=True)), SC.expected(refs[(acc, True)])), \
                "a ReLU mask taken as >= 0 goes unnoticed"
    if c.kind == "wgrad":
        dy, _ = SC.wgrad_operands(c)
        assert not torch.equal(SC.ref_db(dy[:last]), SC.ref_db(dy)), "a dropped row goes unnoticed in dB"


def test_wrong_roundings_are_what_they_claim():
    v = torch.tensor([257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 3.0, 513.0, 514.0, 518.0], dtype=torch.float64)
    assert SC.expected(v).tolist() == [256.0, 258.0, 260.0, 260.0, -256.0, -260.0, 3.0, 512.0, 512.0, 520.0]
    assert SC.truncated(v).tolist() == [256.0, 258.0, 258.0, 260.0, -256.0, -258.0, 3.0, 512.0, 512.0, 516.0]
    assert SC.half_away(v).tolist() == [258.0, 258.0, 260.0, 262.0, -258.0, -260.0, 3.0, 512.0, 516.0, 520.0]
    assert SC.is_tie(v).tolist() == [True, False, True, True, True, True, False, False, True, True]


def test_guarded_buffer_layout():
    g = SC.Guarded(5, 12, torch.bfloat16, SC.NAN16, "cpu", pad=16, batch=3, gap=8)
    assert g.ld == 32 and g.ld % 8 == 0 and g.ld > 12 and g.stride == 13 * 32 and g.ptr % 16 == 0
    assert all(w.shape == (5, 12) and w.stride() == (32, 1) and w.dtype == torch.bfloat16 for w in g.w)
    assert g.w[1].data_ptr() - g.w[0].data_ptr() == g.stride * 2 and g.w[0].data_ptr() == g.ptr
    assert torch.isnan(g.raw.view(torch.bfloat16)).all() and g.intact()
    assert g.raw.numel() >= 64 + (3 * 13 + 32) * 32
    for w in g.w:
        w.fill_(1.0)
    assert g.intact() and int((g.raw.view(torch.bfloat16) == 1).sum()) == 3 * 5 * 12
    snap = g.snapshot()
    for off in (0, 63, 64 + 12, 64 + 5 * 32, g.raw.numel() - 1):      # front guard, row padding, the gap after a window, the tail
        g.raw[off] = 0
        assert not g.intact() and not g.same_as(snap)
        g.raw[off] = g.fill
    assert g.intact() and g.same_as(snap)
    f = SC.Guarded(1, 9, torch.float32, SC.SENTINEL32, "cpu")
    assert f.ptr % 16 == 0 and f.t.shape == (1, 9) and f.intact() and int(f.raw[0]) == SC.SENTINEL32
    f.raw[64 + 9] = 0
    assert not f.intact()
    z = SC.Guarded(0, 64, torch.bfloat16, SC.SENTINEL16, "cpu")
    assert z.t.shape == (0, 64) and z.intact() and bool(z.outside.all())
