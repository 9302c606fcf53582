"""tests/window_attention_cases.py is what tests/test_window_attention_edges_gpu.py takes it for: its oracle equals fp64 autograd of the plain
restatement of the reference's WindowAttention body, the index formula of include/pd_window_attention.h and the region labels of
functions/window_attention.py equal the reference's index and mask, the per-element bounds can be met (the oracle's math with the kernels'
documented roundings inserted stays inside them at exactly the inputs the GPU sees), and every named case has the property it is named for."""
import functools

import pytest
import torch

import window_attention_cases as WC
from test_window_attention_gpu import _ref, _reference_mask, _relative_position_index

N = WC.N


@functools.lru_cache(maxsize=None)
def _case(name):
    case = WC.build(name)
    return case, WC.oracle_of(case)


@pytest.mark.parametrize("name", ["one_window", "mixed_flags", "chunk_masked", "wide_masked"])
def test_oracle_equals_autograd_of_the_plain_restatement(name):
    """`_ref` of tests/test_window_attention_gpu.py run in float64, its gradients from autograd"""
    case, ref = _case(name)
    qkv = case["qkv"].double().requires_grad_()
    table = case["table"].double().requires_grad_()
    mask = _reference_mask(case["H"], case["W"], case["shift"]).double() if case["shift"] else None
    out = _ref(qkv, table, mask, case["heads"], case["scale"])
    dqkv, dtable = torch.autograd.grad(out, (qkv, table), case["d_out"].double())
    for got, want in zip((ref["out"], ref["dt"]) + (ref["dq"], ref["dk"], ref["dv"]), (out.detach(), dtable) + tuple(WC.split_dqkv(dqkv))):
        assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item())
    q, k, v, raw, m, _ = WC.scores(case["qkv"], case["table"], case["H"], case["W"], case["shift"], case["scale"])
    assert torch.equal(ref["lse"], torch.logsumexp(raw + m, -1) * WC.LOG2E) and ref["lse"].shape == (qkv.shape[0], case["heads"], N)


def test_relative_position_index_is_the_header_formula():
    """include/pd_window_attention.h: index(q, key) = A(q) - A(key) + 264, A(t) = t + 11 * (t / 12) — all 144^2 pairs"""
    t = torch.arange(N)
    a = t + 11 * (t // 12)
    idx = WC.relative_position_index()
    assert torch.equal(idx, a[:, None] - a[None, :] + 264)
    assert torch.equal(idx, _relative_position_index()) and idx.min() == 0 and idx.max() == WC.TBL - 1
    assert torch.equal(torch.bincount(idx.view(-1), minlength=WC.TBL)[[0, 22, 506, 528, 264]], torch.tensor([1, 1, 1, 1, 144]))


@pytest.mark.parametrize("H,W", [(12, 12), (24, 24), (30, 30), (25, 40), (13, 12), (36, 24)])
def test_regions_and_flags_are_the_reference_mask(H, W):
    from partdistillation_amd.functions import window_attention as wa
    reg, flags = wa.shifted_window_regions(H, W, 6, "cpu")
    mask = WC.reference_mask(H, W, 6)
    assert reg.shape == (WC.n_windows(H, W), N) and reg.dtype == torch.uint8 and flags.dtype == torch.uint8
    assert torch.equal((reg[:, :, None] != reg[:, None, :]).double() * -100.0, mask)
    assert torch.equal(mask, _reference_mask(H, W, 6).double())
    assert torch.equal(flags.bool(), (mask != 0).flatten(1).any(1))


@pytest.mark.parametrize("name", list(WC.CASES))
def test_the_bounds_can_be_met(name):
    """the rounding emulation against the oracle: ratio error / bound <= 1 for every element of every tensor"""
    case, ref = _case(name)
    emu = WC.emulate(case["qkv"], case["table"], case["d_out"], case["H"], case["W"], case["shift"], case["scale"])
    r = WC.ratios(emu, ref)
    print(name, {n: round(x, 3) for n, x in r.items()})
    assert all(x <= 1.0 for x in r.values()), r
    for n, b in WC.bounds(ref).items():                           # and the bounds are per element: the smallest is far below the old per-tensor one
        assert b.shape == ref[n].shape and (b > 0).all()


@pytest.mark.parametrize("name", ["one_window", "bias_only_plain", "bias_only_shifted"])
def test_the_bounds_see_table_entries_missing_from_the_reduction(name):
    """a table-gradient reduction that skips the entries with |dc| = 11, or those with |dr| = 11 (t = 23 (dr + 11) + dc + 11) — 46 entries
    each, fed by 1 .. 12 pairs per window, the four corners by one — is far outside the per-element bound, in nearly every such entry"""
    case, ref = _case(name)
    b = WC.bounds(ref)["dt"]
    t = torch.arange(WC.TBL)
    for lost in ((t % 23 == 0) | (t % 23 == 22), (t // 23 == 0) | (t // 23 == 22)):
        assert int(lost.sum()) == 46
        err = ref["dt"][lost].abs()
        got = dict(ref, dt=torch.where(lost[:, None], torch.zeros_like(ref["dt"]), ref["dt"]))
        assert WC.ratios(got, ref)["dt"] > 10.0 and ((err / b[lost]) > 1.0).float().mean() > 0.9


def test_wide_masked_needs_the_additive_mask():
    case, ref = _case("wide_masked")
    hard = WC.oracle_of(case, mask_value=float("-inf"))
    _, _, _, raw, m, _ = WC.scores(case["qkv"], case["table"], case["H"], case["W"], case["shift"], case["scale"])
    rows = WC.wide_rows(case["heads"])
    flagged = [w for w in range(case["nW"]) if (m[w] != 0).any()]
    assert sorted({w for w, _, _, _ in rows}) == flagged and len(flagged) == 3 and len(rows) == 3 * case["heads"]
    bound = WC.bounds(ref)["out"]
    for w, h, i, j in rows:
        same = m[w, 0, i] == 0
        assert not same[j] and same[i]
        assert raw[w, h, i, j] > raw[w, h, i][same].max() + 100.0                         # the cross-region key wins even after -100 ...
        cols = slice(h * WC.D, (h + 1) * WC.D)
        diff = (ref["out"][w, i, cols] - hard["out"][w, i, cols]).abs()
        assert (diff > bound[w, i, cols]).any() and diff.max() > 100 * bound[w, i, cols].max()       # ... so -inf gives another answer
    assert ref["lse"].abs().max() > 150


def test_peaky_has_large_lse_and_near_one_hot_rows():
    case, ref = _case("peaky")
    _, _, _, raw, m, _ = WC.scores(case["qkv"], case["table"], case["H"], case["W"], case["shift"], case["scale"])
    top = torch.softmax(raw + m, -1).amax(-1)
    assert ref["lse"].abs().max() > 150 and (top > 0.999).any()
    assert (top > 0.999).float().mean() > 0.25 and (top < 0.9).any()                      # many such rows, and not all of them


@pytest.mark.parametrize("name", ["bias_only_plain", "bias_only_shifted"])
def test_bias_only_scores_are_the_table(name):
    case, ref = _case(name)
    C = case["heads"] * WC.D
    assert (case["qkv"][:, :, :2 * C] == 0).all() and (case["qkv"][:, :, 2 * C:] != 0).any()
    _, _, _, raw, _, _ = WC.scores(case["qkv"], case["table"], case["H"], case["W"], case["shift"], case["scale"])
    want = case["table"].double()[WC.relative_position_index().view(-1)].view(N, N, -1).permute(2, 0, 1)
    assert torch.equal(raw, want.unsqueeze(0).expand_as(raw))
    assert (ref["dq"] == 0).all() and (ref["dk"] == 0).all() and ref["dt"].abs().min() > 0


def test_mixed_flags_has_both_kinds_of_window():
    from partdistillation_amd.functions import window_attention as wa
    case, _ = _case("mixed_flags")
    flags = wa.shifted_window_regions(case["H"], case["W"], case["shift"], "cpu")[1]
    assert flags.tolist() == [0, 1, 1, 1] and case["qkv"].shape[0] == 4
    case, _ = _case("chunk_masked")                               # the chunk sweep: chunks of 2, 3, 5 and 8 straddle images and mix flags
    assert case["qkv"].shape[0] == 12 and case["nW"] == 4
    assert _case("chunk_plain")[0]["qkv"].shape[0] == 7 and _case("chunk_plain")[0]["nW"] == 1


def test_cases_are_bf16_valued_and_deterministic():
    for name in WC.CASES:
        a, b = WC.build(name), WC.build(name)
        assert a["qkv"].dtype == torch.bfloat16 and a["d_out"].dtype == torch.bfloat16 and a["table"].dtype == torch.float32
        assert all(torch.equal(a[n], b[n]) for n in ("qkv", "table", "d_out"))
        assert a["qkv"].shape == (a["images"] * a["nW"], N, 3 * a["heads"] * WC.D) and a["qkv"].is_contiguous()
