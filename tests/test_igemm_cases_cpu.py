"""The cases of tests/igemm_cases.py are what they claim: exact in fp32 in any summation order, rounded and tied often enough that a
bit-for-bit pass says something about the one fp32 -> bf16 rounding, clamped / masked often enough for the ReLU and the gates, and
sensitive to the defects a tolerance of 1e-2 of the tensor's maximum hides (one tap, one K-step, one parity, one border row, one
addend, one 64-row stage) — so that a pass of tests/test_igemm_exact_gpu.py means the kernels computed the right thing."""
import functools
import itertools

import pytest
import torch

import igemm_cases as IC
import smallgemm_cases as SC

GEOS = IC.all_geos()
GEO_IDS = [g.name + f"-{g.seed}" for g in GEOS]


@functools.lru_cache(maxsize=None)
def _conv(g):
    src, w, wk = IC.conv_operands(g)
    return src, w, wk, IC.ref_conv(g, src, w)


def _differs(a, b):
    return not torch.equal(SC.bits(SC.expected(a)), SC.bits(SC.expected(b)))


def _met(g):
    """results that receive at least one product (a stride-2 1 x 1 input gradient leaves three pixels of four empty: only addends land there)"""
    src, _, wk, _ = _conv(g)
    return IC.gemm_view(g, src, wk, absolute=True) > 0


# ------------------------------------------------------------------------------------------------ the tables
def test_the_tables_hold_the_shapes_the_issue_names():
    assert [(g.H, g.ci, g.co) for g in IC.PLAIN] == [(1, 64, 64), (127, 128, 64), (130, 192, 128), (257, 320, 192), (130, 64, 256)]
    assert {IC.contraction(g) // IC.KSTEP for g in IC.PLAIN} == {1, 2, 3, 5}
    assert [len(IC.plain_schedules(g)) for g in IC.PLAIN] == [3, 3, 6, 3, 6]
    assert {-(-IC.rows_of(g) // IC.BM) * (g.co // 64) % 8 for g in IC.PLAIN} != {0}          # workgroup counts that are no multiples of 8
    for g, knobs, splits in IC.SPLIT:
        kt = IC.contraction(g) // IC.KSTEP
        want = knobs.get("ig_splits", 2)
        per = -(-kt // min(want, kt))
        assert -(-kt // per) == splits
    assert {(g.H, g.W, g.k, g.stride) for g in IC.FWD} == {(9, 11, 3, 2), (10, 12, 3, 2), (9, 11, 1, 2), (10, 12, 1, 2), (9, 17, 3, 1)}
    assert {(g.ci, g.co) for g in IC.FWD} == {(64, 64), (128, 128)} and all(g.B == 2 and not g.dgrad for g in IC.FWD)
    assert [(g.H, g.W, g.k, g.stride) for g in IC.DGRAD] == [(9, 11, 1, 1), (9, 11, 1, 2), (10, 12, 1, 2), (9, 11, 3, 2), (10, 12, 3, 2), (9, 17, 3, 1)]
    assert all(g.dgrad for g in IC.DGRAD + IC.PCLS)
    assert [(g.B, g.H, g.W) for g in IC.PCLS] == [(2, 10, 18), (1, 24, 24)] and [IC.rows_of(g) // 4 for g in IC.PCLS] == [90, 144]
    assert len(IC.PATCH) == 16 and {((f.B, f.H, f.W), f.ci) for f, _ in IC.PATCH} == set(itertools.product(IC.PATCH_GRIDS, (64, 128, 192, 320)))
    assert {(f.B, f.H, f.W) for f, _ in IC.PATCH} == set(IC.PATCH_GRIDS) and {f.ci for f, _ in IC.PATCH} == {64, 128, 192, 320} == {b.co for _, b in IC.PATCH}
    for f, b in IC.PATCH:
        assert (f.k, f.stride, f.dgrad, b.k, b.stride, b.dgrad) == (3, 1, 0, 3, 1, 1) and IC.dims(f)["cs"] == IC.dims(b)["cs"]
        assert IC.dims(f)["n"] in (64, 128) and IC.dims(b)["n"] in (64, 128)
    for grid in IC.PATCH_GRIDS:                                  # both widths of n with every grid and every channel count
        assert {f.co for f, _ in IC.PATCH if (f.B, f.H, f.W) == grid} == {64, 128}
    for cs in (64, 128, 192, 320):
        assert {f.co for f, _ in IC.PATCH if f.ci == cs} == {64, 128}
    for cs, forced, chunks in IC.PATCH_SPLIT:
        cch = cs // 64
        per = -(-cch // min(forced, cch))
        assert tuple(min(per, cch - i * per) for i in range(-(-cch // per))) == chunks
    assert IC.TRANSPOSES == [(64, 9, 192, True), (192, 1, 64, False), (128, 9, 64, True), (64, 1, 64, False)]
    assert [(c.M, c.N, c.K) for c in IC.WGRAD] == [(1, 8, 8), (63, 72, 136), (65, 136, 72), (129, 264, 8), (257, 64, 264)]
    assert [IC.wg_plan(IC.WGRAD[4], s) for s in IC.WG_SPLITS] == [(1, 320), (2, 192), (3, 128), (5, 64)]      # 7 slices collapse onto the 5 stages
    assert [IC.wg_plan(IC.WGRAD[0], s)[0] for s in IC.WG_SPLITS] == [1, 1, 1, 1]
    sliced = [IC.wg_plan(c, IC.WGRAD_SEQ_SPLITS)[0] > 1 for c, _ in IC.WGRAD_SEQ]
    assert len(IC.WGRAD_SEQ) == 5 and any(sliced) and not all(sliced) and {f for _, f in IC.WGRAD_SEQ} == {True, False}
    seeds = [g.seed for g in GEOS] + [c.seed for c in IC.WGRAD] + [c.seed for c, _ in IC.WGRAD_SEQ]
    assert len(seeds) == len(set(seeds))


def test_every_epilogue_option_meets_every_other():
    assert 10 <= len(IC.EPILOGUES) <= 16 and len(set(IC.EPILOGUES)) == len(IC.EPILOGUES)
    options = set().union(*(IC.epi_options(e) for e in IC.EPILOGUES))
    assert options == {"scale", "bias_f32", "bias_bf16", "res_dense", "res_up2", "res2", "pre", "act_relu", "act_gelu", "gate_relu", "gate_gelu"}
    missing = [p for p in itertools.combinations(sorted(options), 2) if set(p) not in IC.EXCLUSIVE
               and not any(set(p) <= IC.epi_options(e) for e in IC.EPILOGUES)]
    assert not missing, missing
    for o in options:                                          # ... and every option is also absent somewhere, and on alone-ish (at most two others)
        assert any(o not in IC.epi_options(e) for e in IC.EPILOGUES)
    for _, g, even, _ in IC.EPI_BASES:
        d = IC.dims(even)
        assert d["ho"] % 2 == 0 and d["wo"] % 2 == 0 and (IC.dims(g)["cs"], IC.dims(g)["n"]) == (d["cs"], d["n"])


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("g", GEOS, ids=GEO_IDS)
def test_case_is_exact_in_fp32_and_its_operands_are_bf16(g):
    src, w, wk, ref = _conv(g)
    assert IC.magnitude(g) < SC.EXACT_LIMIT
    for t in (src, w, wk):
        assert t.dtype == torch.bfloat16 and torch.equal(t.double(), t.double().round()) and float(t.double().abs().max()) <= SC.OPERAND
    assert torch.equal(ref.float().double(), ref) and not (ref == 0).logical_and(torch.signbit(ref)).any()
    assert torch.equal(IC.gemm_view(g, src, wk), ref), "the tap-by-tap GEMM view and F.conv2d / its autograd disagree"


@pytest.mark.parametrize("e", IC.EPILOGUES, ids=IC.epi_id)
@pytest.mark.parametrize("base", IC.EPI_BASES, ids=lambda b: b[0])
def test_epilogue_operands_are_exact_and_clamp_and_mask_often_enough(base, e):
    g = IC.epi_geo(base, e)
    _, _, _, acc = _conv(g)
    o = IC.epi_operands(g, e)
    for name, t in o.items():
        assert torch.equal(t.double().bfloat16().double(), t.double()), name           # every addend and factor is a bf16 value
        bound = 2 if name == "scale" else 3 if name == "gate" else SC.ADDEND
        assert float(t.double().abs().max()) <= bound
    if e.scale:
        assert set(o["scale"].tolist()) <= set(IC.SCALES) and len(set(o["scale"].tolist())) >= 4
    r = IC.ref_epilogue(g, e, acc, o)
    assert torch.equal(r["pre"].float().double(), r["pre"]) and float(r["pre"].abs().max()) < SC.EXACT_LIMIT
    if IC.is_exact(e):
        assert torch.equal(r["out"].float().double(), r["out"])
        assert not (r["out"] == 0).logical_and(torch.signbit(r["out"])).any()
    if e.act == IC.ACT_RELU:
        clamped = (r["pre"] < 0).double().mean().item()
        assert clamped >= 0.05, clamped
    if e.gate:
        h = o["gate"]
        z = h == 0
        assert (z & torch.signbit(h)).any() and (z & ~torch.signbit(h)).any() and (h > 0).any() and (h < 0).any()
    if e.gate == IC.GATE_RELU:
        masked = (o["gate"].double() <= 0).double().mean().item()
        assert masked >= 0.05, masked
    if e.act == IC.ACT_GELU:                                   # some pre-activations lie where the GELU is neither 0 nor x
        assert int(((r["pre"].abs() < 4) & (r["pre"] != 0)).sum()) >= 16


@pytest.mark.parametrize("g", [g for g in GEOS if g.name not in IC.INDEXING_ONLY], ids=lambda g: g.name + f"-{g.seed}")
def test_case_rounds_and_ties_often_enough(g):
    """of the results that receive a product at all, at least a quarter are changed by the rounding and at least one is an exact tie"""
    _, _, _, ref = _conv(g)
    met = _met(g)
    rounded = SC.is_rounded(ref)[met].double().mean().item()
    ties = int(SC.is_tie(ref)[met].sum())
    print(f"{g.name}: rounded {rounded:.3f} ties {ties}")
    assert rounded >= 0.25 and ties >= 1, (rounded, ties)


def test_the_indexing_only_cases_are_the_short_contractions():
    names = {g.name: g for g in GEOS}
    for n in IC.INDEXING_ONLY:
        if n.startswith("wg"):
            c = next(c for c in IC.WGRAD if IC.wg_id(c) == n)
            assert c.M <= 64
        else:
            g = names[n]
            # (a 3 x 3 convolution of a 1 x 1 image meets its centre tap only)
            assert IC.contraction(g) <= 64 or (g.H, g.W, IC.dims(g)["cs"]) == (1, 1, 64)


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("g", GEOS, ids=GEO_IDS)
def test_planted_gather_defects_change_the_expected_bits(g):
    src, w, wk, ref = _conv(g)
    d = IC.dims(g)
    taps = g.k * g.k
    if taps == 9 and (g.H, g.W) != (1, 1):
        for tap in range(9):
            assert _differs(IC.gemm_view(g, src, wk, defect=("tap", tap)), ref), f"tap {tap} dropped goes unnoticed"
    if taps == 9 and (g.H, g.W) == (1, 1):
        assert _differs(IC.gemm_view(g, src, wk, defect=("tap", 4)), ref)
    if taps == 9 and g.dgrad and (g.H, g.W) != (1, 1):
        assert _differs(IC.gemm_view(g, src, wk, defect="noflip"), ref), "an input gradient that does not flip the taps goes unnoticed"
    if taps == 9 and g.dgrad and g.stride == 2:
        assert _differs(IC.gemm_view(g, src, wk, defect="parity"), ref), "parity taken from the wrong coordinate goes unnoticed"
    if (g.H, g.W) != (1, 1):
        assert _differs(IC.gemm_view(g, src, wk, defect="kstep"), ref), "the last K-step dropped goes unnoticed"
    assert d["cs"] % 64 == 0 and d["n"] % 64 == 0


@pytest.mark.parametrize("e", IC.EPILOGUES, ids=IC.epi_id)
@pytest.mark.parametrize("base", IC.EPI_BASES, ids=lambda b: b[0])
def test_planted_epilogue_defects_change_the_expected_bits(base, e):
    g = IC.epi_geo(base, e)
    _, _, _, acc = _conv(g)
    o = IC.epi_operands(g, e)
    want = IC.ref_epilogue(g, e, acc, o)
    applied = 0
    for defect, applies in (("res_odd", e.res == "up2"), ("no_res2", e.res2), ("gate_first", e.gate == IC.GATE_GELU and e.act != IC.ACT_NONE),
                            ("scale_after_bias", e.scale and bool(e.bias))):
        if not applies:
            continue
        applied += 1
        got = IC.ref_epilogue(g, e, acc, o, defect=defect)
        key = "pre" if defect in ("res_odd", "no_res2", "scale_after_bias") else "out"
        assert _differs(got[key], want[key]), defect
        if defect == "gate_first" or IC.is_exact(e):
            assert _differs(got["out"], want["out"]), defect
        if not IC.is_exact(e):                                   # ... and by more than the GELU tolerance lets through
            assert ((got["out"] - want["out"]).abs() > IC.gelu_bound(want["out"], want["x"])).any(), defect
    assert applied or IC.epi_options(e) <= {"bias_f32", "res_dense", "act_relu", "act_gelu", "gate_relu", "scale", "pre"}


def test_planted_slab_defect_changes_the_expected_bits():
    _, _, _, acc = _conv(IC.SLAB_GEO)
    assert _differs(IC.slabbed(acc, 128, swapped=True), IC.slabbed(acc, 128))
    assert torch.equal(IC.slabbed(acc, 256)[0], acc) and torch.equal(IC.slabbed(acc, 128)[1], acc[:, 128:])


def test_gelu_references_and_their_tolerance():
    x = torch.linspace(-9, 9, 1801, dtype=torch.float64).requires_grad_()
    y = torch.nn.functional.gelu(x)
    assert torch.allclose(IC.gelu64(x.detach()), y.detach(), rtol=0, atol=1e-14)       # (torch's 1 + erf cancels below -6; erfc does not)
    (gp,) = torch.autograd.grad(y.sum(), x)
    assert torch.allclose(IC.gelu_grad64(x.detach()), gp, rtol=0, atol=1e-14)
    assert IC.GELU_REL == 2.0 ** -8 and IC.GELU_ABS == 2e-6
    assert abs(float(IC.gelu_grad64(torch.tensor([-3.0], dtype=torch.float64))) + 0.0119) < 1e-4      # negative: "gate first" is visible under a ReLU


# ------------------------------------------------------------------------------------------------ weight gradients, transposes
@pytest.mark.parametrize("c", IC.WGRAD + [c for c, _ in IC.WGRAD_SEQ], ids=lambda c: IC.wg_id(c) + f"-{c.seed}")
def test_weight_gradient_case(c):
    dy, x, rs, base = IC.wg_operands(c)
    assert IC.wg_magnitude(c) < SC.EXACT_LIMIT
    assert c.N % 8 == 0 and c.K % 8 == 0 and set(rs.tolist()) <= set(IC.SCALES) and bool((base != 0).any())
    for scale in (None, rs):
        ref = IC.ref_wgrad(c, dy, x, scale)
        assert torch.equal(ref.float().double(), ref)
        if IC.wg_id(c) not in IC.INDEXING_ONLY:
            rounded, ties = SC.is_rounded(ref).double().mean().item(), int(SC.is_tie(ref).sum())
            print(f"{IC.wg_id(c)}: rounded {rounded:.3f} ties {ties}")
            assert rounded >= 0.25 and ties >= 1, (rounded, ties)
        for s in IC.WG_SPLITS:
            assert _differs(IC.ref_wgrad(c, dy, x, scale, drop_last_stage_of_slice=s), ref), f"the last stage of a slice dropped goes unnoticed ({s} slices)"
            assert not torch.equal(IC.ref_wgrad(c, dy, x, scale, drop_last_stage_of_slice=s).float(), ref.float())      # dw_f32 sees it too
    assert not torch.equal(IC.ref_db(dy[:-1], base), IC.ref_db(dy, base)) and not torch.equal(IC.ref_db(dy), IC.ref_db(dy, base))
    assert torch.equal(IC.ref_db(dy, base).float().double(), IC.ref_db(dy, base))


def test_transposes_are_permutations_times_the_scale():
    for i, (co, taps, ci, sc) in enumerate(IC.TRANSPOSES):
        w, s = IC.transpose_operands(i)
        r = IC.ref_transpose(w, s)
        assert r.shape == (ci, taps, co) and (s is not None) == sc
        assert torch.equal(r.double(), (w.double() * (s.double()[:, None, None] if sc else 1.0)).permute(2, 1, 0))
        if taps > 1:
            assert not torch.equal(r, IC.ref_transpose(w.flip(1), s))                # a tap order reversed is seen
        if sc:
            assert not torch.equal(r, IC.ref_transpose(w, None))
