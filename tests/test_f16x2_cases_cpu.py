"""What the exact cases of the two-plane fp16 GEMMs (tests/f16x2_cases.py) must have for a bit-for-bit comparison to mean something,
proved on the CPU for every case tests/test_f16x2_exact_gpu.py launches:

  exact split        hi + lo == x' under the scale the kernel will use (the maxima it is handed, over-stated ones included)
  exact sums         with u a power of two dividing every term of an output (bias and pre-fills included), sum |terms| / u < 2^24: every
                     partial sum, in any order, is exact in fp32; the expected value itself is an fp32 number
  both planes        the lo plane of each operand is non-zero in at least 5 % of its elements
  sensitivity        the expected value differs from the fp32 rounding of the FULL product in >= 5 % of the outputs, from hi hi alone and
                     from each sum that misses one cross product in >= 90 % (sparse mode-2 operands: of the outputs that have a term at all,
                     which are >= 25 % of all — see f16x2_cases.py for why they are sparse)
  ReLU and mask      >= 25 % of the pre-activations on each side of zero, none exactly zero
  limits             scaled maxima in [2^14, 2^15) (the rows named for the clamp excepted), every plane value inside fp16's normal range

Cases marked `indexing` (four outputs, no contraction at all, one row or five pixels of a weight gradient) are too small for the percentages:
they keep every exactness condition."""
import pytest
import torch

import f16x2_cases as FC

LIMIT = float(1 << 24)
FP16_MIN_NORMAL, FP16_MAX = 2.0 ** -14, 65504.0


def _planes_ok(x, amax_given, amax_true, special_rows=()):
    hi, lo, _ = FC.split(x, amax_given)
    assert torch.equal(hi + lo, FC.scaled(x, amax_given)), "hi + lo != x'"
    for p in (hi, lo):
        nz = p[p != 0].abs()
        assert bool(torch.isfinite(p).all())
        assert nz.numel() == 0 or (float(nz.min()) >= FP16_MIN_NORMAL and float(nz.max()) <= FP16_MAX)
    if amax_true is not None and x.shape[1]:
        top = FC.scaled(x, amax_true).abs().amax(1)
        ordinary = torch.ones(x.shape[0], dtype=torch.bool)
        for r in special_rows:
            ordinary[r] = False
        ordinary &= amax_true > 0
        assert bool(((top >= 2.0 ** 14) & (top < 2.0 ** 15))[ordinary].all())
        assert torch.equal(x.abs().amax(1), amax_true)
    return lo


def _sums_exact(a, b, aa, ba, bias, extra_rows=None):
    """sum |terms| / u < 2^24 for every output; returns (S scale, u scale) for the column sums' check"""
    pa = FC.products(a, b, aa, ba, absolute=True)
    s = (pa.hh + pa.hl + pa.lh) * pa.scale
    u = FC.term_unit(a, b, aa, ba) * pa.scale
    if bias is not None:
        s = s + bias.double().abs()
        u = torch.minimum(u, FC.lowbit(bias.double())[None, :])
    assert bool((s / u < LIMIT).all()), float((s / u).max()) / LIMIT
    return s, u


def _differs(x, y, where=None):
    d = x != y
    return float((d[where] if where is not None else d).double().mean())


def _sensitive(p, bias, where=None):
    three = FC.finish(p.hh + p.hl + p.lh, p.scale, bias)
    full = FC.finish(p.hh + p.hl + p.lh + p.ll, p.scale, bias).float().double()
    assert _differs(three, full, where) >= 0.05, _differs(three, full, where)
    for name, wrong in (("hi hi alone", p.hh), ("no hi lo", p.hh + p.lh), ("no lo hi", p.hh + p.hl)):
        assert _differs(three, FC.finish(wrong, p.scale, bias), where) >= 0.90, (name, _differs(three, FC.finish(wrong, p.scale, bias), where))


def _relu_ok(pre):
    assert not bool((pre == 0).any())
    assert float((pre > 0).double().mean()) >= 0.25 and float((pre < 0).double().mean()) >= 0.25


@pytest.mark.parametrize("c", FC.ALL_TN, ids=FC.tn_id)
def test_tn_case_is_exact_and_sensitive(c):
    a, b, bias = FC.tn_operands(c)
    aa, ba = FC.tn_maxima(c, a, b)
    special = (1,) if c.special else ()
    lo_a = _planes_ok(a.x, aa, a.amax if aa is not None else None, special)
    lo_b = _planes_ok(b.x, ba, b.amax if ba is not None else None)
    if aa is None and c.K:                                          # an operand without maxima is O(1): already in the scaled form
        assert bool(((a.amax >= 2.0 ** 14) & (a.amax < 2.0 ** 15)).all())
    if ba is None and c.K:
        assert bool(((b.amax >= 2.0 ** 14) & (b.amax < 2.0 ** 15)).all())
    _sums_exact(a.x, b.x, aa, ba, bias)
    p = FC.products(a.x, b.x, aa, ba)
    pre = FC.finish(p.hh + p.hl + p.lh, p.scale, bias)
    assert FC.exact_in_fp32(pre)
    assert torch.equal(pre, FC.ref_tn(a.x, b.x, aa, ba, bias))
    if c.special:                                                    # the clamped row is there, and its results are ordinary fp32 numbers
        e = int((a.amax[1:2].view(torch.int32) >> 23) & 0xFF)
        assert e == (15 if c.special == "tiny" else 251)
        assert bool((pre[1] != 0).any()) and float(pre[1].abs()[pre[1] != 0].min()) >= 2.0 ** -126
        if c.special == "tiny":
            assert not bool(pre[0].any())
    if c.indexing:
        return
    assert float((lo_a != 0).double().mean()) >= 0.05 and float((lo_b != 0).double().mean()) >= 0.05
    _sensitive(p, bias)
    if c.mode == 1:
        _relu_ok(pre)


def test_row_scale_is_the_headers():
    """row_scale: e clamped to [20, 250], s = 2^(141 - e), inv = 2^(e - 141); the unit scale at e = 141"""
    amax = torch.tensor([0.0, 2.0 ** -120, 2.0 ** -107, 1.0, 24578.0, 2.0 ** 15, 1.5 * 2.0 ** 123, 2.0 ** 127])
    s, inv = FC.row_scale(amax)
    want = [20, 20, 20, 127, 141, 142, 250, 250]
    assert s.tolist() == [2.0 ** (141 - e) for e in want]
    assert inv.tolist() == [2.0 ** (e - 141) for e in want]


@pytest.mark.parametrize("p, maxima", [(p, True) for p in FC.ALL_PAIRS] + [(FC.BITS_CONTRACT, False)],
                         ids=lambda v: f"{v.M}x{v.N}x{v.K}" if isinstance(v, FC.Pair) else ("maxima" if v else "o1"))
def test_relu_pair_is_exact_and_sensitive(p, maxima):
    a1, b1, bias1, a2, b2, prefill = FC.pair_operands(p, maxima)

    def mx(op):
        return op.amax if maxima else None
    # the forward launch: dense, no pre-activation is zero
    for op in (a1, b1):
        lo = _planes_ok(op.x, mx(op), op.amax)
        assert float((lo != 0).double().mean()) >= 0.05
    _sums_exact(a1.x, b1.x, mx(a1), mx(b1), bias1)
    p1 = FC.products(a1.x, b1.x, mx(a1), mx(b1))
    pre = FC.finish(p1.hh + p1.hl + p1.lh, p1.scale, bias1)
    assert FC.exact_in_fp32(pre)
    _relu_ok(pre)
    _sensitive(p1, bias1)
    # the masked launch: sparse, exact down to the column sums over all rows
    for op in (a2, b2):
        lo = _planes_ok(op.x, mx(op), op.amax)
        assert float((lo != 0).double().mean()) >= 0.05
    s, u = _sums_exact(a2.x, b2.x, mx(a2), mx(b2), None)
    kept = pre > 0
    cu = torch.minimum(u.amin(0), FC.lowbit(prefill.double()))
    cs = (s * kept).sum(0) + prefill.double().abs()
    assert bool((cs / cu < LIMIT).all()), float((cs / cu).max()) / LIMIT
    ref, colsum = FC.ref_masked(a2.x, b2.x, mx(a2), mx(b2), pre, prefill)
    assert FC.exact_in_fp32(ref) and FC.exact_in_fp32(colsum)
    p2 = FC.products(a2.x, b2.x, mx(a2), mx(b2))
    some = s > 0
    assert float(some.double().mean()) >= 0.25
    _sensitive(p2, None, some)
    assert float((ref != 0).double().mean()) >= 0.10                # the mask's order shows on every one of these


def test_operands_without_maxima_equal_those_with_them_up_to_the_row_powers():
    """r only moves the exponent: the planes of a scaled row are those of the O(1) row"""
    c = FC.TILE128[2]
    a, _, _ = FC.tn_operands(c)
    a0 = FC.operand(c.M, c.K, c.seed, c.d, r=0, **FC.DENSE)
    h, l, _ = FC.split(a.x, a.amax)
    h0, l0, _ = FC.split(a0.x, None)
    assert torch.equal(h, h0) and torch.equal(l, l0)


def test_amax_and_cast_cases_have_the_edges():
    for rows, cols, ld, off in FC.ROW_AMAX:
        assert ld >= cols and off in (1, 4)
    assert any(off == 1 for *_, off in FC.ROW_AMAX) and any(ld % 4 for _, _, ld, _ in FC.ROW_AMAX)
    assert all(cols % 8 == 0 for _, cols in FC.CAST_AMAX)


@pytest.mark.parametrize("c", FC.ALL_WG, ids=FC.wg_id)
def test_wgrad_case_is_exact_and_sensitive(c):
    dy, x, ya, xa, dw0, db0 = FC.wg_operands(c)
    _wgrad_conditions(dy, x, ya, xa, dw0, db0, c.indexing)


@pytest.mark.parametrize("c", FC.CONV_WGRAD, ids=FC.conv_wg_id)
def test_conv_wgrad_case_is_exact_and_sensitive(c):
    """the second operand is the matrix of patches: the same conditions on it"""
    dy, x, ya, xa, dw0, db0 = FC.conv_wg_operands(c)
    _planes_ok(x.x, xa, x.amax)
    px = FC.patches(c, x.x)
    _wgrad_conditions(dy, FC.Op(px, x.amax), ya, xa, dw0, db0, c.indexing, patch_rows=True)
    wrong = FC.ref_wgrad(dy.x, FC.patches(c, x.x, into_next_image=True), ya, xa, dw0)
    assert float((wrong != FC.ref_wgrad(dy.x, px, ya, xa, dw0)).double().mean()) >= 0.1


def _wgrad_conditions(dy, x, ya, xa, dw0, db0, indexing_only, patch_rows=False):
    lo_y = _planes_ok(dy.x, ya, dy.amax)
    lo_x = _planes_ok(x.x, xa, None if patch_rows else x.amax)
    for op, am in ((dy, ya), (x, xa)):
        assert bool((op.amax == op.amax[0]).all())                  # one power of two per operand
        if am is None:
            assert bool(((op.amax >= 2.0 ** 14) & (op.amax < 2.0 ** 15)).all())
    # the whole contraction over the rows, the pre-fill included
    pa = FC.wg_products(dy.x, x.x, ya, xa, absolute=True)
    hy, ly, _ = FC.split(dy.x, ya)
    hx, lx, _ = FC.split(x.x, xa)
    uhy, uly, uhx, ulx = FC.row_unit(hy.t()), FC.row_unit(ly.t()), FC.row_unit(hx.t()), FC.row_unit(lx.t())
    u = torch.minimum(uhy[:, None] * uhx[None, :], torch.minimum(uhy[:, None] * ulx[None, :], uly[:, None] * uhx[None, :])) * pa.scale
    u = torch.minimum(u, FC.lowbit(dw0.double()))
    s = (pa.hh + pa.hl + pa.lh) * pa.scale + dw0.double().abs()
    assert bool((s / u < LIMIT).all()), float((s / u).max()) / LIMIT
    ub = torch.minimum(FC.row_unit(dy.x.double().t()), FC.lowbit(db0.double()))
    sb = dy.x.double().abs().sum(0) + db0.double().abs()
    assert bool((sb / ub < LIMIT).all()), float((sb / ub).max()) / LIMIT
    assert FC.exact_in_fp32(FC.ref_wgrad(dy.x, x.x, ya, xa, dw0)) and FC.exact_in_fp32(FC.ref_db(dy.x, db0))
    assert bool((dw0 != 0).double().mean() > 0.9) and bool((db0 != 0).double().mean() > 0.9)
    if indexing_only:
        return
    assert float((lo_y != 0).double().mean()) >= 0.05 and float((lo_x != 0).double().mean()) >= 0.05
    _sensitive(FC.wg_products(dy.x, x.x, ya, xa)._replace(scale=pa.scale), dw0)


@pytest.mark.parametrize("c", FC.CONV, ids=FC.conv_id)
def test_conv_case_is_exact_and_sensitive(c):
    x, w, bias = FC.conv_operands(c)
    has_x, has_w = c.amax in ("both", "x"), c.amax in ("both", "w")
    a = FC.patches(c, x.x)
    assert a.shape == (c.B * c.H * c.W, 9 * c.Ci)
    true_a = FC.patch_maxima(c, x.amax)
    assert torch.equal(a.abs().amax(1), true_a)                     # (the pixel itself is always inside)
    aa, wa = (true_a if has_x else None), (w.amax if has_w else None)
    lo_a = _planes_ok(a, aa, true_a)
    lo_w = _planes_ok(w.x, wa, w.amax)
    _sums_exact(a, w.x, aa, wa, bias)
    p = FC.products(a, w.x, aa, wa)
    ref = FC.finish(p.hh + p.hl + p.lh, p.scale, bias)
    assert FC.exact_in_fp32(ref)
    assert float((lo_a != 0).double().mean()) >= 0.05 and float((lo_w != 0).double().mean()) >= 0.05
    _sensitive(p, bias)
    if has_x:                                                       # magnitudes differ inside a neighbourhood
        assert float((true_a != x.amax).double().mean()) >= 0.25
    # a tap that crosses an image border or a row end is a wrong value
    wrong = FC.ref_tn(FC.patches(c, x.x, into_next_image=True), w.x, aa, wa, bias)
    differs = (wrong != ref).any(1)
    assert float(differs.double().mean()) >= 0.1
    if c.B > 1:                                                     # the last pixel of an image and the first of the next
        assert bool(differs[c.H * c.W - 1]) and bool(differs[c.H * c.W])


def test_conv_input_gradient_case_is_the_gradient():
    """the product of dY's patches with CONV_DGRAD's filter is autograd's input gradient of the forward convolution (float64, exact)"""
    import torch.nn.functional as F
    c = FC.CONV_DGRAD
    dy, wk, _ = FC.conv_operands(c)
    got = FC.patches(c, dy.x.double()) @ wk.x.double().t()                                   # [B H W, 32]
    wf = FC.forward_filter(c, wk.x.double())                                                 # [48][3][3][32]
    x = torch.zeros((c.B, c.Co, c.H, c.W), dtype=torch.float64, requires_grad=True)
    (grad,) = torch.autograd.grad(F.conv2d(x, wf.permute(0, 3, 1, 2), None, 1, 1), x, dy.x.double().view(c.B, c.H, c.W, c.Ci).permute(0, 3, 1, 2))
    assert torch.equal(got, grad.permute(0, 2, 3, 1).reshape(-1, c.Co))
