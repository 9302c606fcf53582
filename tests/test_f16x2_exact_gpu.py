"""The two-plane fp16 GEMMs, convolution and weight gradients (include/pd_gemm.h, csrc/gemm_f16x2.hip, the H2 kernels of csrc/gemm_x3.hip) through the C-ABI on the exact cases of tests/f16x2_cases.py: every result
must equal the float64 value of the three-product formula BIT FOR BIT (tests/test_f16x2_cases_cpu.py proves that every partial sum of these
cases is exact in fp32 in any order, and that a missing or an extra product changes the bits).

Every operand is a window of a larger allocation at a 16-byte aligned offset with a row stride larger than its width (lda = K + 4,
ldb = K + 8) and fp32 NaN everywhere else; every result has ldc = N + 3 on a base that is only 4-byte aligned (2-byte for bf16) and the
sentinel everywhere, its window included: afterwards every element outside the window still holds the sentinel and every element inside the
expected bits.  bits, colsum, c_amax, bias and the maxima have exactly the documented number of elements, guarded the same way.  c_amax is
pre-filled with zeros and with values above the row maximum (atomic max: max(prefill, max |C|)).  pd_debug_set("f16x2_tile") is put back
whatever happens, and where a body is claimed pd_gemm_tn_f16x2_which is asserted before the launch
(tests/test_gemm_gpu.py::test_gemm_tn_h2_launches_the_kernel_its_plan_names pins that query to the kernel launched).

Which test reaches which body:
  gemm_tn_f16x2<128, 128, 64, 16, MODE 0 | 1, NRS 2 FAST 1 (debug 0) | NRS 1 FAST 0 (70, 4) | NRS 2 FAST 0 (14)>
        test_tile128_shapes, test_tile128_options (row maxima both / neither / one, over-stated, bias, ReLU, a row of zeros, rows beyond the
        clamp of the exponent, c_amax in modes 0 and 1), test_tile128_bf16out
  gemm_tn_f16x2<256, 256, 128, 16, MODE 0, NRS 1 (debug 3) | NRS 2 FAST 0 (13)>                      test_tile256_forced
  gemm_tn_f16x2<256, 256, 128, 16, MODE 1 | 2, NRS 2 FAST 1 (debug 0, 62) | FAST 0 (13)>              test_tile256_relu_pairs (c_amax in mode 2)
  gemm_rows_f16x2_k256<true | false, 0> (debug 0 and 61; the same bits as the tiled kernel, debug 80)   test_rows
  gemm_rows_f16x2_k256<true, 1 | 2>                                                                     test_rows_relu_pairs
  gemm_rows_f16x2_k256<true | false, 1 | 2>: the four (forward has maxima, backward has maxima) combinations   test_bits_contract
  gemm_kpc_f16x2<true | false>                                                                          test_kpc, test_kpc_many_items
  row_amax_f32 (float4 and scalar path), cast_bf16_f32_amax                                              test_row_amax, test_cast_bf16_amax
  the launcher's refusals                                                                               test_refusals, test_empty_problems
  gemm_tn_f16x2<128, 128, 64, 16, 0, CONV> (debug 0: interleaved step, 70: guarded step, 21: tap-major order) and <256, 256, 128, 16, 0, CONV>
        (debug 3) through pd_conv3x3_nhwc_f16x2                                                          test_conv3x3
  gemm_wgrad_f32x3_tr<0, false, true> + wgrad_tr_reduce, and with atomics (no workspace / one float too few)   test_wgrad_narrow,
        test_wgrad_narrow_body_on_a_wide_shape (pd_debug_set("wgrad_wide", 0))
  gemm_wgrad_f16x2_wide<false> + wgrad_h2w_reduce, and with atomics                                      test_wgrad_wide
  gemm_wgrad_f32x3_tr_grouped<true> + wgrad_tr_reduce_grouped                                            test_wgrad_grouped_narrow, .._mixed_takes_128_tiles
  gemm_wgrad_f16x2_wide_grouped + wgrad_h2w_reduce_grouped (bit for bit the single launches)             test_wgrad_grouped_wide_reproduces_the_single_launches
  gemm_wgrad_f32x3_tr<0, true, true>, gemm_wgrad_f16x2_wide<true> through pd_conv3x3_wgrad_nhwc_f16x2   test_conv3x3_wgrad
  (the weight gradients' and convolutions' refusals: test_wgrad_refusals, test_conv3x3_refuses_.., test_conv3x3_wgrad_refuses_..)
The convolution's input gradient is the same call on dY with the flipped, transposed filter: FC.CONV_DGRAD, the last case of test_conv3x3
(tests/test_f16x2_cases_cpu.py proves with autograd that its product is the gradient).

Found by test_bits_contract (before the fix in f16x2_plan: a bits launch took the row stream only with both maxima, the 256 x 256 tiled kernel
and its other bit order without): the combinations (maxima, none) and (none, maxima) at 8192 x 512 x 256."""
import contextlib

import pytest
import torch

import f16x2_cases as FC
import igemm_cases as IC
import smallgemm_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
PD_ERR_INVALID_ARG = -1
DEFAULTS = dict(f16x2_tile=0, wgrad_wide=1)
TILE128, TILE256, ROWS, KPC = 0, 1, 2, 5


def _libs():
    from partdistillation_amd import lib
    return lib, lib.load()


@pytest.fixture(autouse=True)
def _debug_values_back_at_their_defaults():
    yield
    _, L = _libs()
    for k, v in DEFAULTS.items():
        assert L.pd_debug_set(k.encode(), v) == 0


@contextlib.contextmanager
def _debug(value):
    lib, L = _libs()
    try:
        lib.check(L.pd_debug_set(b"f16x2_tile", value))
        yield
    finally:
        L.pd_debug_set(b"f16x2_tile", 0)


# ------------------------------------------------------------------------------------------------ guarded buffers
class Win:
    """a [rows, cols] window with row stride ld, `front` elements into an allocation that holds the bit pattern `fill` everywhere
    (the window too, unless .t is written): .t the window, .ptr its address, intact(): nothing outside it was written"""

    def __init__(self, rows, cols, ld, dtype, fill, front, tail=64):
        size = torch.empty((), dtype=dtype).element_size()
        idt = torch.int16 if size == 2 else I32
        assert ld >= cols
        self.fill = fill - (1 << (8 * size)) if fill >= 1 << (8 * size - 1) else fill
        self.raw = torch.full((front + rows * ld + tail,), self.fill, dtype=idt, device=DEV)
        body = self.raw[front:front + rows * ld].view(rows, ld)
        inside = torch.zeros(self.raw.shape, dtype=torch.bool, device=DEV)
        inside[front:front + rows * ld].view(rows, ld)[:, :cols] = True
        self.outside = ~inside
        self.t = body[:, :cols].view(dtype)
        self.ld = ld
        self.ptr = self.raw.data_ptr() + front * size

    @classmethod
    def of(cls, value, ld, front=64):
        """an operand: NaN around it, a 16-byte aligned base"""
        w = cls(value.shape[0], value.shape[1], ld, value.dtype, SC.NAN16 if value.element_size() == 2 else IC.NAN32, front)
        assert w.ptr % 16 == 0
        w.t.copy_(value)
        return w

    def intact(self):
        return bool((self.raw[self.outside] == self.fill).all())

    def untouched(self):
        return bool((self.raw == self.fill).all())


def _result(M, N, dtype=F32):
    """ldc = N + 3, the base 4-byte aligned only (2-byte for bf16), the sentinel everywhere"""
    w = Win(M, N, N + 3, dtype, SC.SENTINEL16 if dtype == BF16 else SC.SENTINEL32, front=65)
    assert w.ptr % 16 != 0
    return w


def _vec_in(t):
    """bias / row maxima: exactly t.numel() elements, NaN in front and behind"""
    return SC.Guarded.of(t.to(DEV).contiguous().view(1, -1), IC.NAN32, DEV, gap=0, tail=1)


def _vec_out(n, dtype=F32, prefill=None):
    """colsum / c_amax / bits: exactly n elements, the sentinel around them"""
    g = SC.Guarded(1, n, dtype, SC.SENTINEL32, DEV, gap=0, tail=1)
    if prefill is not None:
        g.t.copy_(prefill.view(1, -1))
    return g


def _ptr(g):
    return None if g is None else g.ptr


def _same_bits(got, want64, dtype=F32):
    want = want64.float().to(dtype)
    sentinel = SC.SENTINEL16 if dtype == BF16 else SC.SENTINEL32
    assert not bool((SC.bits(want) == sentinel).any())
    return torch.equal(SC.bits(got), SC.bits(want.to(got.device)))


def _amax_prefill(ref):
    """zeros and values above the row maximum, alternating"""
    top = ref.abs().amax(1) if ref.shape[1] else torch.zeros(ref.shape[0], dtype=torch.float64, device=ref.device)
    pre = (top * 4.0 + 1.0).float()
    pre[::2] = 0.0
    return pre


class Launch:
    """one pd_gemm_tn_f16x2 (or _bf16out) call on guarded buffers"""

    def __init__(self, a, b, bias=None, aa=None, ba=None, mode=0, bits=None, colsum=None, c_prefill=None, bf16=False):
        self.M, self.K, self.N = a.shape[0], a.shape[1], b.shape[0]
        self.A, self.B = Win.of(a.to(DEV), self.K + 4), Win.of(b.to(DEV), self.K + 8, front=68)
        self.bias = None if bias is None else _vec_in(bias)
        self.aa = None if aa is None else _vec_in(aa)
        self.ba = None if ba is None else _vec_in(ba)
        self.C = _result(self.M, self.N, BF16 if bf16 else F32)
        self.cam = None if c_prefill is None else _vec_out(self.M, F32, c_prefill)
        self.mode, self.bits, self.colsum, self.bf16 = mode, bits, colsum, bf16

    def which(self, L):
        return L.pd_gemm_tn_f16x2_which(self.M, self.N, self.K, self.A.ld, self.B.ld, self.mode, int(self.bits is not None), int(self.aa is not None),
                                        int(self.ba is not None), int(self.cam is not None), int(self.bf16))

    def run(self, lib, L):
        if self.bf16:
            return L.pd_gemm_tn_f16x2_bf16out(self.A.ptr, self.B.ptr, _ptr(self.bias), self.C.ptr, _ptr(self.aa), _ptr(self.ba), self.M, self.N, self.K,
                                              self.A.ld, self.B.ld, self.C.ld, lib.current_stream())
        return L.pd_gemm_tn_f16x2(self.A.ptr, self.B.ptr, _ptr(self.bias), self.C.ptr, _ptr(self.bits), _ptr(self.colsum), _ptr(self.aa), _ptr(self.ba),
                                  _ptr(self.cam), self.M, self.N, self.K, self.A.ld, self.B.ld, self.C.ld, self.mode, lib.current_stream())

    def outputs_untouched(self):
        return self.C.untouched() and all(g is None or g.untouched() for g in (self.bits, self.colsum)) and (self.cam is None or self.cam.intact())


def _reference(c, a, b, bias, aa, ba):
    dev = [None if t is None else t.to(DEV) for t in (a.x, b.x, aa, ba, bias)]
    return FC.ref_tn(dev[0], dev[1], dev[2], dev[3], dev[4], relu=c.mode == 1)


def _run_tn(c, family, with_c_amax=False, bf16=False):
    """launch case c under the current debug value, compare every bit; returns the result window's contents"""
    lib, L = _libs()
    a, b, bias = FC.tn_operands(c)
    aa, ba = FC.tn_maxima(c, a, b)
    ref = _reference(c, a, b, bias, aa, ba)
    pre = _amax_prefill(ref) if with_c_amax else None
    k = Launch(a.x, b.x, bias, aa, ba, mode=c.mode, c_prefill=pre, bf16=bf16)
    if family is not None:
        assert k.which(L) == family, (FC.tn_id(c), k.which(L))
    lib.check(k.run(lib, L))
    what = FC.tn_id(c)
    assert k.C.intact() and k.A.intact() and k.B.intact(), what
    assert _same_bits(k.C.t, ref, BF16 if bf16 else F32), what
    if with_c_amax:
        assert k.cam.intact(), what
        assert _same_bits(k.cam.t.view(-1), FC.ref_c_amax(ref, pre.to(DEV))), what
    return k.C.t.clone()


# ------------------------------------------------------------------------------------------------ 128 x 128 tiles
@pytest.mark.parametrize("dbg", FC.TILE128_DEBUG)
def test_tile128_shapes(dbg):
    with _debug(dbg):
        for c in FC.TILE128:
            _run_tn(c, TILE128)


@pytest.mark.parametrize("dbg", FC.TILE128_OPTIONS_DEBUG)
def test_tile128_options(dbg):
    with _debug(dbg):
        for c in FC.TILE128_OPTIONS:
            _run_tn(c, TILE128, with_c_amax=True)


@pytest.mark.parametrize("dbg", (0, 70))
def test_tile128_bf16out(dbg):
    """the float64 value rounded once to bf16; ldc in bf16 elements"""
    with _debug(dbg):
        for c in FC.BF16OUT:
            _run_tn(c, TILE128, bf16=True)


# ------------------------------------------------------------------------------------------------ 256 x 256 tiles
@pytest.mark.parametrize("dbg", FC.TILE256_DEBUG)
def test_tile256_forced(dbg):
    with _debug(dbg):
        for i, c in enumerate(FC.TILE256):
            _run_tn(c, TILE256, with_c_amax=i == 1)


def _relu_pair(p, family, fwd_maxima=True, bwd_maxima=True, forward=None):
    """mode 1 writes the bits, mode 2 (other operands) reads them.  forward: (bits buffer, forward reference) of an earlier call to reuse."""
    lib, L = _libs()
    words = L.pd_gemm_tn_f16x2_bits_words(p.M, p.N)
    assert words > 0
    if forward is None:
        a1, b1, bias1, _, _, _ = FC.pair_operands(p, fwd_maxima)
        aa, ba = (a1.amax, b1.amax) if fwd_maxima else (None, None)
        ref1 = FC.ref_tn(a1.x.to(DEV), b1.x.to(DEV), None if aa is None else aa.to(DEV), None if ba is None else ba.to(DEV), bias1.to(DEV), relu=True)
        bits = _vec_out(words, I32)
        pre = _amax_prefill(ref1)
        k1 = Launch(a1.x, b1.x, bias1, aa, ba, mode=1, bits=bits, c_prefill=pre)
        assert k1.which(L) == family, k1.which(L)
        lib.check(k1.run(lib, L))
        assert k1.C.intact() and bits.intact() and k1.cam.intact()
        assert _same_bits(k1.C.t, ref1)
        assert _same_bits(k1.cam.t.view(-1), FC.ref_c_amax(ref1, pre.to(DEV)))
        forward = (bits, ref1)
    bits, ref1 = forward
    _, _, _, a2, b2, prefill = FC.pair_operands(p, bwd_maxima)
    aa, ba = (a2.amax, b2.amax) if bwd_maxima else (None, None)
    ref2, colsum_ref = FC.ref_masked(a2.x.to(DEV), b2.x.to(DEV), None if aa is None else aa.to(DEV), None if ba is None else ba.to(DEV), ref1, prefill.to(DEV))
    colsum = _vec_out(p.N, F32, prefill.to(DEV))
    pre = _amax_prefill(ref2)
    snap = bits.snapshot()
    k2 = Launch(a2.x, b2.x, None, aa, ba, mode=2, bits=bits, colsum=colsum, c_prefill=pre)
    assert k2.which(L) == family, k2.which(L)
    lib.check(k2.run(lib, L))
    assert k2.C.intact() and colsum.intact() and k2.cam.intact() and bits.same_as(snap)
    assert _same_bits(k2.C.t, ref2), "the mask is not the forward's pattern (or the product is wrong)"
    assert _same_bits(colsum.t.view(-1), colsum_ref)
    assert _same_bits(k2.cam.t.view(-1), FC.ref_c_amax(ref2, pre.to(DEV)))
    return forward


@pytest.mark.parametrize("dbg", FC.RELU_PAIRS_TILED_DEBUG)
def test_tile256_relu_pairs(dbg):
    with _debug(dbg):
        for p in FC.RELU_PAIRS_TILED:
            _relu_pair(p, TILE256)


# ------------------------------------------------------------------------------------------------ the row stream
@pytest.mark.parametrize("c", FC.ROWS, ids=FC.tn_id)
def test_rows(c):
    """the product's default and debug 61 take the row stream; the tiled kernel (debug 80) gives the same bits"""
    _, L = _libs()
    got = []
    for dbg, family, cam in ((0, ROWS, False), (61, ROWS, True), (80, None, False)):
        with _debug(dbg):
            if family is None:
                assert L.pd_gemm_tn_f16x2_which(c.M, c.N, c.K, c.K + 4, c.K + 8, 0, 0, int(c.amax == "both"), int(c.amax == "both"), 0, 0) in (TILE128, TILE256)
            got.append(_run_tn(c, family, with_c_amax=cam))
    assert torch.equal(SC.bits(got[0]), SC.bits(got[2])) and torch.equal(SC.bits(got[1]), SC.bits(got[2]))


@pytest.mark.parametrize("p", FC.RELU_PAIRS_ROWS, ids=lambda p: f"{p.M}x{p.N}x{p.K}")
def test_rows_relu_pairs(p):
    _relu_pair(p, ROWS)


def test_bits_contract():
    """the order of the sign bits is a function of (M, N, K) alone: a backward launch with or without row maxima masks with the pattern a
    forward launch with or without them wrote.  A bits launch with the maxima of one operand only is refused where the row stream carries
    the bits (its kernel scales both operands or neither)."""
    lib, L = _libs()
    p = FC.BITS_CONTRACT
    for fwd in (True, False):
        forward = _relu_pair(p, ROWS, fwd, True)
        _relu_pair(p, ROWS, fwd, False, forward=forward)
    a1, b1, bias1, _, _, _ = FC.pair_operands(p, True)
    for aa, ba in ((a1.amax, None), (None, b1.amax)):
        k = Launch(a1.x, b1.x, bias1, aa, ba, mode=1, bits=_vec_out(L.pd_gemm_tn_f16x2_bits_words(p.M, p.N), I32))
        assert k.which(L) == -1
        assert k.run(lib, L) == PD_ERR_INVALID_ARG and k.outputs_untouched()


# ------------------------------------------------------------------------------------------------ producer / consumer wavefronts
@pytest.mark.parametrize("c", FC.KPC, ids=FC.tn_id)
def test_kpc(c):
    _run_tn(c, KPC)


def test_kpc_many_items():
    """more 192-row work items than CUs: a workgroup carries its counters and the inverse-scale slot from one item to the next; every
    192-row block has its own magnitude"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = FC.kpc_many(cus)
    assert -(-c.M // FC.KPC_BLOCK) * (c.N // 256) > cus
    _run_tn(c, KPC)


# ------------------------------------------------------------------------------------------------ row maxima
def _amax_input(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, cols), generator=g)
    x[0] = 0.0                                                    # a row of zeros
    if rows > 1:
        x[1, 0], x[1, cols // 2] = -0.0, -torch.finfo(F32).max      # -0.0 and the largest finite value
    if rows > 2:
        x[2, cols - 1] = 1e6                                      # the maximum in the last column
    return x


@pytest.mark.parametrize("rows, cols, ld, off", FC.ROW_AMAX)
def test_row_amax(rows, cols, ld, off):
    lib, L = _libs()
    x = _amax_input(rows, cols, 3000 + rows + cols)
    X = Win(rows, cols, ld, F32, IC.NAN32, front=64 + (off % 4))
    X.t.copy_(x)
    assert (X.ptr % 16 == 0) == (off == 4)
    out = _vec_out(rows)
    lib.check(L.pd_row_amax_f32(X.ptr, rows, cols, ld, out.ptr, lib.current_stream()))
    assert out.intact() and X.intact()
    assert torch.equal(SC.bits(out.t.view(-1)), SC.bits(x.abs().amax(1).to(DEV)))


@pytest.mark.parametrize("rows, cols", FC.CAST_AMAX)
def test_cast_bf16_amax(rows, cols):
    lib, L = _libs()
    x = _amax_input(rows, cols, 3100 + rows).to(BF16)
    if rows > 1:
        x[1, cols // 2] = -torch.finfo(BF16).max                  # (fp32's largest value rounds to infinity)
    X = _vec_in_bf16(x)
    Y, out = _vec_out(rows * cols), _vec_out(rows)
    lib.check(L.pd_cast_bf16_f32_amax(X.ptr, rows, cols, Y.ptr, out.ptr, lib.current_stream()))
    assert Y.intact() and out.intact()
    assert torch.equal(SC.bits(Y.t.view(rows, cols)), SC.bits(x.float().to(DEV)))
    assert torch.equal(SC.bits(out.t.view(-1)), SC.bits(x.float().abs().amax(1).to(DEV)))


def _vec_in_bf16(t):
    return SC.Guarded.of(t.to(DEV).contiguous().view(1, -1), SC.NAN16, DEV, gap=0, tail=1)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(k, what, **over):
    lib, L = _libs()
    args = dict(A=k.A.ptr, B=k.B.ptr, M=k.M, N=k.N, K=k.K, lda=k.A.ld, ldb=k.B.ld, mode=k.mode, bits=_ptr(k.bits), colsum=_ptr(k.colsum))
    args.update(over)
    rc = L.pd_gemm_tn_f16x2(args["A"], args["B"], _ptr(k.bias), k.C.ptr, args["bits"], args["colsum"], _ptr(k.aa), _ptr(k.ba), _ptr(k.cam), args["M"], args["N"],
                            args["K"], args["lda"], args["ldb"], k.C.ld, args["mode"], lib.current_stream())
    assert rc == PD_ERR_INVALID_ARG, (what, rc)
    assert L.pd_last_error().decode().startswith("pd_gemm_tn_f16x2"), what
    assert k.outputs_untouched(), what


def test_refusals():
    lib, L = _libs()
    c = FC.TILE128[1]
    a, b, _ = FC.tn_operands(c)
    k = Launch(a.x, b.x, None, a.amax, b.amax)
    _refused(k, "K % 4", K=c.K - 2)
    _refused(k, "lda % 4", lda=c.K + 2)
    _refused(k, "ldb % 4", ldb=c.K + 2)
    _refused(k, "A misaligned", A=k.A.ptr + 4)
    _refused(k, "B misaligned", B=k.B.ptr + 8)
    _refused(k, "mode 3", mode=3)
    kb = Launch(a.x, b.x, None, a.amax, b.amax, bf16=True)
    for what, K, lda, A in (("K % 4", c.K - 2, kb.A.ld, kb.A.ptr), ("lda % 4", c.K, kb.A.ld + 2, kb.A.ptr), ("A misaligned", c.K, kb.A.ld, kb.A.ptr + 4)):
        assert L.pd_gemm_tn_f16x2_bf16out(A, kb.B.ptr, None, kb.C.ptr, kb.aa.ptr, kb.ba.ptr, kb.M, kb.N, K, lda, kb.B.ld, kb.C.ld, lib.current_stream()) == PD_ERR_INVALID_ARG, what
        assert kb.C.untouched(), ("bf16out", what)
    # mode 2 without bits / without colsum, on a shape that takes bits
    p = FC.RELU_PAIRS_TILED[0]
    a1, b1, _, _, _, pre = FC.pair_operands(p, True)
    words = L.pd_gemm_tn_f16x2_bits_words(p.M, p.N)
    k = Launch(a1.x, b1.x, None, a1.amax, b1.amax, mode=2, bits=_vec_out(words, I32), colsum=_vec_out(p.N))
    _refused(k, "mode 2 without bits", bits=None)
    _refused(k, "mode 2 without colsum", colsum=None)
    # sign bits where N % 256 != 0 or M < 1024 (the 256 x 256 kernel's order), and forced wide tiles on such shapes
    for M, N in ((1024, 132), (130, 256)):
        a = FC.operand(M, 16, 3201, **FC.DENSE)
        b = FC.operand(N, 16, 3202, **FC.DENSE)
        k = Launch(a.x, b.x, None, a.amax, b.amax, mode=1, bits=_vec_out(4096, I32))
        assert k.which(L) == -1
        _refused(k, f"bits on {M} x {N}")
        k = Launch(a.x, b.x, None, a.amax, b.amax)
        for dbg in (3, 13):
            with _debug(dbg):
                assert k.which(L) == -1
                _refused(k, f"forced wide tiles on {M} x {N}")


def test_empty_problems():
    """M = 0 or N = 0: returns 0, writes nothing"""
    lib, L = _libs()
    c = FC.TILE128[1]
    a, b, _ = FC.tn_operands(c)
    k = Launch(a.x, b.x, None, a.amax, b.amax, c_prefill=torch.zeros(c.M))
    for M, N in ((0, c.N), (c.M, 0)):
        assert L.pd_gemm_tn_f16x2(k.A.ptr, k.B.ptr, None, k.C.ptr, None, None, k.aa.ptr, k.ba.ptr, k.cam.ptr, M, N, c.K, k.A.ld, k.B.ld, k.C.ld, 0,
                                  lib.current_stream()) == 0
        assert k.C.untouched() and bool((k.cam.t == 0).all()) and k.cam.intact()


# ------------------------------------------------------------------------------------------------ two-plane weight gradients
class Wgrad:
    """one weight-gradient problem on guarded buffers: ldy = N + 4, ldx = K + 8, ldw = K + 5 on a 4-byte aligned base, dW and dB pre-filled"""

    def __init__(self, c, with_db=True):
        self.c = c
        dy, x, ya, xa, dw0, db0 = FC.wg_operands(c)
        self.dY, self.X = Win.of(dy.x.to(DEV), c.N + 4), Win.of(x.x.to(DEV), c.K + 8, front=68)
        self.ya = None if ya is None else _vec_in(ya)
        self.xa = None if xa is None else _vec_in(xa)
        self.dW = Win(c.N, c.K, c.K + 5, F32, SC.SENTINEL32, front=65)
        self.dW.t.copy_(dw0)
        self.dB = _vec_out(c.N, F32, db0.to(DEV))
        self.with_db = with_db
        self.db_snap = self.dB.snapshot()
        dev = [None if t is None else t.to(DEV) for t in (dy.x, x.x, ya, xa, dw0, db0)]
        self.ref_dw, self.ref_db = FC.ref_wgrad(*dev[:5]), FC.ref_db(dev[0], dev[5])

    def desc(self, d):
        c = self.c
        d.dY, d.X, d.dW, d.dB = self.dY.ptr, self.X.ptr, self.dW.ptr, (self.dB.ptr if self.with_db else None)
        d.M, d.N, d.K, d.ldy, d.ldx, d.ldw = c.M, c.N, c.K, self.dY.ld, self.X.ld, self.dW.ld
        d.y_amax, d.x_amax = _ptr(self.ya), _ptr(self.xa)

    def run(self, ws, ws_floats):
        lib, L = _libs()
        c = self.c
        return L.pd_gemm_wgrad_acc_f16x2_ws(self.dY.ptr, self.X.ptr, self.dW.ptr, self.dB.ptr if self.with_db else None, _ptr(self.ya), _ptr(self.xa),
                                            ws, ws_floats, c.M, c.N, c.K, self.dY.ld, self.X.ld, self.dW.ld, lib.current_stream())

    def check(self, what=""):
        what = (FC.wg_id(self.c), what)
        assert self.dW.intact() and self.dB.intact() and self.dY.intact() and self.X.intact(), what
        assert _same_bits(self.dW.t, self.ref_dw), what
        if self.with_db:
            assert _same_bits(self.dB.t.view(-1), self.ref_db), what
        else:
            assert self.dB.same_as(self.db_snap), what          # dB == NULL: nothing written


def _wgrad_single(c, wide, workspace, with_db=True):
    """workspace: "exact" (the floats the header's size function returns, guarded: pd_gemm_wgrad_f16x2_ws_floats covers whichever tile shape a
    launch may take, 64 MB for an output of one 256-tile) | "null" | "short" (one float fewer than the launch's partial tiles need: atomics)"""
    lib, L = _libs()
    assert L.pd_gemm_wgrad_f16x2_takes_wide_tiles(c.N, c.K) == int(wide), FC.wg_id(c)
    need = L.pd_gemm_wgrad_f16x2_ws_floats(c.N, c.K)
    assert need > 0
    tiles, slices = FC.wg_narrow_plan(c)
    reduces = not wide and slices >= 2                         # the 128-tile body goes through the workspace at all
    floats = need if workspace == "exact" or not reduces else tiles * slices * 128 * 128 - 1
    assert floats <= need
    ws = None if workspace == "null" else _vec_out(floats)
    w = Wgrad(c, with_db)
    lib.check(w.run(_ptr(ws), 0 if ws is None else floats))
    w.check(workspace)
    assert ws is None or ws.intact()
    if ws is not None and not wide:                            # partial tiles in the workspace, or atomics and a workspace nobody touched
        assert ws.untouched() == (not reduces or workspace == "short"), (FC.wg_id(c), workspace)
    return w.dW.t.clone()


@pytest.mark.parametrize("workspace", ("exact", "null", "short"))
def test_wgrad_narrow(workspace):
    """gemm_wgrad_f32x3_tr<.., H2> with wgrad_tr_reduce (workspace) and with atomics (none, or one float too small)"""
    for i, c in enumerate(FC.WGRAD_NARROW):
        _wgrad_single(c, False, workspace, with_db=i != 1)


def test_wgrad_narrow_body_on_a_wide_shape():
    lib, L = _libs()
    try:
        lib.check(L.pd_debug_set(b"wgrad_wide", 0))
        _wgrad_single(FC.WGRAD_WIDE[0], False, "exact")
    finally:
        L.pd_debug_set(b"wgrad_wide", 1)


@pytest.mark.parametrize("workspace", ("exact", "null"))
def test_wgrad_wide(workspace):
    """gemm_wgrad_f16x2_wide with wgrad_h2w_reduce, and with atomics"""
    for i, c in enumerate(FC.WGRAD_WIDE):
        _wgrad_single(c, True, workspace, with_db=i != 2)


def _wgrad_grouped(cases, wide):
    lib, L = _libs()
    Desc = lib.struct("PdGemmWgradDesc")
    probs = [Wgrad(c, with_db=i != 1) for i, c in enumerate(cases)]
    descs = (Desc * len(probs))()
    for d, w in zip(descs, probs):
        w.desc(d)
    assert all(L.pd_gemm_wgrad_f16x2_takes_wide_tiles(c.N, c.K) for c in cases) == wide
    need = L.pd_gemm_wgrad_f16x2_grouped_ws_floats(descs, len(probs))
    assert need > 0
    nbytes = L.pd_gemm_wgrad_f32x3_grouped_table_bytes(len(probs))
    host, table, ws = torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), torch.zeros(nbytes, dtype=torch.uint8, device=DEV), _vec_out(need)
    lib.check(L.pd_gemm_wgrad_f16x2_grouped(descs, len(probs), host.data_ptr(), table.data_ptr(), ws.ptr, need, lib.current_stream()))
    torch.cuda.synchronize()
    for w in probs:
        w.check("grouped")
    assert ws.intact()
    return [w.dW.t.clone() for w in probs]


def test_wgrad_grouped_narrow():
    """three problems of unequal M (one row among them) on 128 tiles"""
    _wgrad_grouped(FC.WGRAD_GROUPED_NARROW, False)


def test_wgrad_grouped_wide_reproduces_the_single_launches():
    got = _wgrad_grouped(FC.WGRAD_WIDE, True)
    for c, g in zip(FC.WGRAD_WIDE, got):
        assert torch.equal(SC.bits(g), SC.bits(_wgrad_single(c, True, "exact")))


def test_wgrad_grouped_mixed_takes_128_tiles():
    _wgrad_grouped(FC.WGRAD_GROUPED_MIXED, False)


def test_wgrad_refusals():
    lib, L = _libs()
    c = FC.WGRAD_NARROW[1]
    w = Wgrad(c)
    snap = w.dW.raw.clone()
    need = L.pd_gemm_wgrad_f16x2_ws_floats(c.N, c.K)
    ws = _vec_out(need)
    st = lib.current_stream()
    for what, N, K, ldy, ldx, dy in (("N % 4", c.N - 2, c.K, w.dY.ld, w.X.ld, w.dY.ptr), ("K % 4", c.N, c.K - 2, w.dY.ld, w.X.ld, w.dY.ptr),
                                     ("ldy % 4", c.N, c.K, w.dY.ld + 2, w.X.ld, w.dY.ptr), ("ldx % 4", c.N, c.K, w.dY.ld, w.X.ld + 2, w.dY.ptr),
                                     ("dY misaligned", c.N, c.K, w.dY.ld, w.X.ld, w.dY.ptr + 4)):
        rc = L.pd_gemm_wgrad_acc_f16x2_ws(dy, w.X.ptr, w.dW.ptr, w.dB.ptr, None, None, ws.ptr, need, c.M, N, K, ldy, ldx, w.dW.ld, st)
        assert rc == PD_ERR_INVALID_ARG, what
        assert torch.equal(w.dW.raw, snap) and w.dB.same_as(w.db_snap) and ws.untouched(), what
    # a grouped count of 257
    Desc = lib.struct("PdGemmWgradDesc")
    descs = (Desc * 257)()
    for d in descs:
        w.desc(d)
    nbytes = L.pd_gemm_wgrad_f32x3_grouped_table_bytes(257)
    host, table = torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    assert L.pd_gemm_wgrad_f16x2_grouped(descs, 257, host.data_ptr(), table.data_ptr(), ws.ptr, need, st) == PD_ERR_INVALID_ARG
    assert torch.equal(w.dW.raw, snap) and w.dB.same_as(w.db_snap) and ws.untouched()
    # no rows: returns 0, writes nothing
    assert L.pd_gemm_wgrad_acc_f16x2_ws(w.dY.ptr, w.X.ptr, w.dW.ptr, w.dB.ptr, None, None, ws.ptr, need, 0, c.N, c.K, w.dY.ld, w.X.ld, w.dW.ld, st) == 0
    assert torch.equal(w.dW.raw, snap) and w.dB.same_as(w.db_snap) and ws.untouched()


# ------------------------------------------------------------------------------------------------ 3 x 3 convolution
@pytest.mark.parametrize("dbg", FC.CONV_DEBUG)
def test_conv3x3(dbg):
    """gemm_tn_f16x2<128, 128, 64, 16, 0, CONV>: the interleaved step (debug 0), the guarded step (70), tap-major order (21), and
    <256, 256, 128, 16, 0, CONV> forced (3).  The tensors are dense (the entry point takes no strides): NaN in front of and behind X and Wk,
    the sentinel around Y and y_amax."""
    lib, L = _libs()
    with _debug(dbg):
        for c in FC.CONV:
            x, w, bias = FC.conv_operands(c)
            has_x, has_w = c.amax in ("both", "x"), c.amax in ("both", "w")
            M = c.B * c.H * c.W
            aa = FC.patch_maxima(c, x.amax.to(DEV)) if has_x else None
            ref = FC.ref_tn(FC.patches(c, x.x.to(DEV)), w.x.to(DEV), aa, w.amax.to(DEV) if has_w else None, None if bias is None else bias.to(DEV))
            X, Wk, Y = _vec_in(x.x), _vec_in(w.x), _vec_out(M * c.Co)
            xa, wa, bv = (_vec_in(x.amax) if has_x else None), (_vec_in(w.amax) if has_w else None), (None if bias is None else _vec_in(bias))
            pre = _amax_prefill(ref)
            ya = _vec_out(M, F32, pre)
            lib.check(L.pd_conv3x3_nhwc_f16x2(X.ptr, Wk.ptr, _ptr(bv), Y.ptr, _ptr(xa), _ptr(wa), ya.ptr, c.B, c.H, c.W, c.Ci, c.Co, lib.current_stream()))
            what = (FC.conv_id(c), dbg)
            assert Y.intact() and ya.intact() and X.intact() and Wk.intact(), what
            assert _same_bits(Y.t.view(M, c.Co), ref), what
            assert _same_bits(ya.t.view(-1), FC.ref_c_amax(ref, pre)), what


def test_conv3x3_refuses_channels_that_are_no_multiple_of_16():
    lib, L = _libs()
    x, w = torch.ones(2 * 3 * 3, 24), torch.ones(8, 9 * 24)
    X, Wk, Y, ya = _vec_in(x), _vec_in(w), _vec_out(18 * 8), _vec_out(18)
    assert L.pd_conv3x3_nhwc_f16x2(X.ptr, Wk.ptr, None, Y.ptr, None, None, ya.ptr, 2, 3, 3, 24, 8, lib.current_stream()) == PD_ERR_INVALID_ARG
    assert Y.untouched() and ya.untouched()


@pytest.mark.parametrize("i", range(len(FC.CONV_WGRAD)), ids=[FC.conv_wg_id(c) for c in FC.CONV_WGRAD])
def test_conv3x3_wgrad(i):
    """pd_conv3x3_wgrad_nhwc_f16x2 on the 128-tile body (gemm_wgrad_f32x3_tr<0, true, true>) and, for 256 channels, the wide one
    (gemm_wgrad_f16x2_wide<true>); dense tensors, dWk and dB accumulated into exact pre-fills, the workspace exactly as large as asked"""
    lib, L = _libs()
    c = FC.CONV_WGRAD[i]
    M, K = c.B * c.H * c.W, 9 * c.Ci
    assert bool(L.pd_gemm_wgrad_f16x2_takes_wide_tiles(c.Co, K) and c.Ci % 256 == 0) == c.wide
    dy, x, ya, xa, dw0, db0 = FC.conv_wg_operands(c)
    dev = [None if t is None else t.to(DEV) for t in (dy.x, x.x, ya, xa, dw0, db0)]
    ref_dw, ref_db = FC.ref_wgrad(dev[0], FC.patches(c, dev[1]), dev[2], dev[3], dev[4]), FC.ref_db(dev[0], dev[5])
    need = L.pd_gemm_wgrad_f16x2_ws_floats(c.Co, K)
    assert need > 0
    dY, X, dW, dB, ws = _vec_in(dy.x), _vec_in(x.x), _vec_out(c.Co * K, F32, dev[4]), _vec_out(c.Co, F32, dev[5]), _vec_out(need)
    yv, xv = (None if ya is None else _vec_in(ya)), (None if xa is None else _vec_in(xa))
    with_db = i != 1
    snap = dB.snapshot()
    lib.check(L.pd_conv3x3_wgrad_nhwc_f16x2(dY.ptr, X.ptr, dW.ptr, dB.ptr if with_db else None, _ptr(yv), _ptr(xv), ws.ptr, need, c.B, c.H, c.W, c.Ci, c.Co,
                                            lib.current_stream()))
    assert dW.intact() and dB.intact() and ws.intact() and dY.intact() and X.intact()
    assert _same_bits(dW.t.view(c.Co, K), ref_dw)
    assert _same_bits(dB.t.view(-1), ref_db) if with_db else dB.same_as(snap)


def test_conv3x3_wgrad_refuses_channels_that_are_no_multiple_of_128():
    lib, L = _libs()
    dY, X, dW, dB, ws = _vec_in(torch.ones(9, 8)), _vec_in(torch.ones(9, 64)), _vec_out(8 * 9 * 64), _vec_out(8), _vec_out(1 << 16)
    assert L.pd_conv3x3_wgrad_nhwc_f16x2(dY.ptr, X.ptr, dW.ptr, dB.ptr, None, None, ws.ptr, 1 << 16, 1, 3, 3, 64, 8, lib.current_stream()) == PD_ERR_INVALID_ARG
    assert dW.untouched() and dB.untouched() and ws.untouched()
