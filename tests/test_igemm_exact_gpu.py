"""Every kernel body of csrc/igemm_bf16.hip, csrc/igemm_epilogue.inc and csrc/wgrad_bf16.hip on the exact cases of tests/igemm_cases.py
(its docstring lists which body each table reaches), through the C-ABI of include/pd_igemm.h: integer-valued bf16 operands whose products
and partial sums are exact in fp32 in any order, so a result must equal the float64 reference rounded ONCE to bf16, bit for bit (GELU and
GELU' results: within the derived bound of igemm_cases.gelu_bound; the pre-activation of the same launch stays bit-exact).
Every operand and result is a dense window at a 16-byte aligned offset of a larger allocation — bf16 / fp32 NaN around every input, a
sentinel around AND inside every output, compared afterwards; workspaces have exactly the size the header's functions return, with a
sentinel behind them; pd_igemm_bf16's 4096 ticket words start at zero and must be zero again after every launch; the first 16 KB of
pd_wgrad_bf16's workspace must come back untouched.  Schedules are forced with pd_debug_set and put back whatever happens.

Kernel bodies and the tests that reach them:
  igemm_bf16<64 | 128, 1 | 2 | 3, P1 = true>    test_plain_rows_every_tile_width_and_ring_depth (1, 2, 3, 5 K-steps under every ring)
  igemm_bf16<64 | 128, 1 | 2 | 3, P1 = false>   test_gathered_forward, test_gathered_input_gradient (nine-tap walk, stride-2 1 x 1)
    ... with parity classes                    test_parity_classes_equal_the_nine_tap_walk
  igemm3x3_bf16                                test_patch_form_equals_the_gathered_kernel, test_patch_form_channel_chunk_splits
  splitk_seam<1>, splitk_seam<2>               test_split_k_seam_is_exact_and_repeats (<1> also behind igemm3x3_bf16's chunk splits and the
                                               gathered 3 x 3 kernels), test_epilogue[split3-bn128-*]
  igemm_epilogue.inc                           test_epilogue (<64, 1>, <128, 1>: EPI_PIPE == false, parity classes, patch form, behind the seam),
                                               test_column_slabs, test_gate_pointer_is_ignored_under_gate_mode_none
  pd_igemm_bf16_seq                            test_sequence_of_three_problems_shares_one_workspace
  filter_transpose_grouped                     test_grouped_filter_transposes
  wgrad_bf16<1 | 2>, wgrad_bf16_reduce         test_weight_gradient
  wgrad_bf16_reduce_grouped                    test_weight_gradient_sequence_equals_the_single_launches
  make_plan / wg_plan refusals                 test_igemm_refuses_bad_arguments_and_launches_nothing, test_weight_gradient_refuses_bad_arguments_and_launches_nothing"""
import contextlib
import ctypes
import functools

import pytest
import torch

import igemm_cases as IC
import smallgemm_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
PD_ERR_INVALID_ARG = -1
TICKET_WORDS = 4096                                            # 16 KB: pd_igemm_bf16's tickets, pd_wgrad_bf16's untouched header
DEFAULTS = dict(ig_bn=0, ig_nst=0, ig_splits=0, ig_pcls=1, ig_patch=1, wg_nst=0, wg_splits=0)


def _libs():
    from partdistillation_amd import lib
    return lib, lib.load()


@pytest.fixture(autouse=True)
def _every_knob_back_at_its_default():
    yield
    _, L = _libs()
    for k, v in DEFAULTS.items():
        assert L.pd_debug_set(k.encode(), v) == 0


@contextlib.contextmanager
def _knobs(kn):
    lib, L = _libs()
    try:
        for k, v in kn.items():
            lib.check(L.pd_debug_set(k.encode(), v))
        yield
    finally:
        for k in kn:
            L.pd_debug_set(k.encode(), DEFAULTS[k])


def _kid(kn):
    return "-".join(f"{k[3:]}{v}" for k, v in kn.items()) or "auto"


# ------------------------------------------------------------------------------------------------ guarded buffers
def _in(t):
    """an input: one dense window, NaN in front of and behind it"""
    return SC.Guarded.of(t.contiguous().view(1, -1), SC.NAN16 if t.element_size() == 2 else IC.NAN32, DEV, gap=0, tail=1)


def _out(numel, dtype=BF16, pad=8):
    """a result: the sentinel everywhere, the window included (an element the kernel skips keeps it)"""
    return SC.Guarded(1, numel, dtype, SC.SENTINEL16 if dtype == BF16 else SC.SENTINEL32, DEV, pad=pad, gap=0, tail=1)


def _igemm_workspace(nbytes):
    """exactly nbytes, the sentinel behind (and in the slabs); the ticket words zero"""
    assert nbytes > TICKET_WORDS * 4 and nbytes % 4 == 0
    ws = _out(nbytes // 4, I32)
    ws.t[0, :TICKET_WORDS] = 0
    return ws


def _assert_exact(got, ref64, what):
    g, w = SC.bits(got.cpu()), SC.bits(SC.expected(ref64))
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} results differ from the float64 reference rounded once; first at {i}: "
                             f"got {float(got.cpu()[i])} want {float(SC.expected(ref64)[i])} (reference {float(ref64[i])})")


def _assert_within_gelu_bound(got, ref, what):
    g = got.cpu().double()
    assert not torch.isnan(g).any() and not (SC.bits(got.cpu()) == SC.SENTINEL16).any(), what + ": NaN, or an element never written"
    err, bound = (g - ref["out"]).abs(), IC.gelu_bound(ref["out"], ref["x"])
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} results beyond 2^-8 |ref| + 2e-6 max(|x|, 1); first at {i}: got {float(g[i])} "
                             f"reference {float(ref['out'][i])} x {float(ref['x'][i])} error {float(err[i])} bound {float(bound[i])}")


# ------------------------------------------------------------------------------------------------ pd_igemm_bf16
@functools.lru_cache(maxsize=None)
def _reference(g, e):
    """computed once per (case, epilogue), shared, never modified"""
    src, w, wk = IC.conv_operands(g)
    o = IC.epi_operands(g, e)
    return src, wk, o, IC.ref_epilogue(g, e, IC.ref_conv(g, src, w), o)


class _Problem:
    """the descriptor of one launch and its guarded buffers"""

    def __init__(self, g, e=IC.NO_EPI, slab=0):
        lib, _ = _libs()
        self.g, self.e, self.slab = g, e, slab
        src, wk, o, self.ref = _reference(g, e)
        self.M, self.n = IC.rows_of(g), IC.dims(g)["n"]
        self.inputs = dict(src=_in(src), w=_in(wk), **{k: _in(v) for k, v in o.items()})
        self.out = _out(self.M * self.n)
        self.pre = _out(self.M * self.n) if e.pre else None
        d = self.d = lib.struct("PdIgemm")()
        for k, v in IC.dims(g).items():
            setattr(d, k, v)
        d.src, d.w, d.out = self.inputs["src"].ptr, self.inputs["w"].ptr, self.out.ptr
        for k in ("scale", "bias", "res", "res2", "gate"):
            setattr(d, k, self.inputs[k].ptr if k in self.inputs else None)
        d.out_pre = self.pre.ptr if e.pre else None
        d.act, d.gate_mode, d.res_mode = e.act, e.gate, IC.RES_UP2 if e.res == "up2" else IC.RES_DENSE
        d.bias_bf16, d.out_col_slab = int(e.bias == "bf16"), slab
        self.snap = {k: b.snapshot() for k, b in self.inputs.items()}

    def check(self, what):
        """exact (or within the GELU bound), every element written, nothing outside, no input touched"""
        want = self.ref["out"] if not self.slab else IC.slabbed(self.ref["out"], self.slab).view(self.M, self.n)
        got = self.out.t.view(self.M, self.n)
        if IC.is_exact(self.e):
            _assert_exact(got, want, what)
        else:
            _assert_within_gelu_bound(got, self.ref, what)
        assert self.out.intact(), what + ": a store outside the result"
        if self.pre is not None:
            _assert_exact(self.pre.t.view(self.M, self.n), self.ref["pre"], what + " (out_pre)")
            assert self.pre.intact(), what + ": a store outside out_pre"
        assert all(b.same_as(self.snap[k]) for k, b in self.inputs.items()), what + ": an input was written"
        return SC.bits(got.cpu())


def _launch(p, what, ws=None):
    """one pd_igemm_bf16 launch under the knobs in force, with a workspace of exactly pd_igemm_bf16_workspace_bytes -> (bits, workspace bytes)"""
    lib, L = _libs()
    need = L.pd_igemm_bf16_workspace_bytes(ctypes.byref(p.d))
    assert need == 0 or need > TICKET_WORDS * 4, (what, need, L.pd_last_error().decode())
    if need and ws is None:
        ws = _igemm_workspace(need)
    lib.check(L.pd_igemm_bf16(ctypes.byref(p.d), ws.ptr if need else None, need, lib.current_stream()))
    torch.cuda.synchronize()
    if need:
        assert ws.intact(), what + ": a store behind the workspace"
        assert not ws.t[0, :TICKET_WORDS].any(), what + ": tickets not back at zero"
    return p.check(what), need


def _run(g, e=IC.NO_EPI, knobs=None, slab=0):
    what = f"{g.name} {IC.epi_id(e)} {_kid(knobs or {})}"
    with _knobs(knobs or {}):
        return _launch(_Problem(g, e, slab), what)


def _slab_bytes(g, bn, splits, patch=False):
    """the workspace the split schedule of the header needs: tickets + tiles x splits fp32 partial tiles"""
    d = IC.dims(g)
    if patch:
        tiles = d["batch"] * -(-d["ho"] // 8) * -(-d["wo"] // 16) * (d["n"] // 64)
    else:
        tiles = -(-IC.rows_of(g) // IC.BM) * (d["n"] // bn)
    return TICKET_WORDS * 4 + tiles * splits * IC.BM * bn * 4


@pytest.mark.parametrize("g,kn", [(g, kn) for g in IC.PLAIN for kn in IC.plain_schedules(g)], ids=lambda v: v.name if isinstance(v, IC.Geo) else _kid(v))
def test_plain_rows_every_tile_width_and_ring_depth(g, kn):
    _, need = _run(g, knobs=kn)
    assert need == 0


@pytest.mark.parametrize("g,kn,splits", IC.SPLIT, ids=lambda v: v.name if isinstance(v, IC.Geo) else _kid(v) if isinstance(v, dict) else f"{v}splits")
def test_split_k_seam_is_exact_and_repeats(g, kn, splits):
    """splitk_seam<1> (64-wide tiles) and <2> (128-wide): forced 3 | 2 and 2 | 2 | 1 K-steps, 3 splits clipped to KT = 2, and the automatic schedule
    of 16 K-steps under 2 tiles; twice into fresh sentinel-filled outputs"""
    a, need = _run(g, knobs=kn)
    b, _ = _run(g, knobs=kn)
    assert need == _slab_bytes(g, kn.get("ig_bn", 64), splits), (need, "the plan did not arrive at the splits this case is about")
    assert torch.equal(a, b)


@pytest.mark.parametrize("g,kn", [(g, kn) for g in IC.FWD for kn in IC.fwd_schedules(g)], ids=lambda v: v.name if isinstance(v, IC.Geo) else _kid(v))
def test_gathered_forward(g, kn):
    """3 x 3 and 1 x 1 stride 2 on an odd and an even grid, 3 x 3 stride 1 on the gathered kernel; a row tile spans both images"""
    assert g.B == 2 and (IC.dims(g)["ho"] * IC.dims(g)["wo"]) % IC.BM != 0
    _run(g, knobs=kn)
    _run(g, IC.Epi(True, "f32", "dense", False, False, IC.ACT_RELU, IC.GATE_NONE), knobs=kn)      # the bottleneck's own epilogue


@pytest.mark.parametrize("g", IC.DGRAD, ids=lambda g: g.name)
def test_gathered_input_gradient(g):
    """1 x 1; stride-2 1 x 1 (pixels with an odd coordinate receive only the addends); the nine-tap walk of the stride-2 3 x 3 on an odd grid and,
    under ig_pcls = 0, on an even one; 3 x 3 stride 1 on the gathered kernel"""
    kn = IC.gathered_knobs(g)
    for nst in (0, 1, 2, 3):                                   # the plan's own ring depth, then each one forced
        _run(g, knobs=dict(kn, ig_nst=nst))
    _run(g, IC.Epi(False, None, "dense", True, False, IC.ACT_NONE, IC.GATE_RELU), knobs=kn)      # both addends and the ReLU mask of the layer below
    if g.stride == 2 and g.k == 1:
        acc = IC.ref_conv(g, *IC.conv_operands(g)[:2]).view(g.B, g.H, g.W, -1)
        assert not acc[:, 1::2].any() and not acc[:, :, 1::2].any() and acc[:, ::2, ::2].any()


@pytest.mark.parametrize("kn", IC.PCLS_SCHEDULES, ids=_kid)
@pytest.mark.parametrize("g", IC.PCLS, ids=lambda g: g.name)
def test_parity_classes_equal_the_nine_tap_walk(g, kn):
    a, _ = _run(g, knobs=kn)
    b, _ = _run(g, knobs=dict(kn, ig_pcls=0))
    assert torch.equal(a, b)
    e = IC.Epi(False, None, "up2", True, False, IC.ACT_NONE, IC.GATE_RELU)                      # the strided shortcut's compact gradient as the addend
    a, _ = _run(g, e, knobs=kn)
    b, _ = _run(g, e, knobs=dict(kn, ig_pcls=0))
    assert torch.equal(a, b)


@pytest.mark.parametrize("fwd,bwd", IC.PATCH, ids=lambda g: g.name)
def test_patch_form_equals_the_gathered_kernel(fwd, bwd):
    """igemm3x3_bf16 forward and input gradient: one pixel, exactly one 8 x 16 block, three ragged blocks in a row, 2 x 2 ragged blocks of two
    images; 1, 2, 3, 5 channel chunks (5: split over workgroups by the plan itself)"""
    for g in (fwd, bwd):
        cs = IC.dims(g)["cs"]
        a, need = _run(g)
        assert need == (_slab_bytes(g, 64, 3, patch=True) if cs >= 256 else 0), need
        b, _ = _run(g, knobs=dict(ig_patch=0))
        assert torch.equal(a, b)


@pytest.mark.parametrize("cs,forced,chunks", IC.PATCH_SPLIT, ids=lambda v: str(v))
def test_patch_form_channel_chunk_splits(cs, forced, chunks):
    """chunks 3 + 2 and 2 + 2 + 1 of five, 5 splits clipped to the 3 chunks there are; twice; equal to the gathered kernel under the same split"""
    for g in IC.patch_split_pair(cs, 1680 + cs):
        a, need = _run(g, knobs=dict(ig_splits=forced))
        b, _ = _run(g, knobs=dict(ig_splits=forced))
        c, _ = _run(g, knobs=dict(ig_splits=forced, ig_patch=0))
        assert need == _slab_bytes(g, 64, len(chunks), patch=True), need
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("e", IC.EPILOGUES, ids=IC.epi_id)
@pytest.mark.parametrize("base", IC.EPI_BASES, ids=lambda b: b[0])
def test_epilogue(base, e):
    """igemm_epilogue.inc in the plain-rows kernels on one stage (64-wide, and 128-wide: the unpipelined EPI_PIPE == false one), behind the parity
    classes, in the patch kernel and behind the 128-wide split-K seam"""
    _run(IC.epi_geo(base, e), e, knobs=base[3])


@pytest.mark.parametrize("bias", [None, "bf16"])
@pytest.mark.parametrize("S", IC.SLABS)
def test_column_slabs(S, bias):
    _run(IC.SLAB_GEO, IC.Epi(False, bias, None, False, False, IC.ACT_NONE, IC.GATE_NONE), slab=S)
    _run(IC.SLAB_GEO, IC.Epi(True, bias, None, False, False, IC.ACT_RELU, IC.GATE_NONE), knobs=dict(ig_bn=128, ig_nst=1), slab=S)


@pytest.mark.parametrize("g,kn", [(IC.PLAIN[2], dict(ig_bn=128, ig_nst=1)), (IC.PATCH[13][0], dict()), (IC.PCLS[0], dict())], ids=lambda v: v.name if isinstance(v, IC.Geo) else _kid(v))
def test_gate_pointer_is_ignored_under_gate_mode_none(g, kn):
    """PD_IG_GATE_NONE with gate != NULL: the result of the ungated launch (the gate's buffer holds values whose GELU' is far from 1)"""
    lib, L = _libs()
    e = IC.Epi(False, "f32", None, False, False, IC.ACT_RELU, IC.GATE_NONE)
    p = _Problem(g, e)
    gate = _in(SC.relu_mask_operand((p.M, p.n), 77))
    p.d.gate, p.d.gate_mode = gate.ptr, IC.GATE_NONE
    with _knobs(kn):
        a, _ = _launch(p, g.name + " gate pointer under PD_IG_GATE_NONE")
        b, _ = _launch(_Problem(g, e), g.name + " no gate")
    assert torch.equal(a, b)


def test_sequence_of_three_problems_shares_one_workspace():
    """pd_igemm_bf16_seq: a split plain-rows problem, a patch problem with a chunk split and a parity-class problem back to back on ONE workspace
    of exactly pd_igemm_bf16_seq_workspace_bytes"""
    lib, L = _libs()
    ps = [_Problem(g, e) for g, e in IC.SEQ]
    arr = (lib.struct("PdIgemm") * len(ps))()
    for i, p in enumerate(ps):
        ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(p.d), ctypes.sizeof(p.d))
    singles = [L.pd_igemm_bf16_workspace_bytes(ctypes.byref(p.d)) for p in ps]
    need = L.pd_igemm_bf16_seq_workspace_bytes(arr, len(ps))
    assert singles == [_slab_bytes(IC.SEQ[0][0], 64, 2), _slab_bytes(IC.SEQ[1][0], 64, 3, patch=True), 0] and need == max(singles)
    ws = _igemm_workspace(need)
    lib.check(L.pd_igemm_bf16_seq(arr, len(ps), ws.ptr, need, lib.current_stream()))
    torch.cuda.synchronize()
    assert ws.intact() and not ws.t[0, :TICKET_WORDS].any()
    for p in ps:
        p.check("sequence: " + p.g.name)
    for p in ps:                                                # one byte short of the LARGEST need: the patch problem (the second) is refused,
        p.out.raw.fill_(p.out.fill)                             # nothing from it on is launched; the first one, whose need is met, has run
    assert L.pd_igemm_bf16_seq(arr, len(ps), ws.ptr, need - 1, lib.current_stream()) == PD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert ps[1].out.untouched() and ps[2].out.untouched() and not ws.t[0, :TICKET_WORDS].any()
    ps[0].check("sequence, refused at its second problem: " + ps[0].g.name)


def test_grouped_filter_transposes():
    """one launch, four filters (9 and 1 taps, 1 x 3, 3 x 1, 2 x 1, 1 x 1 blocks of 64 x 64), two with the frozen-BN scale folded in; every destination
    a window of its own with sentinels between and around"""
    lib, L = _libs()
    Desc = lib.struct("PdFilterTranspose")
    n = len(IC.TRANSPOSES)
    descs, bufs = (Desc * n)(), []
    for i, (co, taps, ci, _) in enumerate(IC.TRANSPOSES):
        w, s = IC.transpose_operands(i)
        gw, gs, gd = _in(w), (_in(s) if s is not None else None), _out(co * taps * ci)
        d = descs[i]
        d.src, d.dst, d.scale, d.co, d.taps, d.ci = gw.ptr, gd.ptr, (gs.ptr if gs else None), co, taps, ci
        bufs.append((w, s, gw, gs, gd))
    nbytes = L.pd_filter_transpose_table_bytes(n)
    assert nbytes > 0 and L.pd_filter_transpose_table_bytes(2 * n) == 2 * nbytes
    host, table = torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    lib.check(L.pd_filter_transpose_grouped(descs, n, host.data_ptr(), table.data_ptr(), lib.current_stream()))
    torch.cuda.synchronize()
    for i, (w, s, gw, gs, gd) in enumerate(bufs):
        want = IC.ref_transpose(w, s)
        assert torch.equal(SC.bits(gd.t.view(want.shape).cpu()), SC.bits(want)), f"filter {i} {IC.TRANSPOSES[i]}"
        assert gd.intact(), f"filter {i}: a store outside its destination"
    snaps = [b[4].snapshot() for b in bufs]
    assert L.pd_filter_transpose_grouped(descs, 0, host.data_ptr(), table.data_ptr(), lib.current_stream()) == PD_ERR_INVALID_ARG       # count = 0
    assert L.pd_last_error().decode().startswith("pd_filter_transpose_grouped")
    descs[1].ci = 96
    assert L.pd_filter_transpose_grouped(descs, n, host.data_ptr(), table.data_ptr(), lib.current_stream()) == PD_ERR_INVALID_ARG
    assert L.pd_filter_transpose_grouped(None, n, host.data_ptr(), table.data_ptr(), lib.current_stream()) == PD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all(b[4].same_as(s) for b, s in zip(bufs, snaps))


# ------------------------------------------------------------------------------------------------ pd_igemm_bf16: argument checks
def _refused(p, ws_ptr, ws_bytes, what):
    _, L = _libs()
    assert L.pd_igemm_bf16(ctypes.byref(p.d), ws_ptr, ws_bytes, _libs()[0].current_stream()) == PD_ERR_INVALID_ARG, what
    assert L.pd_last_error().decode().startswith("pd_igemm_bf16"), (what, L.pd_last_error().decode())
    torch.cuda.synchronize()
    assert p.out.untouched(), what + ": refused, but the output was written"


def test_igemm_refuses_bad_arguments_and_launches_nothing():
    lib, L = _libs()
    g = IC.FWD[0]                                               # 3 x 3 stride 2, 9 x 11 -> 5 x 6 (an odd result grid), 64 -> 64
    p = _Problem(g)
    addend = _in(SC.ints((IC.rows_of(g), 64), SC.ADDEND, 5))
    fields = [f for f, _ in p.d._fields_]
    good = {f: getattr(p.d, f) for f in fields}
    bad = {"null src": dict(src=None), "null w": dict(w=None), "null out": dict(out=None), "cs = 96": dict(cs=96), "n = 96": dict(n=96),
           "k = 5": dict(k=5, pad=2), "stride = 3": dict(stride=3), "pad != k / 2": dict(pad=0), "pad = 2": dict(pad=2), "batch = 0": dict(batch=0),
           "ho = 0": dict(ho=0), "wo = 0": dict(wo=0), "hs = 0": dict(hs=0), "ws = 0": dict(ws=0),
           "RES_UP2 on an odd grid": dict(res=addend.ptr, res_mode=IC.RES_UP2)}
    assert IC.dims(g)["ho"] % 2 == 1
    for what, change in bad.items():
        for f, v in dict(good, **change).items():
            setattr(p.d, f, v)
        _refused(p, None, 0, what)
        assert L.pd_igemm_bf16_workspace_bytes(ctypes.byref(p.d)) == -1, what
    for f, v in good.items():
        setattr(p.d, f, v)
    _launch(p, "the unchanged problem is accepted")

    p = _Problem(IC.SLAB_GEO, slab=128)                         # n = 256
    addend = _in(SC.ints((p.M, p.n), SC.ADDEND, 6))
    for what, change in {"out_col_slab = 96": dict(out_col_slab=96), "out_col_slab = 384 does not divide n": dict(out_col_slab=384),
                         "out_col_slab with res": dict(res=addend.ptr), "out_col_slab with res2": dict(res2=addend.ptr),
                         "out_col_slab with gate": dict(gate=addend.ptr, gate_mode=IC.GATE_RELU), "out_col_slab with out_pre": dict(out_pre=addend.ptr)}.items():
        q = _Problem(IC.SLAB_GEO, slab=128)
        for f, v in change.items():
            setattr(q.d, f, v)
        _refused(q, None, 0, what)
    _launch(p, "the slab problem is accepted")

    with _knobs(dict(ig_splits=2)):                             # a split problem without its workspace
        p = _Problem(IC.SPLIT_GEO)
        need = L.pd_igemm_bf16_workspace_bytes(ctypes.byref(p.d))
        ws = _igemm_workspace(need)
        _refused(p, None, need, "null workspace")
        _refused(p, ws.ptr, need - 1, "workspace one byte short")
        _refused(p, ws.ptr, 0, "workspace of no bytes")
        assert ws.intact() and not ws.t[0, :TICKET_WORDS].any() and bool((ws.t[0, TICKET_WORDS:] == ws.fill).all())
        _launch(p, "the split problem with its workspace", ws)


# ------------------------------------------------------------------------------------------------ pd_wgrad_bf16
def _wg_problem(c, row_scale, db, dw_f32):
    """descriptor + buffers: ldy = n + 8, ldx = k + 16, ldw = k + 4 (bf16) / k + 12 (fp32): no multiple of 8 — dW is written element by element"""
    lib, _ = _libs()
    dy, x, rs, base = IC.wg_operands(c)
    gdy, gx = SC.Guarded.of(dy, SC.NAN16, DEV, pad=8), SC.Guarded.of(x, SC.NAN16, DEV, pad=16)
    gdw = SC.Guarded(c.N, c.K, F32 if dw_f32 else BF16, SC.SENTINEL32 if dw_f32 else SC.SENTINEL16, DEV, pad=12 if dw_f32 else 4)
    grs = _in(rs) if row_scale else None
    gdb = _out(c.N, F32) if db else None
    if db:
        gdb.t[0].copy_(base)
    assert gdy.ld > c.N and gx.ld > c.K and gdw.ld > c.K and gdw.ld % 8 == 4
    d = lib.struct("PdWgrad")()
    d.dy, d.x, d.dw, d.db, d.row_scale = gdy.ptr, gx.ptr, gdw.ptr, (gdb.ptr if db else None), (grs.ptr if row_scale else None)
    d.m, d.n, d.k, d.ldy, d.ldx, d.ldw, d.dw_f32 = c.M, c.N, c.K, gdy.ld, gx.ld, gdw.ld, int(dw_f32)
    return d, (gdy, gx, grs), gdw, gdb


def _wg_check(c, row_scale, db, dw_f32, gdw, gdb, what):
    dy, x, rs, base = IC.wg_operands(c)
    ref = IC.ref_wgrad(c, dy, x, rs if row_scale else None)
    if dw_f32:
        assert torch.equal(SC.bits(gdw.t.cpu()), SC.bits(ref.float())), what + ": fp32 dW differs from the float64 reference"
    else:
        _assert_exact(gdw.t, ref, what)
    assert gdw.intact(), what + ": a store outside dW [N, K]"
    if db:
        assert torch.equal(SC.bits(gdb.t[0].cpu()), SC.bits(IC.ref_db(dy, base).float())), what + ": dB is not base + column sums"
        assert gdb.intact(), what + ": a store outside dB [N]"
    return SC.bits(gdw.t.cpu()), (SC.bits(gdb.t.cpu()) if db else None)


def _wg_workspace(nbytes):
    """exactly nbytes of sentinel: the first 16 KB must come back untouched"""
    assert nbytes > TICKET_WORDS * 4 and nbytes % 4 == 0
    return _out(nbytes // 4, I32)


@pytest.mark.parametrize("splits", IC.WG_SPLITS)
@pytest.mark.parametrize("nst", IC.WG_NST)
@pytest.mark.parametrize("c", IC.WGRAD, ids=IC.wg_id)
def test_weight_gradient(c, nst, splits):
    """wgrad_bf16<1 | 2> unsliced and with wgrad_bf16_reduce behind 2, 3 and 5 (7 asked for) slices; bf16 and fp32 results, row scale, dB onto a
    nonzero base; two runs bit-identical"""
    lib, L = _libs()
    slices, _ = IC.wg_plan(c, splits)
    with _knobs(dict(wg_nst=nst, wg_splits=splits)):
        for row_scale, db, dw_f32 in IC.WG_OPTIONS:
            what = f"{IC.wg_id(c)} nst={nst} splits={splits} row_scale={row_scale} db={db} f32={dw_f32}"
            runs = []
            for _ in range(2):
                d, ins, gdw, gdb = _wg_problem(c, row_scale, db, dw_f32)
                need = L.pd_wgrad_bf16_workspace_bytes(ctypes.byref(d))
                assert need == (TICKET_WORDS * 4 + IC.wg_tiles(c) * slices * (IC.TILE * IC.TILE + IC.TILE) * 4 if slices > 1 else 0), (what, need)
                ws = _wg_workspace(need) if need else None
                lib.check(L.pd_wgrad_bf16(ctypes.byref(d), ws.ptr if need else None, need, lib.current_stream()))
                torch.cuda.synchronize()
                if need:
                    assert ws.intact(), what + ": a store behind the workspace"
                    assert bool((ws.t[0, :TICKET_WORDS] == ws.fill).all()), what + ": the first 16 KB of the workspace were written"
                runs.append(_wg_check(c, row_scale, db, dw_f32, gdw, gdb, what))
            assert torch.equal(runs[0][0], runs[1][0]) and (not db or torch.equal(runs[0][1], runs[1][1])), what + ": two runs differ"


def test_weight_gradient_sequence_equals_the_single_launches():
    """pd_wgrad_bf16_seq (wgrad_bf16_reduce_grouped): five problems, three of them sliced, both result types, one workspace of exactly
    pd_wgrad_bf16_seq_workspace_bytes; count = 0 and count = 9 are refused"""
    lib, L = _libs()
    with _knobs(dict(wg_splits=IC.WGRAD_SEQ_SPLITS)):
        probs = [(c, f32) + _wg_problem(c, i % 2 == 0, i != 3, f32) for i, (c, f32) in enumerate(IC.WGRAD_SEQ)]
        arr = (lib.struct("PdWgrad") * 9)()
        for i, pr in enumerate(probs):
            ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(pr[2]), ctypes.sizeof(pr[2]))
        singles = [L.pd_wgrad_bf16_workspace_bytes(ctypes.byref(pr[2])) for pr in probs]
        need = L.pd_wgrad_bf16_seq_workspace_bytes(arr, 5)
        assert sum(s > 0 for s in singles) == 3 and need == TICKET_WORDS * 4 + sum(s - TICKET_WORDS * 4 for s in singles if s)
        ws = _wg_workspace(need)
        for count in (0, 9):
            assert L.pd_wgrad_bf16_seq(arr, count, ws.ptr, need, lib.current_stream()) == PD_ERR_INVALID_ARG
            assert L.pd_wgrad_bf16_seq_workspace_bytes(arr, count) == -1
        assert L.pd_wgrad_bf16_seq(arr, 5, ws.ptr, need - 1, lib.current_stream()) == PD_ERR_INVALID_ARG
        assert L.pd_wgrad_bf16_seq(arr, 5, None, need, lib.current_stream()) == PD_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert all(pr[4].untouched() for pr in probs) and ws.untouched()
        lib.check(L.pd_wgrad_bf16_seq(arr, 5, ws.ptr, need, lib.current_stream()))
        torch.cuda.synchronize()
        assert ws.intact() and bool((ws.t[0, :TICKET_WORDS] == ws.fill).all())
        for i, (c, f32, d, ins, gdw, gdb) in enumerate(probs):
            got = _wg_check(c, i % 2 == 0, i != 3, f32, gdw, gdb, f"sequence problem {i} {IC.wg_id(c)}")
            d1, _, gdw1, gdb1 = _wg_problem(c, i % 2 == 0, i != 3, f32)
            ws1 = _wg_workspace(singles[i]) if singles[i] else None
            lib.check(L.pd_wgrad_bf16(ctypes.byref(d1), ws1.ptr if ws1 else None, singles[i], lib.current_stream()))
            torch.cuda.synchronize()
            assert torch.equal(got[0], SC.bits(gdw1.t.cpu())) and (gdb is None or torch.equal(got[1], SC.bits(gdb1.t.cpu())))


def test_weight_gradient_refuses_bad_arguments_and_launches_nothing():
    lib, L = _libs()
    c = IC.WGRAD[4]                                             # (257, 64, 264)
    with _knobs(dict(wg_splits=2)):
        d, ins, gdw, gdb = _wg_problem(c, True, True, False)
        need = L.pd_wgrad_bf16_workspace_bytes(ctypes.byref(d))
        ws = _wg_workspace(need)
        good = {f: getattr(d, f) for f, _ in d._fields_}
        bad = {"n % 8": dict(n=60), "k % 8": dict(k=260), "ldy % 8": dict(ldy=good["ldy"] + 4), "ldx % 8": dict(ldx=good["ldx"] + 4), "ldy < n": dict(ldy=56),
               "ldx < k": dict(ldx=256), "ldw < k": dict(ldw=256), "dy 8 bytes off": dict(dy=good["dy"] + 8), "x 2 bytes off": dict(x=good["x"] + 2),
               "dw 1 byte off": dict(dw=good["dw"] + 1), "m = 0": dict(m=0), "null dy": dict(dy=None), "null x": dict(x=None), "null dw": dict(dw=None)}
        for what, change in bad.items():
            for f, v in dict(good, **change).items():
                setattr(d, f, v)
            assert L.pd_wgrad_bf16(ctypes.byref(d), ws.ptr, need, lib.current_stream()) == PD_ERR_INVALID_ARG, what
            assert L.pd_last_error().decode().startswith("pd_wgrad_bf16"), what
            assert L.pd_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == -1, what
        for f, v in good.items():
            setattr(d, f, v)
        for what, (ptr, nbytes) in {"null workspace": (None, need), "workspace one byte short": (ws.ptr, need - 1)}.items():
            assert L.pd_wgrad_bf16(ctypes.byref(d), ptr, nbytes, lib.current_stream()) == PD_ERR_INVALID_ARG, what
        d.dw_f32, d.dw = 1, good["dw"] + 2                      # an fp32 result needs 4-byte alignment
        assert L.pd_wgrad_bf16(ctypes.byref(d), ws.ptr, need, lib.current_stream()) == PD_ERR_INVALID_ARG
        d.dw_f32, d.dw = 0, good["dw"]
        torch.cuda.synchronize()
        assert gdw.untouched() and ws.untouched() and bool((gdb.raw[gdb.outside] == gdb.fill).all())
        lib.check(L.pd_wgrad_bf16(ctypes.byref(d), ws.ptr, need, lib.current_stream()))            # the unchanged problem is accepted (ldw = k + 4)
        torch.cuda.synchronize()
        _wg_check(c, True, True, False, gdw, gdb, "the unchanged problem")
