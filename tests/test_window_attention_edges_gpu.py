"""GPU tests of the Swin window-attention kernels (csrc/window_attention.hip) that compare EVERY ELEMENT of out, lse (base 2), dq, dk, dv and
dtable with the fp64 oracle of tests/window_attention_cases.py under its per-element bounds (derived there from the kernels' rounding points;
tests/test_window_attention_cases_cpu.py proves that they can be met and that each case is what it is named for).  Calls go through fwd_raw /
bwd_raw.  All cases have heads * B_ <= 256 workgroups, for which chunk_of (windows per workgroup) gives 1 in both directions; the chunk sweep
forces the other values through pd_debug_set("wattn_chunk", c).

Which case reaches what:

  case / test              | heads, images x H x W, shift | reaches
  -------------------------+------------------------------+--------------------------------------------------------------------------------
  one_window               |  1, 1 x 12 x 12, 0           | B_ = 1, no mask; every table entry from its 1 .. 144 pairs, the corners from one
  mixed_flags              |  3, 1 x 24 x 24, 6           | wattn_*<MASK>: nW = 4, window 0 unflagged (mask arithmetic skipped), 1 .. 3 flagged
  ragged_masked            |  2, 2 x 25 x 40, 6           | padded 36 x 48 grid, nW = 12, B_ = 24: b % nW over two images, 9 region labels
  wide_masked              |  2, 1 x 24 x 24, 6           | additive -100 (a cross-region key still wins its row), not -inf; |lse| in the hundreds
  peaky                    |  4, 1 x 12 x 12, 0           | max subtraction; exp2(t - lse) of near one-hot rows in both backward phases
  bias_only_plain/_shifted |  2, 1 x 24 x 24, 0 / 6       | q = k = 0: the table index map alone, forward and dtable (dq = dk = 0)
  heads48                  | 48, 1 x 24 x 24, 6           | C = 1536 (Swin-L stage 4): row pitch 3 C, table / dtable stride 48, blockIdx.y up to 47
  chunk sweep, chunk_plain |  2, 7 x 12 x 12, 0           | chunks 1, 2, 3, 5, 8 of B_ = 7: tails of 1, 1, 2, 7 windows; u & 1 buffer parity; dacc over windows
  chunk sweep, chunk_masked|  2, 3 x 24 x 24, 6           | chunks of B_ = 12 (tails 2 and 4): mbits per unit, b % nW across an image inside a chunk,
                           |                              | flagged and unflagged windows in one workgroup
  accumulation             | one_window; chunk_plain at 8 | dtable += gradient (one atomic add per entry: one workgroup per head)
  non-contiguous d_out     | mixed_flags, dO = 1          | WindowAttention12.backward's .contiguous() of an expanded gradient
  bad arguments            |                              | region without win_flags, misaligned qkv / region: PdHipError before any launch

Largest observed |error| / bound on the MI355X, for the next reader (the bounds are those of window_attention_cases.py and do not follow from
these figures): out 0.694 (wide_masked), lse 0.033 (heads48), dq 0.489, dk 0.558 (wide_masked), dv 0.841 (bias_only_plain), dtable 0.574 (heads48);
dtable at a forced chunk against chunk 1: 0.217 of 2^-20 sum |dS| (chunk_masked, chunk 2).  In every case the kernels' ratios equal those of the
fp64 rounding emulation (window_attention_cases.emulate, printed by the CPU test) to three digits on out, dq, dk, dv and dtable: no rounding
point beyond the documented ones shows.  Run with -s to see them ("RATIO ..." lines)."""
import functools

import pytest
import torch

import window_attention_cases as WC

pytestmark = pytest.mark.gpu

NAMED = ["one_window", "mixed_flags", "ragged_masked", "wide_masked", "peaky", "bias_only_plain", "bias_only_shifted", "heads48"]
CHUNKS = (1, 2, 3, 5, 8)


def _lib():
    from partdistillation_amd import lib
    return lib.load()


def _chunk(c):
    assert _lib().pd_debug_set(b"wattn_chunk", int(c)) == 0


@pytest.fixture(autouse=True)
def _reset_knob():
    yield
    _chunk(0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs on the device, the regions the product builds for the case's grid, and the oracle (computed once per case, on the CPU)"""
    from partdistillation_amd.functions import window_attention as wa
    case = WC.build(name)
    regions = wa.shifted_window_regions(case["H"], case["W"], case["shift"], "cuda") if case["shift"] else None
    dev = {n: case[n].cuda() for n in ("qkv", "table", "d_out")}
    return case, dev, regions, WC.oracle_of(case)


def _run(case, dev, regions, dtable=None, d_out=None):
    from partdistillation_amd.functions import window_attention as wa
    out, lse = wa.fwd_raw(dev["qkv"], dev["table"], regions, case["scale"], case["nW"])
    dqkv, dt = wa.bwd_raw(dev["qkv"], dev["table"], regions, out, dev["d_out"] if d_out is None else d_out, lse, case["scale"], case["nW"],
                          dtable=dtable)
    dq, dk, dv = WC.split_dqkv(dqkv)
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16 and lse.dtype == torch.float32 and dt.dtype == torch.float32
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dt=dt, dqkv=dqkv)


def _within(got, ref, what, extra=None):
    r = WC.ratios(got, ref, extra)
    print(f"RATIO {what}: " + " ".join(f"{n} {r[n]:.3f}" for n in WC.TENSORS))
    assert all(x <= 1.0 for x in r.values()), f"{what}: |error| / bound per tensor {r}"


@pytest.mark.parametrize("name", NAMED)
def test_every_element_against_the_oracle(name):
    case, dev, regions, ref = _case(name)
    _within(_run(case, dev, regions), ref, name)


@pytest.mark.parametrize("name", ["chunk_plain", "chunk_masked"])
def test_chunked_walk_equals_one_window_per_workgroup(name):
    """out, lse and dqkv do not depend on the chunk at all (bit-identical); dtable sums the same fp32 dS in another order: within
    2^-20 * sum |dS| of the chunk-1 result, and within the oracle's bound like everything else"""
    case, dev, regions, ref = _case(name)
    _chunk(1)
    base = _run(case, dev, regions)
    _within(base, ref, f"{name} chunk 1")
    for c in CHUNKS[1:]:
        _chunk(c)
        got = _run(case, dev, regions)
        for n in ("out", "lse", "dqkv"):
            assert torch.equal(got[n], base[n]), f"{name}: {n} at chunk {c} differs from chunk 1"
        d = ((got["dt"].double() - base["dt"].double()).abs().cpu() / (2.0 ** -20 * ref["a_dt"] + WC.FLOOR)).max().item()
        print(f"RATIO {name} chunk {c} vs chunk 1: dt {d:.3f}")
        assert d <= 1.0, f"{name}: dtable at chunk {c} is {d:.3f} x (2^-20 sum |dS|) away from chunk 1"
        _within(got, ref, f"{name} chunk {c}")


def test_chunk_knob_takes_0_to_8_only():
    from partdistillation_amd import lib
    for bad in (-1, 9, 64):
        assert _lib().pd_debug_set(b"wattn_chunk", bad) != 0 and b"wattn_chunk" in _lib().pd_last_error()
        with pytest.raises(lib.PdHipError):
            lib.check(_lib().pd_debug_set(b"wattn_chunk", bad))
    for ok in range(9):
        assert _lib().pd_debug_set(b"wattn_chunk", ok) == 0


@pytest.mark.parametrize("name,chunk", [("one_window", 0), ("chunk_plain", 8)])
def test_dtable_is_accumulated_into(name, chunk):
    """bwd_raw(..., dtable = prefill) returns prefill + gradient.  Both cases run ONE workgroup per head, so every entry receives exactly one
    atomic add: its rounding is half an ulp of the result, at most an ulp of the prefill plus 2^-24 |gradient| (inside the 2^-20 term)"""
    case, dev, regions, ref = _case(name)
    g = torch.Generator().manual_seed(7)
    prefill = torch.randn(WC.TBL, case["heads"], generator=g)
    _chunk(chunk)
    got = _run(case, dev, regions, dtable=prefill.cuda())
    ulp = 2.0 ** (torch.floor(torch.log2(prefill.double().abs())) - 23)
    want = dict(ref, dt=prefill.double() + ref["dt"])
    _within(got, want, f"{name} accumulate", extra={"dt": ulp})
    assert not torch.equal(got["dt"].cpu(), prefill)


def test_non_contiguous_gradient_of_ones():
    """.float().sum().backward() hands the Function an expanded gradient of ones (stride 0); the same through autograd.grad with the
    expanded tensor itself.  Both equal the oracle with dO = 1."""
    from partdistillation_amd.functions import window_attention as wa
    case, dev, regions, _ = _case("mixed_flags")
    ones = torch.ones_like(case["d_out"])
    ref = WC.oracle(case["qkv"], case["table"], ones, case["H"], case["W"], case["shift"], case["scale"])
    qkv, table = dev["qkv"].clone().requires_grad_(), dev["table"].clone().requires_grad_()
    out = wa.window_attention(qkv, table, regions, case["scale"], case["nW"])
    out.float().sum().backward()
    expanded = torch.ones((), dtype=torch.bfloat16, device="cuda").expand(out.shape)
    assert not expanded.is_contiguous()
    dqkv2, dt2 = torch.autograd.grad(wa.window_attention(qkv, table, regions, case["scale"], case["nW"]), (qkv, table), expanded)
    lse = WC.LOG2E * torch.logsumexp(sum(WC.scores(case["qkv"], case["table"], case["H"], case["W"], case["shift"], case["scale"])[3:5]), -1)
    for what, dqkv, dt in (("sum().backward()", qkv.grad, table.grad), ("expanded grad_outputs", dqkv2, dt2)):
        dq, dk, dv = WC.split_dqkv(dqkv)
        _within(dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv, dt=dt), ref, "dO = 1, " + what)


def test_rejects_region_without_flags_and_misaligned_bases():
    """each is PdHipError from the argument check, before any launch: a prefilled dtable is untouched, the device stays healthy"""
    from partdistillation_amd import lib
    from partdistillation_amd.functions import window_attention as wa
    case, dev, regions, _ = _case("mixed_flags")
    B_, heads, nW = dev["qkv"].shape[0], case["heads"], case["nW"]
    out, lse = wa.fwd_raw(dev["qkv"], dev["table"], regions, case["scale"], nW)
    prefill = torch.full((WC.TBL, heads), 3.0, device="cuda")

    def both(qkv, regs, match):
        with pytest.raises(lib.PdHipError, match=match):
            wa.fwd_raw(qkv, dev["table"], regs, case["scale"], nW)
        with pytest.raises(lib.PdHipError, match=match):
            wa.bwd_raw(qkv, dev["table"], regs, out, dev["d_out"], lse, case["scale"], nW, dtable=prefill)

    both(dev["qkv"], (regions[0], None), "go together")
    flat = torch.zeros(dev["qkv"].numel() + 8, dtype=torch.bfloat16, device="cuda")
    off = flat[1:1 + dev["qkv"].numel()].view_as(dev["qkv"])
    off.copy_(dev["qkv"])
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    both(off, regions, "16-byte aligned")
    rbuf = torch.zeros(regions[0].numel() + 4, dtype=torch.uint8, device="cuda")
    roff = rbuf[1:1 + regions[0].numel()].view_as(regions[0])
    roff.copy_(regions[0])
    assert roff.is_contiguous() and roff.data_ptr() % 4 == 1
    both(dev["qkv"], (roff, regions[1]), "4-byte aligned")
    torch.cuda.synchronize()
    assert (prefill == 3.0).all()


def test_two_runs_are_bit_identical():
    case, dev, regions, _ = _case("ragged_masked")
    a, b = _run(case, dev, regions), _run(case, dev, regions)
    for n in ("out", "lse", "dqkv"):
        assert torch.equal(a[n], b[n]), n
