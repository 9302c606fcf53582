"""GPU tests of the masked-attention kernels (csrc/attention.hip) where their -inf bookkeeping and their max subtraction are at work:
structured masks with dead tiles, key halves, chunks and rows, logits far beyond what exp() holds in fp32, partial last chunks, no keys at all.
Every case compares o, lse, dq, dk and dv — every element — with the fp64 reference of tests/attention_cases.py (whose cases
tests/test_attention_cases_cpu.py proves to be what they are named for).

Which case reaches which kernel and chunk size (kc = keys per workgroup):

  path, kc                      | reached by
  ------------------------------+----------------------------------------------------------------------------------------
  mfma fwd, 256, single chunk   | MFMA shapes Lk = 200, 256 (no combine launch)
  mfma fwd, 64                  | MFMA shapes B=1, H=2, Lk = 321 .. 1025 (6 chunks at 321, the last one key)
  mfma fwd, 128                 | MFMA shape  B=2, H=8, Lk = 4097 (33 chunks, the last one key)
  mfma fwd, 256                 | MFMA shape  B=4, H=8, Lk = 4097 (17 chunks, the last one key)
  attn_fwd_combine              | every multi-chunk case above (tail loop at 6 chunks, 8-wide loop + tail at 17 and 33) and the scalar cases
  mfma bwd, 128                 | Lk = 321, 322 automatically (last chunk 65 / 66 keys: 3 tiles, one of them 1 / 2 keys; wave 3 idle), 200, 256
  mfma bwd, 256                 | Lk = 513 forced (last chunk one key: waves 1..3 idle), Lk = 4097 with B=2 automatically
  mfma bwd, 512                 | Lk = 1025 forced (last chunk one key), Lk = 4097 with B=4 automatically
  mfma, unaligned mask4         | Lk = 321, 322 (322 is not a multiple of 4 and not odd), 513, 1025, 4097
  scalar fwd (256-key chunks)   | SCALAR shapes: fp32 and bf16 at Lq=129, Lk=577 (3 chunks, the last 65 keys; the second query pass has one query),
  scalar dq (512-key chunks)    |   bf16 with attn_scalar=1 at Lq=40, Lk=321, fp32 at Lq=5, Lk=63 (one partial tile)
  scalar dkv (256-key groups)   |   (the same cases: 3 / 2 / 1 workgroups per (image, head), 32-query stages with a partial last stage)

Tolerances are the existing test's (tests/test_attention_gpu.py) as a fraction of each reference tensor's max-abs: 1e-4 for fp32, 2e-2 for
bf16, on o, dq, dk, dv; lse is an fp32 sum of fp32 scores on every path: 1e-4 * max(1, |lse|) for both dtypes."""
import functools

import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu

FRAC = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
LSE_TOL = 1e-4


def _lib():
    from partdistillation_amd import lib
    return lib.load()


@pytest.fixture(autouse=True)
def _reset_knobs():
    yield
    assert _lib().pd_debug_set(b"attn_scalar", 0) == 0 and _lib().pd_debug_set(b"attn_bwd_kc", 0) == 0


def _knobs(scalar, bwd_kc):
    assert _lib().pd_debug_set(b"attn_scalar", int(scalar)) == 0 and _lib().pd_debug_set(b"attn_bwd_kc", int(bwd_kc)) == 0


# keys per workgroup of attn_fwd_mfma, the rule of mfma_fwd_chunk (csrc/attention.hip):
#     kc = 256;  if (Lk > 256) while (kc > 64 && B * H * ceil(Lk / kc) < 512) kc /= 2;
def mfma_fwd_kc(B, H, Lk):
    kc = 256
    if Lk > 256:
        while kc > 64 and B * H * -(-Lk // kc) < 512:
            kc //= 2
    return kc


def test_the_shapes_reach_the_chunk_sizes_the_table_claims():
    assert [mfma_fwd_kc(1, 2, 200), mfma_fwd_kc(1, 2, 256), mfma_fwd_kc(1, 2, 321), mfma_fwd_kc(2, 8, 4097), mfma_fwd_kc(4, 8, 4097)] == [256, 256, 64, 128, 256]
    assert [-(-321 // 64), 321 - 5 * 64, -(-4097 // 128), 4097 - 32 * 128, -(-4097 // 256), 4097 - 16 * 256] == [6, 1, 33, 1, 17, 1]


def _mask_for(masking, B, Lq, Lk, kc):
    if masking == "none":
        return None
    if masking == "mixed":
        return AC.mixed(B, Lq, Lk, kc=kc)
    assert masking == "alternate_chunks"
    return AC.alternate_chunks(B, Lq, Lk, kc=kc)


@functools.lru_cache(maxsize=4)
def _case(kind, masking, Lq, Lk, B, H, dtype, kc):
    """inputs on the device and the fp64 reference of all five results, computed once per case"""
    q, k, v, d_o = AC.unit_inputs(Lq, Lk, B, H, dtype) if kind == "unit" else AC.wide_inputs(kind, Lq, Lk, B, H, dtype)
    mask = _mask_for(masking, B, Lq, Lk, kc)
    q, k, v, d_o = (a.cuda() for a in (q, k, v, d_o))
    mask = mask.cuda() if mask is not None else None
    qr, kr, vr = (a.double().requires_grad_() for a in (q, k, v))
    ro, rlse = AC.reference(qr, kr, vr, mask, H)
    rq, rk, rv = torch.autograd.grad(ro, (qr, kr, vr), d_o.double())
    dead = mask.all(-1) if mask is not None else torch.zeros(B, Lq, dtype=torch.bool, device="cuda")
    return (q, k, v, d_o, mask), dict(o=ro.detach(), lse=rlse.detach(), dq=rq, dk=rk, dv=rv), dead


def _kernels(q, k, v, d_o, mask, H):
    """o, lse, dq, dk, dv of pd_attn_fwd_d32_ld / pd_attn_bwd_d32_ld in the layouts of the reference"""
    from partdistillation_amd.functions.attention import attn_bwd_raw, attn_fwd_raw
    Lq, B, C = q.shape
    Lk = k.shape[0]
    m8 = mask.view(torch.uint8) if mask is not None else None
    q2, k2, v2, g2 = q.reshape(Lq * B, C), k.reshape(Lk * B, C), v.reshape(Lk * B, C), d_o.reshape(Lq * B, C)
    o, lse = attn_fwd_raw(q2, k2, v2, m8, B, H, AC.SCALE)
    dq, dk, dv = attn_bwd_raw(q2, k2, v2, m8, o, g2, lse, B, H, AC.SCALE)
    return dict(o=o.view(Lq, B, C), lse=lse, dq=dq.view(Lq, B, C), dk=dk.view(Lk, B, C), dv=dv.view(Lk, B, C))


def _compare(got, ref, dead, dtype, what, format_error=None):
    """every element of o, dq, dk, dv within FRAC of the reference tensor's max-abs (or, where `format_error` names the tensor, within 4 x
    that deviation if it is the larger: see _run); lse within LSE_TOL * max(1, |lse|) and -inf exactly where the
    reference is; blocked rows exactly o = 0, lse = -inf, dq = 0; everything else finite"""
    bad = []
    format_error = format_error or {}
    for name in ("o", "dq", "dk", "dv"):
        g, r = got[name].double(), ref[name]
        assert g.shape == r.shape and got[name].dtype == dtype
        if not torch.isfinite(g).all():
            bad.append(f"{name}: {int((~torch.isfinite(g)).sum())} non-finite values")
            continue
        err, scale = (g - r).abs().max().item(), r.abs().max().item()
        bound = max(FRAC[dtype] * scale, 4.0 * format_error.get(name, 0.0))
        print(f"{what} {name}: max abs err {err:.3e}, bound {bound:.3e} ({FRAC[dtype]} * {scale:.3e}, format error {format_error.get(name, 0.0):.3e})")
        if not err <= bound:
            bad.append(f"{name}: max abs err {err:.3e} > {bound:.3e} ({FRAC[dtype]} * {scale:.3e}, format error {format_error.get(name, 0.0):.3e})")
    g, r = got["lse"].double(), ref["lse"]
    assert g.shape == r.shape and got["lse"].dtype == torch.float32
    inf = torch.isneginf(r)
    if not torch.equal(torch.isneginf(g), inf):
        bad.append(f"lse: -inf at {int(torch.isneginf(g).sum())} places, the reference at {int(inf.sum())}")
    elif not torch.isfinite(g[~inf]).all():
        bad.append("lse: non-finite values")
    else:
        excess = ((g - r).abs() - LSE_TOL * r.abs().clamp(min=1.0))[~inf]
        print(f"{what} lse: max abs err {(g - r).abs()[~inf].max().item():.3e}, max |lse| {r[~inf].abs().max().item():.3e}")
        if excess.numel() and excess.max().item() > 0:
            bad.append(f"lse: error exceeds {LSE_TOL} * max(1, |lse|) by {excess.max().item():.3e}")
    assert torch.equal(inf, dead[:, None].expand_as(inf)), "the reference's blocked rows are not the mask's"
    rows = dead.t()                                                   # [Lq, B]
    if rows.any():
        for name in ("o", "dq"):
            if not (got[name][rows] == 0).all():
                bad.append(f"{name}: a blocked row is not exactly zero (max abs {got[name][rows].float().abs().max().item():.3e})")
    assert not bad, what + ": " + "; ".join(bad)


def _run(kind, masking, Lq, Lk, B, H, dtype, kc, scalar=0, bwd_kc=0):
    """One case on one path.  Wide-range inputs in bf16 cannot meet 2e-2 on dq (and, where the true gradient is ~0, on dk) on ANY path, and no
    kernel is to blame: the softmax of logits with a standard deviation of 6 is nearly one-hot, so dS = P * (dP - delta) is a difference of
    nearly equal numbers, and delta = rowsum(dO * O) is taken from the o the forward stored in bf16 (2^-9 relative) — times key channel 0,
    which is up to 90 here.  AC.working_precision evaluates the same formulas in plain torch (fp32 throughout, o rounded to bf16, P and dS
    rounded to bf16 on the matrix-core path) and deviates from the fp64 reference on these inputs by
        dq 0.19 .. 0.48 (3 % .. 13 % of max |dq| = 3.4 .. 12.4; 1.5e-5 where the true dq is 4e-15), dk 0.004 .. 0.10 (max |dk| 1.3 .. 14.7)
    (shapes (40, 200), (1, 321), (40, 321), (40, 513), (129, 577), both paths); the kernels' dq error equals that deviation to four digits
    (0.3711 at ascending (40, 200), 0.4453 descending, 0.2119 scrambled).  So for these cases dq and dk are held to
    max(2e-2 * max-abs, 4 x the deviation measured on the same inputs) — 4 x covers summation order and __expf / __logf; o, dv, lse and every
    fp32 case keep the plain bounds."""
    inputs, ref, dead = _case(kind, masking, Lq, Lk, B, H, dtype, kc)
    format_error = None
    if kind != "unit" and dtype == torch.bfloat16:
        w = AC.working_precision(*inputs, H, matrix_core=not scalar and Lq <= 128)
        format_error = {n: (w[n].double() - ref[n]).abs().max().item() for n in ("dq", "dk")}
    _knobs(scalar, bwd_kc)
    got = _kernels(*inputs, H)
    _compare(got, ref, dead, dtype, f"{kind}/{masking} Lq={Lq} Lk={Lk} B={B} H={H} {dtype} scalar={scalar} bwd_kc={bwd_kc}", format_error)


INPUTS = [("unit", "mixed")] + [(kind, masking) for kind in AC.WIDE for masking in ("none", "alternate_chunks")]
INPUT_IDS = [f"{a}-{b}" for a, b in INPUTS]

# matrix-core path (bf16, Lq <= 128): (Lq, Lk, B, H, forced backward kc or 0)
MFMA = [(40, 200, 1, 2, 0), (40, 256, 1, 2, 0),                        # forward: one chunk of 256
        (1, 321, 1, 2, 0), (1, 321, 9, 2, 0), (33, 321, 1, 2, 0), (97, 321, 1, 2, 0), (128, 321, 1, 2, 0),      # forward kc 64; waves without a valid query / partly valid
        # (Lq = 1, B = 9: the single row of image b carries pattern 4b mod 9 — all nine)
        (40, 4097, 2, 8, 0), (40, 4097, 4, 8, 0),                      # forward kc 128 / 256, backward kc 256 / 512
        (40, 322, 1, 2, 0),                                            # Lk % 4 != 0: the byte-wise mask4 route
        (40, 513, 1, 2, 256), (40, 1025, 1, 2, 512),                   # backward kc forced; last chunk = one key
        (33, 321, 1, 2, 256), (33, 321, 1, 2, 512)]


@pytest.mark.parametrize("kind,masking", INPUTS, ids=INPUT_IDS)
@pytest.mark.parametrize("Lq,Lk,B,H,bwd_kc", MFMA)
def test_matrix_core_path(Lq, Lk, B, H, bwd_kc, kind, masking):
    kc = bwd_kc or mfma_fwd_kc(B, H, Lk)                              # chunk size of the masks: the one the kernels cut the keys by
    _run(kind, masking, Lq, Lk, B, H, torch.bfloat16, kc, bwd_kc=bwd_kc)


# scalar paths: (Lq, Lk, B, H, dtype, attn_scalar)
SCALAR = [(129, 577, 2, 2, torch.float32, 0), (129, 577, 2, 2, torch.bfloat16, 0), (40, 321, 1, 2, torch.bfloat16, 1), (5, 63, 2, 2, torch.float32, 0)]


@pytest.mark.parametrize("kind,masking", INPUTS, ids=INPUT_IDS)
@pytest.mark.parametrize("Lq,Lk,B,H,dtype,scalar", SCALAR)
def test_scalar_paths(Lq, Lk, B, H, dtype, scalar, kind, masking):
    _run(kind, masking, Lq, Lk, B, H, dtype, 256, scalar=scalar)      # forward chunks of 256 keys
    if masking != "none" and Lk > 512:
        _run(kind, masking, Lq, Lk, B, H, dtype, 512, scalar=scalar)  # the dq kernel's chunks of 512 keys


@pytest.mark.parametrize("Lq,Lk,B,H,dtype,scalar,bwd_kc", [(40, 321, 1, 2, torch.bfloat16, 0, 0), (40, 513, 1, 2, torch.bfloat16, 0, 256),
                                                            (40, 321, 1, 2, torch.bfloat16, 1, 0), (129, 577, 1, 2, torch.float32, 0, 0)])
def test_backward_takes_an_lse_of_minus_inf_as_a_dead_row(Lq, Lk, B, H, dtype, scalar, bwd_kc):
    """The backward recomputes p = exp(s - lse); lse = -inf marks a row without any open key, whatever the mask says about its keys: the row
    gets dq = 0 and adds nothing to dk / dv (unmasked call, lse and o of rows 3 and Lq-1 overwritten: without the guard p would be exp(+inf))."""
    from partdistillation_amd.functions.attention import attn_bwd_raw, attn_fwd_raw
    q, k, v, d_o = (a.cuda() for a in AC.unit_inputs(Lq, Lk, B, H, dtype, seed=3))
    rows = [3, Lq - 1]
    mask = torch.zeros(B, Lq, Lk, dtype=torch.bool, device="cuda")
    mask[:, rows] = True
    qr, kr, vr = (a.double().requires_grad_() for a in (q, k, v))
    ro, rlse = AC.reference(qr, kr, vr, mask, H)
    rq, rk, rv = torch.autograd.grad(ro, (qr, kr, vr), d_o.double())
    _knobs(scalar, bwd_kc)
    C = H * 32
    q2, k2, v2, g2 = q.reshape(Lq * B, C), k.reshape(Lk * B, C), v.reshape(Lk * B, C), d_o.reshape(Lq * B, C)
    o, lse = attn_fwd_raw(q2, k2, v2, None, B, H, AC.SCALE)
    assert torch.isfinite(lse).all()
    lse[:, :, rows] = float("-inf")
    o.view(Lq, B, C)[rows] = 0
    dq, dk, dv = attn_bwd_raw(q2, k2, v2, None, o, g2, lse, B, H, AC.SCALE)
    got = dict(o=o.view(Lq, B, C), lse=lse, dq=dq.view(Lq, B, C), dk=dk.view(Lk, B, C), dv=dv.view(Lk, B, C))
    _compare(got, dict(o=ro.detach(), lse=rlse.detach(), dq=rq, dk=rk, dv=rv), mask.all(-1), dtype, f"lse=-inf rows Lq={Lq} Lk={Lk} {dtype} scalar={scalar}")


@pytest.mark.parametrize("Lq,Lk,B,H,cols,at,bwd_kc", [(40, 321, 2, 4, 384, 128, 0), (97, 1025, 1, 2, 192, 64, 512)])
def test_strided_keys_and_values_with_dead_chunks(Lq, Lk, B, H, cols, at, bwd_kc):
    """k / v as column slices of wider matrices under a mask with dead tiles, chunks and rows: forward, lse and the three gradients
    bit-identical to the calls on dense copies, and o / lse / gradients equal to those of masked_attention_d32 on the same data"""
    from partdistillation_amd.functions.attention import attn_bwd_raw, attn_fwd_raw, masked_attention_d32
    torch.manual_seed(Lq + Lk)
    C = H * 32
    q = torch.randn(Lq * B, C, device="cuda").bfloat16()
    kw, vw = torch.randn(Lk * B, cols, device="cuda").bfloat16(), torch.randn(Lk * B, cols, device="cuda").bfloat16()
    ks, vs = kw[:, at:at + C], vw[:, at:at + C]
    kd, vd = ks.contiguous(), vs.contiguous()
    mask = AC.mixed(B, Lq, Lk, kc=bwd_kc or mfma_fwd_kc(B, H, Lk)).cuda()
    m8 = mask.view(torch.uint8)
    _knobs(0, bwd_kc)
    o1, l1 = attn_fwd_raw(q, ks, vs, m8, B, H, AC.SCALE)
    o2, l2 = attn_fwd_raw(q, kd, vd, m8, B, H, AC.SCALE)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    d_o = torch.randn_like(o1)
    g1 = attn_bwd_raw(q, ks, vs, m8, o1, d_o, l1, B, H, AC.SCALE)
    g2 = attn_bwd_raw(q, kd, vd, m8, o2, d_o, l2, B, H, AC.SCALE)
    for a, b in zip(g1, g2):
        assert a.is_contiguous() and torch.equal(a, b)
    q3, k3, v3 = (t.view(-1, B, C).clone().requires_grad_() for t in (q, kd, vd))
    o3 = masked_attention_d32(q3, k3, v3, mask, H)
    l3 = o3.grad_fn.saved_tensors[5]
    assert torch.equal(o3.view(-1, C), o1) and torch.equal(l3, l1)
    g3 = torch.autograd.grad(o3, (q3, k3, v3), d_o.view(-1, B, C))
    for a, b in zip(g1, g3):
        assert torch.equal(a, b.view(-1, C))
    # and they are right
    ref_in = [t.detach().double().requires_grad_() for t in (q3, k3, v3)]
    ro, rlse = AC.reference(*ref_in, mask, H)
    rq, rk, rv = torch.autograd.grad(ro, ref_in, d_o.view(-1, B, C).double())
    got = dict(o=o1.view(-1, B, C), lse=l1, dq=g1[0].view(-1, B, C), dk=g1[1].view(-1, B, C), dv=g1[2].view(-1, B, C))
    _compare(got, dict(o=ro.detach(), lse=rlse.detach(), dq=rq, dk=rk, dv=rv), mask.all(-1), torch.bfloat16, f"strided Lq={Lq} Lk={Lk}")


def _dirty(shape, dtype, B, H, Lq, Lk):
    """leave 1.0 in the attention workspace and in the allocator's cached blocks of this size: a result that is not written shows"""
    from partdistillation_amd.functions import attention as A
    A._workspace(B, H, Lq, Lk, torch.device("cuda", torch.cuda.current_device())).fill_(1.0)
    junk = [torch.ones(shape, dtype=dtype, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_keys(dtype):
    """Lk = 0, Lq = 5: every row is a blocked row — o = 0, lse = -inf, dq = 0 (written, not left as allocated), dk / dv empty"""
    from partdistillation_amd.functions.attention import attn_bwd_raw, attn_fwd_raw, masked_attention_d32
    Lq, B, H = 5, 2, 2
    C = H * 32
    q = torch.randn(Lq * B, C, device="cuda").to(dtype)
    k = torch.empty(0, C, device="cuda", dtype=dtype)
    _dirty((Lq * B, C), dtype, B, H, Lq, 0)
    o, lse = attn_fwd_raw(q, k, k, None, B, H, AC.SCALE)
    assert o.shape == q.shape and (o == 0).all() and lse.shape == (B, H, Lq) and torch.isneginf(lse).all()
    _dirty((Lq * B, C), dtype, B, H, Lq, 0)
    dq, dk, dv = attn_bwd_raw(q, k, k, None, o, torch.ones_like(o), lse, B, H, AC.SCALE)
    print("Lk = 0: dq min / max", dq.float().min().item(), dq.float().max().item())
    assert dq.shape == q.shape and (dq == 0).all() and dk.shape == (0, C) and dv.shape == (0, C)
    # the same through autograd, with a (0-key) mask
    q3 = q.view(Lq, B, C).clone().requires_grad_()
    k3 = torch.empty(0, B, C, device="cuda", dtype=dtype, requires_grad=True)
    v3 = torch.empty(0, B, C, device="cuda", dtype=dtype, requires_grad=True)
    _dirty((Lq, B, C), dtype, B, H, Lq, 0)
    o3 = masked_attention_d32(q3, k3, v3, torch.zeros(B, Lq, 0, dtype=torch.bool, device="cuda"), H)
    assert (o3 == 0).all()
    _dirty((Lq, B, C), dtype, B, H, Lq, 0)
    gq, gk, gv = torch.autograd.grad(o3, (q3, k3, v3), torch.ones_like(o3))
    assert (gq == 0).all() and gk.shape == (0, B, C) and gv.shape == (0, B, C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_queries(dtype):
    """Lq = 0: o, lse and dq are empty; no key or value receives a gradient, and dk / dv are written as zeros (pd_attention.h: "dq/dk/dv are
    written completely")"""
    from partdistillation_amd.functions.attention import attn_bwd_raw, attn_fwd_raw
    Lk, B, H = 70, 2, 2
    C = H * 32
    q = torch.empty(0, C, device="cuda", dtype=dtype)
    k, v = (torch.randn(Lk * B, C, device="cuda").to(dtype) for _ in range(2))
    o, lse = attn_fwd_raw(q, k, v, None, B, H, AC.SCALE)
    assert o.shape == (0, C) and lse.shape == (B, H, 0)
    _dirty((Lk * B, C), dtype, B, H, 0, Lk)
    dq, dk, dv = attn_bwd_raw(q, k, v, None, o, o, lse, B, H, AC.SCALE)
    assert dq.shape == (0, C) and dk.shape == k.shape and (dk == 0).all() and (dv == 0).all()
