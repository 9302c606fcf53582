"""GPU tests of the 7 x 7 window-attention kernels (include/pd_window_attention.h, pd_window_attn_*_w7) against a plain torch restatement of
the reference's WindowAttention.forward body (modeling/backbone/swin.py:146-173) for N = 49 — the bias gathered with the reference's
relative_position_index (:110-125), the mask built the reference's way (:425-441) — run in float64 on the bf16-rounded inputs.

Tolerances: the kernel family's own (tests/test_window_attention_gpu.py: operands are bf16, scores / softmax fp32): max abs error <= 2e-2
of each tensor's max abs for out, dqkv and dtable, 5e-2 for the block-level parameter gradients.  lse is fp32 arithmetic on identical
inputs: its error against the float64 oracle was measured on the first GPU run — 2.7e-5 in base-2 units, the largest over all cases of
this file (MEASURED_LSE_ERR below) — and is bounded at 4 x that = 1.08e-4, never more than 1e-3."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
WS, N, TBL = 7, 49, 169
LOG2E = 1.4426950408889634
MEASURED_LSE_ERR = 2.7e-5          # MI355X: 2.692e-05 in test_padding_keys_carry_no_weight (|lse| = 286, one fp32 ulp there is 3.1e-5); <= 8.9e-6 elsewhere
LSE_BOUND = min(4 * MEASURED_LSE_ERR, 1e-3)

CASES = [(1, 1, 7, 7, 0), (3, 1, 14, 14, 3), (3, 2, 10, 17, 3), (6, 1, 10, 17, 0), (24, 1, 7, 7, 0), (3, 24, 70, 70, 3)]


def _relative_position_index():
    ch, cw = torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")
    coords = torch.stack([ch.reshape(-1), cw.reshape(-1)])
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += WS - 1
    rel[:, :, 1] += WS - 1
    rel[:, :, 0] *= 2 * WS - 1
    return rel.sum(-1)


def _reference_mask(H, W, shift):
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    img = torch.zeros((1, Hp, Wp, 1))
    cnt = 0
    for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
        for wsl in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = img.view(1, Hp // WS, WS, Wp // WS, WS, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, N)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)


def _ref(qkv, table, mask, heads, scale):
    """-> (out [B_, N, C], scores [B_, heads, N, N] after bias and mask)"""
    B_, _, C3 = qkv.shape
    C = C3 // 3
    q, k, v = qkv.reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = (q * scale) @ k.transpose(-2, -1)
    bias = table[_relative_position_index().view(-1).to(table.device)].view(N, N, -1).permute(2, 0, 1)
    attn = attn + bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    return (attn.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, C), attn


def _close(got, want, frac, what):
    err = (got.double() - want.double()).abs().max().item()
    scale = want.double().abs().max().item()
    print(f"{what}: max abs err {err:.3e}, scale {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    assert math.isfinite(err) and err <= frac * scale, f"{what}: max abs err {err:.3e} > {frac} * {scale:.3e}"


def _lse_close(got, want, what):
    err = (got.double() - want).abs().max().item()
    print(f"{what}: lse max abs err {err:.3e} (base 2), max |lse| {want.abs().max().item():.3e}")
    assert math.isfinite(err) and err <= LSE_BOUND, f"{what}: lse max abs err {err:.3e} > {LSE_BOUND:.3e}"


def _inputs(heads, images, H, W, shift, table_shift=0.0, qkv_gain=1.0):
    g = torch.Generator(device="cuda").manual_seed(heads * 1000 + H * 10 + images)
    nW = (-(-H // WS)) * (-(-W // WS))
    B_, C = images * nW, heads * 32
    qkv = (torch.randn(B_, N, 3 * C, device="cuda", generator=g) * qkv_gain).to(torch.bfloat16)
    table = table_shift + torch.randn(TBL, heads, device="cuda", generator=g) * 0.5
    go = torch.randn(B_, N, C, device="cuda", generator=g).to(torch.bfloat16)
    return nW, qkv, table, go


@functools.lru_cache(maxsize=None)
def _oracle(heads, images, H, W, shift, table_shift=0.0, qkv_gain=1.0):
    """float64 out, lse (base 2), dqkv, dtable of a case on the very tensors the kernel gets (computed once, shared, never modified)"""
    nW, qkv, table, go = _inputs(heads, images, H, W, shift, table_shift, qkv_gain)
    mask = _reference_mask(H, W, shift).cuda().double() if shift else None
    qr, tr = qkv.double().requires_grad_(), table.double().requires_grad_()
    ro, scores = _ref(qr, tr, mask, heads, 32 ** -0.5)
    rq, rt = torch.autograd.grad(ro, (qr, tr), go.double())
    return ro.detach(), (torch.logsumexp(scores.detach(), -1) * LOG2E), rq, rt


def _check_case(heads, images, H, W, shift, table_shift=0.0, qkv_gain=1.0, what=""):
    from partdistillation_amd.functions import window_attention as wa
    nW, qkv, table, go = _inputs(heads, images, H, W, shift, table_shift, qkv_gain)
    B_, C = qkv.shape[0], heads * 32
    scale = 32 ** -0.5
    regions = wa.shifted_window_regions(H, W, shift, "cuda", window=WS) if shift else None
    if shift:
        assert regions[0].shape == (nW, N) and int(regions[1].sum()) > 0
    ro, rl, rq, rt = _oracle(heads, images, H, W, shift, table_shift, qkv_gain)
    qkv_g, table_g = qkv.clone().requires_grad_(), table.clone().requires_grad_()
    out = wa.window_attention(qkv_g, table_g, regions, scale, nW)
    dqkv, dtable = torch.autograd.grad(out, (qkv_g, table_g), go)
    out_raw, lse = wa.fwd_raw_w7(qkv, table, regions, scale, nW)
    assert out.dtype == torch.bfloat16 and out.shape == (B_, N, C) and dqkv.dtype == torch.bfloat16 and dqkv.shape == qkv.shape
    assert dtable.dtype == torch.float32 and dtable.shape == (TBL, heads) and lse.shape == (B_, heads, N) and lse.dtype == torch.float32
    assert torch.equal(out_raw, out.detach())
    for t in (out, lse, dqkv, dtable):
        assert torch.isfinite(t).all()
    _close(out, ro, 2e-2, what + "out")
    _close(dqkv, rq, 2e-2, what + "dqkv")
    _close(dtable, rt, 2e-2, what + "dtable")                 # every element: max over the whole table, entries 0 and 168 included
    _lse_close(lse, rl, what)
    return regions, dtable, rt


@pytest.mark.parametrize("heads,images,H,W,shift", CASES)
def test_window_attention_w7_fwd_bwd(heads, images, H, W, shift):
    regions, dtable, rt = _check_case(heads, images, H, W, shift)
    if (heads, H, shift) == (3, 14, 3):
        assert regions[0].shape[0] == 4 and int(regions[1].sum()) == 3     # none, column split, row split, both
    if images == 24:
        # entries 0 and 168 get one (query, key) pair per window; checked against their own magnitude, not the table's
        for i in (0, 168):
            _close(dtable[i], rt[i], 2e-2, f"dtable[{i}]")


def test_padding_keys_carry_no_weight():
    """softmax is shift-invariant: with table - 200 the oracle's out and gradients are those of the plain table and lse moves by
    -200 * log2(e); a padded key left at score 0, or at the mask's -100, would take the whole softmax"""
    _check_case(3, 1, 14, 14, 3, table_shift=-200.0, what="table - 200: ")
    plain, moved = _oracle(3, 1, 14, 14, 3), _oracle(3, 1, 14, 14, 3, -200.0)
    # (the fp32 table loses ~1.5e-5 of its random part next to -200: the two oracles differ by that much and no more)
    for a, b, tol in zip(plain, moved, (1e-3, 1e-3, 1e-3, 1e-3)):
        if a is plain[1]:
            b = b + 200.0 * LOG2E
        assert (a - b).abs().max().item() <= tol * max(1.0, a.abs().max().item())


def test_wide_logits():
    """raw scores spanning roughly +-60 with masks on: finite and within the same bounds"""
    nW, qkv, table, go = _inputs(3, 1, 14, 14, 3, 0.0, 3.9)
    q, k = qkv[:, :, :32].double(), qkv[:, :, 96:128].double()
    s = (q @ k.transpose(1, 2)) * 32 ** -0.5
    assert s.max().item() > 40 and s.min().item() < -40
    _check_case(3, 1, 14, 14, 3, qkv_gain=3.9, what="wide: ")


def test_window_attention_w7_rejects_bad_arguments():
    from partdistillation_amd import lib
    from partdistillation_amd.functions import window_attention as wa
    qkv = torch.zeros(5, N, 96, device="cuda", dtype=torch.bfloat16)
    table = torch.zeros(TBL, 1, device="cuda")
    with pytest.raises(lib.PdHipError, match="multiple of nW"):
        wa.fwd_raw_w7(qkv, table, None, 1.0, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.window_attention(qkv.cpu(), table.cpu(), None, 1.0, 1)
    out, lse = wa.fwd_raw_w7(qkv[:0], table, None, 1.0, 1)
    assert out.shape == (0, N, 32) and lse.shape == (0, 1, N)
    dqkv, dtable = wa.bwd_raw_w7(qkv[:0], table, None, out, out.clone(), lse, 1.0, 1)
    assert dqkv.shape == (0, N, 96) and dtable.shape == (TBL, 1) and not dtable.any()


def test_window_12_untouched():
    """window_attention on a 144-token input still is the 12 x 12 kernel, bit for bit"""
    from partdistillation_amd.functions import window_attention as wa
    g = torch.Generator(device="cuda").manual_seed(12)
    qkv = torch.randn(9, 144, 3 * 64, device="cuda", generator=g).to(torch.bfloat16)
    table = torch.randn(529, 2, device="cuda", generator=g) * 0.5
    regions = wa.shifted_window_regions(30, 30, 6, "cuda")
    assert regions[0].shape == (9, 144)
    out = wa.window_attention(qkv, table, regions, 32 ** -0.5, 9)
    raw, _ = wa.fwd_raw(qkv, table, regions, 32 ** -0.5, 9)
    assert torch.equal(out, raw)
    assert wa.supported(qkv, (12, 12), 2, 0.0) and not wa.supported(qkv, (7, 7), 2, 0.0) and not wa.supported(qkv, (12, 12), 2, 0.1)
    assert not wa.supported(qkv[:, :64], (8, 8), 2, 0.0)


def test_swin_block_w7_fused_matches_library_attention_path():
    """one plain + one shifted window-7 Swin block (Swin-T's first stage) under bf16 autocast: the fused kernel == the torch SDPA path the same
    module takes when the kernel does not apply (same weights, same input), forward and parameter gradients"""
    from partdistillation_amd.functions import window_attention as wa
    from partdistillation_amd.modeling.backbone import swin
    torch.manual_seed(0)
    layer = swin.BasicLayer(dim=96, depth=2, num_heads=3, window_size=7, drop_path=0.0).cuda()
    for blk in layer.blocks:
        torch.nn.init.normal_(blk.attn.relative_position_bias_table, std=0.5)
    x = torch.randn(2, 30 * 26, 96, device="cuda")
    seen = []
    orig = wa.supported

    def spy(qkv, *a, **k):
        seen.append(orig(qkv, *a, **k))
        return seen[-1]

    res = {}
    for fused in (True, False):
        wa.supported = spy if fused else (lambda *a, **k: False)
        try:
            layer.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = layer(x, 30, 26)[0]
            (y.float() ** 2).mean().backward()
            res[fused] = (y.detach().float(), {k: p.grad.clone() for k, p in layer.named_parameters()})
        finally:
            wa.supported = orig
    assert seen == [True, True]                                # both blocks' qkv took the kernel
    _close(res[True][0], res[False][0], 2e-2, "block output")
    for k, gr in res[False][1].items():
        _close(res[True][1][k], gr, 5e-2, "grad " + k)


def test_swin_backbone_w7_matches_cpu_oracle():
    """two window-7 stages (96 / 192 wide, 3 / 6 heads; the second one's 7 x 9 grid is padded to 7 x 14) under bf16 autocast against
    oracle/swin_ref.py in fp32 on the CPU"""
    from oracle import swin_ref
    from partdistillation_amd.modeling.backbone.swin import SwinTransformer
    torch.manual_seed(1)
    net = SwinTransformer(embed_dim=96, depths=[2, 2], num_heads=[3, 6], window_size=7, drop_path_rate=0.0, out_indices=(0, 1)).eval()
    for m in net.modules():
        if hasattr(m, "relative_position_bias_table"):
            torch.nn.init.normal_(m.relative_position_bias_table, std=0.5)
    x = torch.randn(2, 3, 56, 72)
    with torch.no_grad():
        want = swin_ref.swin_forward({k: v.clone() for k, v in net.state_dict().items()}, "", x, depths=[2, 2], num_heads=[3, 6],
                                     window_size=7, out_indices=(0, 1))
        net = net.cuda()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got = net(x.cuda())
    assert sorted(got) == sorted(want) == ["res2", "res3"]
    for k in want:
        assert got[k].shape == want[k].shape
        _close(got[k].float().cpu(), want[k], 2e-2, k)
