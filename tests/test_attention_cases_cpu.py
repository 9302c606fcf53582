"""The cases of tests/attention_cases.py are what their names claim, at the shapes tests/test_attention_edges_gpu.py uses — so that a pass
of the kernels on them means the -inf bookkeeping (dead tiles, key halves, chunks, rows) and the max subtraction were really exercised."""
import math

import pytest
import torch

import attention_cases as AC

# (Lq, Lk) of the GPU tests; B = 2 is enough to show that images start at different patterns
SHAPES = [(40, 200), (40, 256), (33, 321), (97, 321), (128, 321), (40, 4097), (40, 322), (40, 513), (40, 1025), (129, 577), (5, 63)]
KCS = (64, 128, 256, 512)
FP32_MIN_NORMAL = 2.0 ** -126


def _chunks(Lk, kc):
    return (Lk + kc - 1) // kc


@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_each_builder_has_its_property(Lq, Lk):
    B = 2
    ar = torch.arange(Lk)
    m = AC.only_last_key(B, Lq, Lk)
    assert (~m).sum(-1).eq(1).all() and not m[..., Lk - 1].any()
    assert (AC.first_open_key(m) == Lk - 1).all()
    if Lk % AC.TILE:                                           # the first open key is in the last, partial tile
        assert (AC.first_open_key(m) >= (Lk // AC.TILE) * AC.TILE).all() and Lk - (Lk // AC.TILE) * AC.TILE < AC.TILE
    m = AC.only_first_key(B, Lq, Lk)
    assert (~m).sum(-1).eq(1).all() and not m[..., 0].any()
    m = AC.upper_half_of_tiles(B, Lq, Lk)
    assert torch.equal(~m[0, 0], (ar % 64) >= 32)
    for k0 in range(0, Lk, 64):                                # the first key half of every 64-key tile is dead
        assert m[..., k0:k0 + 32].all()
    m = AC.hi_lanes(B, Lq, Lk)
    assert torch.equal(~m[0, 0], (ar % 8) >= 4)
    m = AC.dead_then_live(B, Lq, Lk)
    assert m[..., :(Lk + 1) // 2].all() and not m[..., (Lk + 1) // 2:].any()
    m = AC.live_then_dead(B, Lq, Lk)
    assert not m[..., :(Lk + 1) // 2].any() and m[..., (Lk + 1) // 2:].all()
    assert AC.blocked_row(B, Lq, Lk).all()
    m = AC.image_like(B, Lq, Lk)
    h, w = AC.grid_of(Lk)
    assert h * w == Lk
    op = (~m).view(B, Lq, h, w)
    rows, cols = op.any(-1), op.any(-2)
    assert rows.any(-1).all()                                  # never empty
    assert torch.equal(op, rows[..., :, None] & cols[..., None, :])          # a rectangle: the outer product of its row and column extents ...
    for line in (rows, cols):                                  # ... which are intervals
        edges = (line[..., 1:] != line[..., :-1]).sum(-1) + line[..., 0].long() + line[..., -1].long()
        assert (edges == 2).all()
    if Lq > 1:
        assert not torch.equal(m[0, 0], m[0, 1]) or Lk < 8     # rows differ
    for name in AC.NAMES:                                      # no builder but blocked_row blocks a whole row
        full = AC.BUILDERS[name](B, Lq, Lk).all(-1)
        assert full.all() if name == "blocked_row" else not full.any(), name


@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_alternate_chunks_and_mixed_mask(Lq, Lk, kc):
    B = 2
    m = AC.alternate_chunks(B, Lq, Lk, kc=kc)
    assert not m.all(-1).any()
    if _chunks(Lk, kc) == 1:
        assert not m.any()
    for c in range(_chunks(Lk, kc) if _chunks(Lk, kc) > 1 else 0):
        blk = m[:, :, c * kc:(c + 1) * kc]
        assert blk[:, 0::2].all() if c % 2 == 0 else not blk[:, 0::2].any()         # even rows: chunk 0 dead, 1 open, ...
        if Lq > 1:
            assert blk[:, 1::2].all() if c % 2 == 1 else not blk[:, 1::2].any()     # odd rows the other way round
    if _chunks(Lk, kc) > 1:
        assert AC.dead_chunk_rows(m, kc).all()
    mixed = AC.mixed(B, Lq, Lk, kc=kc)
    for b in range(B):
        for i in range(Lq):
            assert torch.equal(mixed[b, i], AC.BUILDERS[AC.pattern_of(b, i)](B, Lq, Lk, kc=kc)[b, i])
    # exactly the intended rows are fully blocked
    assert torch.equal(mixed.all(-1), AC.blocked_rows_of(B, Lq))
    if B * Lq >= len(AC.NAMES):
        assert {AC.pattern_of(b, i) for b in range(B) for i in range(Lq)} == set(AC.NAMES)
        assert AC.blocked_rows_of(B, Lq).any()
    if _chunks(Lk, kc) > 1 and B * Lq >= len(AC.NAMES):
        assert AC.dead_chunk_rows(mixed, kc).any()             # at least one query has a fully dead chunk (and a live one)
    if Lk % AC.TILE and B * Lq >= len(AC.NAMES):               # at least one query has its first open key in the last partial tile
        fo = AC.first_open_key(mixed)
        assert ((fo >= (Lk // AC.TILE) * AC.TILE) & (fo < Lk)).any()


@pytest.mark.parametrize("Lq,Lk", [(5, 63), (33, 321), (40, 513)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", AC.WIDE)
def test_wide_inputs_defeat_exp_without_max_subtraction(kind, dtype, Lq, Lk):
    B, H = 1, 2
    q, k, v, d_o = AC.wide_inputs(kind, Lq, Lk, B, H, dtype)
    assert q.dtype == dtype and k.dtype == dtype
    s = AC.scaled_logits(q, k, H)
    off = AC.tile_offsets(kind, Lk)
    noise = s - off[torch.arange(Lk) // AC.TILE] * (q.double()[0, 0, 0] * AC.SCALE)
    assert 4.0 < noise.std().item() < 8.0                      # "about 6"
    if kind == "scrambled":
        # offsets within +-60 (exp(60) is still an fp32 number): what this case has is a running maximum that rises again and again,
        # and rows whose spread is beyond what exp() resolves — the smallest terms vanish against the maximum
        assert off.abs().max() == 60
        ups = (off[1:] > off[:-1]).sum().item()
        assert ups >= (len(off) - 1) // 3
        if len(off) >= 5:                                      # all five offsets present (Lk = 63 has two tiles: -60, 0)
            assert (s.amax(-1) - s.amin(-1)).min().item() > 88.8
    else:
        assert s.abs().max().item() > 88.8                     # exp() of the raw logit overflows fp32 ...
        assert torch.isinf(torch.exp(s.float())).any() or (torch.exp(s.float()) == 0).any()
        assert s.amax(-1).min().item() > 60                    # ... in every row
    if kind == "ascending":                                    # the rescale of the first tile's partial sums really underflows
        nt = len(off)
        m_first = s[..., :AC.TILE].amax(-1)
        m_last = s[..., (nt - 1) * AC.TILE:].amax(-1)
        assert torch.exp(m_first - m_last).max().item() < FP32_MIN_NORMAL
        assert (s.view(-1, Lk)[:, AC.TILE:2 * AC.TILE].amax(-1) > s.view(-1, Lk)[:, :AC.TILE].amax(-1)).float().mean() > 0.9


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", AC.WIDE + ("unit",))
@pytest.mark.parametrize("masked", [False, True])
def test_reference_and_its_gradients_are_finite(kind, masked, dtype):
    Lq, Lk, B, H = 33, 321, 2, 2
    q, k, v, d_o = AC.unit_inputs(Lq, Lk, B, H, dtype) if kind == "unit" else AC.wide_inputs(kind, Lq, Lk, B, H, dtype)
    mask = AC.mixed(B, Lq, Lk, kc=64) if masked else None
    qr, kr, vr = (a.double().requires_grad_() for a in (q, k, v))
    o, lse = AC.reference(qr, kr, vr, mask, H)
    grads = torch.autograd.grad(o, (qr, kr, vr), d_o.double())
    assert o.shape == (Lq, B, H * 32) and lse.shape == (B, H, Lq)
    assert torch.isfinite(o).all() and all(torch.isfinite(g_).all() for g_ in grads)
    dead = AC.blocked_rows_of(B, Lq) if masked else torch.zeros(B, Lq, dtype=torch.bool)
    assert torch.equal(torch.isneginf(lse), dead[:, None].expand(B, H, Lq)) and torch.isfinite(lse[~torch.isneginf(lse)]).all()
    if masked:                                                 # a blocked row: o = 0 exactly, dq = 0 exactly
        rows = dead.t()                                        # [Lq, B]
        assert rows.any() and o[rows].abs().max() == 0 and grads[0][rows].abs().max() == 0


@pytest.mark.parametrize("kind", AC.WIDE + ("unit",))
def test_reference_equals_softmax_attention_where_no_row_is_blocked(kind):
    Lq, Lk, B, H = 33, 321, 2, 2
    q, k, v, d_o = AC.unit_inputs(Lq, Lk, B, H, torch.float32) if kind == "unit" else AC.wide_inputs(kind, Lq, Lk, B, H, torch.float32)
    mask = AC.mixed(B, Lq, Lk, kc=64)
    mask[AC.blocked_rows_of(B, Lq)] = AC.hi_lanes(1, 1, Lk)[0, 0]          # un-block the blocked rows
    assert not mask.all(-1).any()

    def plain(q_, k_, v_):
        qh = q_.reshape(Lq, B, H, 32).permute(1, 2, 0, 3)
        kh = k_.reshape(Lk, B, H, 32).permute(1, 2, 0, 3)
        vh = v_.reshape(Lk, B, H, 32).permute(1, 2, 0, 3)
        s = (qh @ kh.transpose(-1, -2) * AC.SCALE).masked_fill(mask[:, None], float("-inf"))
        return (torch.softmax(s, -1) @ vh).permute(2, 0, 1, 3).reshape(Lq, B, H * 32), torch.logsumexp(s, -1)

    a = [t.double().requires_grad_() for t in (q, k, v)]
    b = [t.double().requires_grad_() for t in (q, k, v)]
    o1, l1 = AC.reference(*a, mask, H)
    o2, l2 = plain(*b)
    g1 = torch.autograd.grad(o1, a, d_o.double())
    g2 = torch.autograd.grad(o2, b, d_o.double())
    torch.testing.assert_close(o1, o2, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(l1, l2, rtol=1e-12, atol=1e-12)
    for x, y in zip(g1, g2):
        torch.testing.assert_close(x, y, rtol=1e-10, atol=1e-10 * max(1.0, y.abs().max().item()))


def test_reference_without_keys():
    q = torch.randn(5, 2, 64, dtype=torch.float64, requires_grad=True)
    k = torch.zeros(0, 2, 64, dtype=torch.float64, requires_grad=True)
    o, lse = AC.reference(q, k, k, None, 2)
    assert o.abs().max() == 0 and torch.isneginf(lse).all() and lse.shape == (2, 2, 5)
    (dq,) = torch.autograd.grad(o, q, torch.ones_like(o))
    assert dq.abs().max() == 0 and math.isfinite(dq.sum().item())


@pytest.mark.parametrize("matrix_core", [False, True])
def test_working_precision_is_the_same_function(matrix_core):
    """AC.working_precision (what the GPU tests derive the bf16 wide-range bound from) computes the reference's function: on unit fp32
    inputs under the mixed mask it agrees to fp32 accuracy (to bf16 accuracy of P / dS with `matrix_core`), blocked rows exactly zero"""
    Lq, Lk, B, H = 33, 321, 2, 2
    q, k, v, d_o = AC.unit_inputs(Lq, Lk, B, H, torch.float32)
    mask = AC.mixed(B, Lq, Lk, kc=64)
    a = [t.double().requires_grad_() for t in (q, k, v)]
    o, lse = AC.reference(*a, mask, H)
    ref = dict(zip(("dq", "dk", "dv"), torch.autograd.grad(o, a, d_o.double())), o=o.detach(), lse=lse.detach())
    w = AC.working_precision(q, k, v, d_o, mask, H, matrix_core=matrix_core)
    frac = 2.0 ** -8 if matrix_core else 1e-5
    for n in ("o", "dq", "dk", "dv"):
        assert (w[n].double() - ref[n]).abs().max() <= frac * ref[n].abs().max(), n
    dead = AC.blocked_rows_of(B, Lq)
    assert torch.equal(torch.isneginf(w["lse"]), dead[:, None].expand(B, H, Lq))
    live = ~torch.isneginf(ref["lse"])
    assert (w["lse"].double() - ref["lse"])[live].abs().max() < 1e-5
    assert w["o"][dead.t()].abs().max() == 0 and w["dq"][dead.t()].abs().max() == 0
