"""What the LDS-window MSDA backward kernels (msda_bwd_owner4_d32 with a 5- and a 9-cell halo, msda_bwd_tiled_d32; pd_msda_backward
and pd_msda_fused_backward) promise in their source, against the C oracle (oracle/msda_ref.c):
  A  every dispatch branch at small shapes — block decode, batch, levels without a window, the G cap, degenerate levels;
  B  the limits of the int32 fixed-point accumulation, with inputs whose reference sum is exact;
  C  the launch gate: what a launch publishes, the hysteresis, the ring of 64 slots;
  D  non-finite locations and grad_out on the window path.
Inputs and the window rule: tests/msda_window_oracle.py (checked on the CPU by tests/test_msda_window_oracle_cpu.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import msda_window_oracle as W
from oracle import msda as omsda

pytestmark = pytest.mark.gpu

def _lib():
    from partdistillation_amd import lib
    return lib.load()


def _knob(key):
    v = ctypes.c_int(-1)
    assert _lib().pd_debug_get(key, ctypes.byref(v)) == 0
    return v.value


class _variant:
    """forces a backward variant; the variant and the gate's threshold (per mille) in force before come back at the end"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.before = (_knob(b"msda_bwd_variant"), _knob(b"msda_gate_pct"))
        _lib().pd_debug_set(b"msda_bwd_variant", self.v)
        return self.before[1]

    def __exit__(self, *exc):
        _lib().pd_debug_set(b"msda_bwd_variant", self.before[0])
        _lib().pd_debug_set(b"msda_gate_pct", self.before[1])


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _operator_backward(case, loc, attn, gout=None):
    import partdistillation_amd.MultiScaleDeformableAttention as MSDA
    v, sh, lv, lo, at, go = _cuda(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"] if gout is None else gout)
    return MSDA.ms_deform_attn_backward(v, sh, lv, lo, at, go, 128)


def _fused_inputs(case):
    """device inputs of pd_msda_fused_backward, after the fused forward that leaves the softmax statistics"""
    from partdistillation_amd.functions import encoder_core as EC
    N, S, M, D, L, P = case["dims"]
    v, sh, lv, oa, ref, go = _cuda(case["value"], case["shapes"], case["lvl"], case["oa"], case["ref"], case["gout"])
    out, stats = EC.msda_fused_forward(v, sh, lv, oa, ref, torch.zeros(N * S, device="cuda"))
    return v, sh, lv, oa, ref, stats, out, go


def _fused_backward(case, inputs=None):
    """-> grad_value, d_oa, its rows' maxima"""
    from partdistillation_amd.functions import encoder_core as EC
    return EC.msda_fused_backward(*(inputs if inputs is not None else _fused_inputs(case)))


def _fused_supported(case):
    from partdistillation_amd.functions import encoder_core as EC
    N, S, M, D, L, P = case["dims"]
    return EC.msda_fused_supported(N, S, M, D, L, S, P)


def _want_doa(case, loc, attn, ol, og):
    """the chain rule of the fused form in float64 (tests/test_msda_gpu.py): d offset = grad_loc / (W, H); d logit = a (g - sum a g)"""
    N, S, M, D, L, P = case["dims"]
    sh = case["shapes"]
    norm = torch.stack([sh[:, 1], sh[:, 0]], -1).double()
    d_off = ol.double().view(N * S, M, L, P, 2) / norm[None, None, :, None, :]
    a64, g64 = attn.double().view(N * S, M, L * P), og.double().view(N * S, M, L * P)
    d_lg = a64 * (g64 - (a64 * g64).sum(-1, keepdim=True))
    return torch.cat([d_off.reshape(N * S, -1), d_lg.reshape(N * S, -1)], 1).float()


def _assert_fused(case, loc, attn, want3, got, what):
    gv, d_oa, d_am = got
    ov, ol, og = want3
    assert W.grad_misses("grad_value", gv, ov) == 0.0, (what, (gv.cpu() - ov).abs().max().item(), ov.abs().max().item())
    want = _want_doa(case, loc, attn, ol, og)
    err = (d_oa.cpu() - want).abs()
    bound = 2e-5 * want.abs().max() + 1e-4 * want.abs()                  # as test_fused_forward_backward_vs_oracle
    assert (~(err <= bound)).float().mean().item() <= 1e-5, (what, err.max().item(), want.abs().max().item())
    torch.testing.assert_close(d_am.cpu(), d_oa.abs().amax(1).cpu(), rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------------------- A: branches
@functools.lru_cache(maxsize=None)
def _random(key):
    """case, loc, attn and the oracle's three gradients — computed once per input, shared by the variants, never modified"""
    shapes, N, M, spread, seed = key
    case = W.random_case([tuple(s) for s in shapes], N, M, spread, seed)
    loc, attn = W.loc_attn(case)
    return case, loc, attn, omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])


def _branch_keys():
    return [(tuple(shapes), N, M, spread, W.case_seed(i, r)) for i, (shapes, N, M) in enumerate(W.BRANCH_CASES) for spread, r in W.REGIMES]


def _key_id(key):
    return "-".join(f"{h}x{w}" for h, w in key[0]) + f"-N{key[1]}-M{key[2]}-spread{key[3]:g}"


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("key", _branch_keys(), ids=_key_id)
def test_operator_backward_every_branch_vs_c_oracle(key, variant):
    """pd_msda_backward, fp32, D = 32, P = 4, Lq == S, every window kernel forced and the gated choice, offsets of ~1 cell (window
    hits) and ~12 cells (global atomics), locations outside [0, 1].  Tolerances of the config-2 test: grad_value 2e-5 of its
    maximum, grad_loc / grad_attn rtol 1e-4 + 1e-5 of the maximum."""
    case, loc, attn, want = _random(key)
    with _variant(variant):
        got = _operator_backward(case, loc, attn)
        torch.cuda.synchronize()
    W.assert_grads(got, want, (_key_id(key), variant))


@pytest.mark.parametrize("spread,r", W.REGIMES)
@pytest.mark.parametrize("L", sorted(W.TILED_LEVELS))
def test_tiled_backward_other_level_counts_vs_c_oracle(L, spread, r):
    """msda_bwd_tiled_d32 is the only window kernel for num_levels != 3 (the host admits up to 8): 1, 2, 4 and 8 levels"""
    j = sorted(W.TILED_LEVELS).index(L)
    key = (tuple(W.TILED_LEVELS[L]), 2, 3, spread, W.case_seed(20 + j, r))
    case, loc, attn, want = _random(key)
    for variant in (0, 1):                         # (no other window kernel serves them: both must take the tiled one)
        with _variant(variant):
            got = _operator_backward(case, loc, attn)
            torch.cuda.synchronize()
        W.assert_grads(got, want, (L, spread, variant))


@pytest.mark.parametrize("variant", [0, 2, 3])
@pytest.mark.parametrize("key", _branch_keys(), ids=_key_id)
def test_fused_backward_every_branch_vs_c_oracle(key, variant):
    case, loc, attn, want = _random(key)
    if not _fused_supported(case):
        pytest.skip("pd_msda_fused_supported declines this geometry")
    with _variant(variant):
        got = _fused_backward(case)
        torch.cuda.synchronize()
    _assert_fused(case, loc, attn, want, got, (_key_id(key), variant))


# ------------------------------------------------------------------------------------------------- B: fixed-point limits
@functools.lru_cache(maxsize=None)
def _fixed(name):
    case, loc, attn = W.fixed_point_case(name)
    return case, loc, attn, omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("name", W.FIXED_POINT_CASES)
def test_operator_backward_outside_and_inside_the_fixed_point_precondition(name, variant):
    """attention weights the operator's ABI allows and the int32 windows cannot hold (a weight of 3; 1344 unit weights on one cell;
    768 one-hot queries on one cell) and two that they can (onehot336; mixed, whose negative weights go through the windows and
    the one-FMA rounding): the reference sums are exact in fp32, a wrapped or mis-rounded sum is off by ~2^10 of max |grad_out|,
    so grad_value within 2e-5 of its maximum tells them apart.  Without the kernels' test of the precondition (max |a| <= 1,
    sum |a| <= 511 per tile, else global atomics) a3 fails in the owner kernels, unit12 and eq768_wide in all; eq768 itself
    passes either way: max |grad_out| = 1 exactly leaves the scale a factor 2 of headroom."""
    case, loc, attn, want = _fixed(name)
    with _variant(variant):
        got = _operator_backward(case, loc, attn)
        torch.cuda.synchronize()
    err = (got[0].cpu() - want[0]).abs().max().item()
    print(f"fixed-point {name} variant {variant}: max err {err:.3e} of max {want[0].abs().max().item():.3e}")
    W.assert_grads(got, want, (name, variant))


@pytest.mark.parametrize("variant", [0, 2, 3])
@pytest.mark.parametrize("name", W.FIXED_POINT_FUSED)
def test_fused_backward_outside_and_inside_the_fixed_point_precondition(name, variant):
    """the fused form's weights are a softmax, so only the one-hot cases exist for it (logits 0 / -1e4: probabilities exactly 1 / 0)"""
    case, loc, attn, want = _fixed(name)
    assert _fused_supported(case)
    with _variant(variant):
        got = _fused_backward(case)
        torch.cuda.synchronize()
    err = (got[0].cpu() - want[0]).abs().max().item()
    print(f"fixed-point fused {name} variant {variant}: max err {err:.3e} of max {want[0].abs().max().item():.3e}")
    assert W.grad_misses("grad_value", got[0], want[0]) == 0.0, (name, variant, err)


# ------------------------------------------------------------------------------------------------------------------ C: gate
def _gate():
    g = (ctypes.c_uint * 3)()
    assert _lib().pd_msda_backward_last_gate(g) == 0
    return int(g[0]), int(g[1]), int(g[2])


@functools.lru_cache(maxsize=None)
def _aimed(shapes, N, M, aim):
    case = W.aimed_case([tuple(s) for s in shapes], N, M, aim, 5 + len(aim))
    loc, attn = W.loc_attn(case)
    assert W.windows_fit(shapes) and W.windows_fit(shapes, W.HALO9, W.WIN9, W.CELLS9)
    want = omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])
    dev = dict(op=_cuda(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"]), want=[w.cuda() for w in want],
               fused=_fused_inputs(case))                    # (on the device once: an upload between launches would synchronise them)
    return case, loc, attn, want, W.count_misses(shapes, loc.numpy()), dev


class _Gated:
    """launches of one geometry through the gated (default-variant) operator or fused entry point; every launch's gradients are
    compared with the oracle's (on the device)"""

    def __init__(self, shapes, N, M, fused=False):
        self.key, self.fused = (tuple(shapes), N, M), fused
        self.total = N * W.level_starts(shapes)[1] * M * 12

    def launch(self, aim, sync=True, check=True):
        import partdistillation_amd.MultiScaleDeformableAttention as MSDA
        case, loc, attn, want, counts, dev = _aimed(*self.key, aim)
        if self.fused:
            got = _fused_backward(case, dev["fused"])
        else:
            got = MSDA.ms_deform_attn_backward(*dev["op"], 128)
        if sync:
            torch.cuda.synchronize()
        variant = _gate()[2]
        if check:
            self.check(aim, got)
        return got, variant

    def check(self, aim, got):
        case, loc, attn, want, counts, dev = _aimed(*self.key, aim)
        if self.fused:
            _assert_fused(case, loc, attn, want, got, aim)
        else:
            W.assert_grads(got, dev["want"], aim)

    def counts(self, aim):
        return _aimed(*self.key, aim)[4]

    def settle_low(self):
        """whatever the gate's state: seven synchronised launches without a miss -> the seventh sees six results of 0 misses, all of
        them the most recent that arrived, and must take the halo-5 kernel"""
        for _ in range(7):
            _, variant = self.launch("home")
        assert variant == 3 and _gate() == (0, self.total, 3)


GATE_PYRAMID = ((64, 64), (32, 32), (16, 16))


@pytest.mark.parametrize("fused", [False, True], ids=["operator", "fused"])
def test_gate_publishes_exact_counts_and_flips_with_hysteresis(fused):
    """one launch publishes {missed, looked-at} of exactly that launch; a result above the threshold sends the NEXT launches to the
    halo-9 kernel for as long as it is among the six most recent results; six low results in a row bring the halo-5 kernel back"""
    g = _Gated(GATE_PYRAMID, 1, 2, fused)
    with _variant(0) as GATE_PCT:                             # (the threshold in force, per mille)
        g.settle_low()
        missed, total = g.counts("far")
        assert total == g.total and missed * 1000 > total * GATE_PCT and g.counts("home") == (0, total)
        _, variant = g.launch("far")
        assert variant == 3                                   # picked before its own result existed
        assert _gate()[:2] == (missed, total)
        for i in range(6):                                    # the high result is among the six most recent of each of these
            _, variant = g.launch("home")
            assert variant == 2, i
            assert _gate()[:2] == (0, total)                  # the halo-9 kernel counts against the halo-5 windows too
        _, variant = g.launch("home")
        assert variant == 3
        # the halo-9 kernel measures a high launch as the halo-5 kernel does
        _, v1 = g.launch("far")
        _, v2 = g.launch("far")
        assert (v1, v2) == (3, 2) and _gate()[:2] == (missed, total)
        # a threshold of which even 0.7 is above any share (per mille): the same results now read as low
        _lib().pd_debug_set(b"msda_gate_pct", 2000)
        for _ in range(7):
            _, variant = g.launch("far")
        assert variant == 3 and _gate()[:2] == (missed, total)


@pytest.mark.parametrize("fused", [False, True], ids=["operator", "fused"])
@pytest.mark.parametrize("shapes", [((16, 16), (8, 8), (4, 4)), ((32, 32), (16, 16), (8, 8))], ids=["16-8-4", "32-16-8"])
def test_gate_ring_of_64_slots_is_recycled(shapes, fused):
    """130 launches issued back to back: every slot of the ring is used at least twice before anything is read.  The counts that
    arrive are those of ONE launch, and a slot used again publishes again: its counts and its ticket returned to zero.  (On
    16 / 8 / 4 the whole maps are inside the windows and nothing can miss; on 32 / 16 / 8 the far corner does.)"""
    g = _Gated(shapes, 2, 3, fused)
    with _variant(0) as GATE_PCT:                             # (the threshold in force, per mille)
        g.settle_low()
        missed, total = g.counts("far")
        assert (missed > 0) == (shapes[0][0] > 16)
        for i in range(130):
            got, _ = g.launch("far", sync=False, check=False)
        torch.cuda.synchronize()
        assert _gate()[:2] == (missed, total)
        g.check("far", got)
        for aim in ("home", "far", "home"):                   # slots on their third use
            g.launch(aim)
            assert _gate()[:2] == g.counts(aim), aim
        if missed * 1000 > total * GATE_PCT:
            assert _gate()[2] == 2
        g.settle_low()


def test_gate_is_not_moved_by_tiles_outside_the_fixed_point_precondition():
    """three 16 x 16 levels, one tile of 768 queries, every sample inside the windows (they cover the maps).  The fused form
    bypasses the windows of such a tile (512 queries or more): it sees every corner as uncached, which says nothing about the halo,
    so the tile is left out of the counts and the launch publishes nothing — the earlier results stand.  The operator form finds
    the weights outside the precondition after its main pass and redoes the tile; its counts are the geometric ones.  Either way
    the gate stays on the halo-5 kernel."""
    import partdistillation_amd.MultiScaleDeformableAttention as MSDA
    g = _Gated(((16, 16), (8, 8), (4, 4)), 1, 2)
    case, loc, attn, want = _fixed("eq768")
    N, S, M, D, L, P = case["dims"]
    fused_in = _fused_inputs(case)
    op_in = _cuda(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])
    with _variant(0):
        g.settle_low()
        low = _gate()
        for _ in range(8):
            gv = _fused_backward(case, fused_in)[0]
            torch.cuda.synchronize()
            assert _gate() == low
            assert W.grad_misses("grad_value", gv, want[0]) == 0.0
        for _ in range(8):
            got = MSDA.ms_deform_attn_backward(*op_in, 128)
            torch.cuda.synchronize()
            assert _gate() == (0, N * S * M * L * P, 3)
            W.assert_grads(got, want, "eq768 operator")
        g.settle_low()


# --------------------------------------------------------------------------------------------------------- D: non-finite
def _nonfinite_base(r=0):
    spread = W.REGIMES[r][0]
    return _random((tuple(W.NONFINITE_SHAPES), 1, 3, spread, W.case_seed(40, r)))


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_nonfinite_and_far_locations_on_the_window_path(variant):
    """queries whose locations are NaN, +-inf, 7.0 or -3.0: exact zeros in their grad_loc / grad_attn, every gradient finite, and
    grad_value that of the oracle with those samples removed (zero weight at a harmless location)"""
    case, loc, attn, _ = _nonfinite_base()
    S = case["dims"][1]
    bad = {3: float("nan"), 100: float("inf"), 577: float("-inf"), 580: 7.0, S - 1: -3.0, S - 40: float("nan")}      # all three levels
    loc, loc_ref, attn_ref = loc.clone(), loc.clone(), attn.clone()
    for q, v in bad.items():
        loc[0, q] = v
        loc_ref[0, q] = 0.5
        attn_ref[0, q] = 0.0
    loc[0, 7, 1, 2, 3, 0] = float("nan")                   # one coordinate of one sample
    loc_ref[0, 7, 1, 2, 3], attn_ref[0, 7, 1, 2, 3] = 0.5, 0.0
    want = omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc_ref, attn_ref, case["gout"])
    with _variant(variant):
        gv, gl, ga = _operator_backward(case, loc, attn)
        torch.cuda.synchronize()
    gv, gl, ga = gv.cpu(), gl.cpu(), ga.cpu()
    assert torch.isfinite(gv).all() and torch.isfinite(gl).all() and torch.isfinite(ga).all()
    qs = sorted(bad)
    assert gl[0, qs].abs().sum() == 0 and ga[0, qs].abs().sum() == 0
    assert gl[0, 7, 1, 2, 3].abs().sum() == 0 and ga[0, 7, 1, 2, 3] == 0
    assert W.grad_misses("grad_value", gv, want[0]) == 0.0
    keep = torch.ones(S, dtype=torch.bool)
    keep[qs] = False
    keep[7] = False
    W.assert_grads((gv, gl[0, keep], ga[0, keep]), (want[0], want[1][0, keep], want[2][0, keep]), variant)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_nonfinite_grad_out_stays_in_its_tile(what, variant):
    """one grad_out row non-finite: its tile's workgroups leave the fixed-point windows (a scale cannot be formed) and add with
    plain atomics.  Every grad_value cell that no query of that tile touches equals the oracle's; the cells the query itself
    reaches are non-finite."""
    case, loc, attn, _ = _nonfinite_base()
    shapes, S = W.NONFINITE_SHAPES, case["dims"][1]
    qbad = 24 * 9 + 13                                         # level 0, row 9, column 13: tile (0, 1) of the 2 x 2 tiles
    gout = case["gout"].clone()
    gout[0, qbad] = float(what)
    want = omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, gout)[0]
    tile, _ = W.query_tiles(shapes)
    in_tile = W.touched_cells(shapes, loc.numpy(), tile == tile[qbad])[0]
    assert not in_tile.all()
    with _variant(variant):
        gv = _operator_backward(case, loc, attn, gout)[0]
        torch.cuda.synchronize()
    gv = gv.cpu()
    for m in range(case["dims"][2]):                           # (every weight is a softmax's and no sample sits on a cell border: all four corners count)
        own = W.touched_cells(shapes, loc.numpy(), np.arange(S) == qbad, head=m)[0]
        assert own.any() and (in_tile | ~own).all()
        assert not torch.isfinite(gv[0, torch.from_numpy(own), m]).any(), m
    outside = torch.from_numpy(~in_tile)
    assert torch.isfinite(want[0, outside]).all()
    scale = want[torch.isfinite(want)].abs().max()
    assert ((gv[0, outside] - want[0, outside]).abs() <= 2e-5 * scale).all()
