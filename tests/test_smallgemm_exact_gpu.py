"""Every kernel body of csrc/smallgemm.hip on the exact cases of tests/smallgemm_cases.py: integer-valued bf16 operands whose products
and partial sums are exact in fp32 in any order, so the result must equal the float64 reference rounded ONCE to bf16, bit for bit.
Every operand and result is a window of a larger allocation (leading dimension above the width, NaN around the inputs, a sentinel
pattern around the outputs that is compared afterwards); split workspaces and ticket arrays have exactly the size the header's size
functions return.  The argument checks are called with one wrong argument at a time and must launch nothing."""
import ctypes

import pytest
import torch

import smallgemm_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
PD_ERR_INVALID_ARG = -1


def _libs():
    from partdistillation_amd import lib
    return lib, lib.load()


def _in(value, **kw):
    """an input: NaN everywhere outside the window(s)"""
    return SC.Guarded.of(value, SC.NAN16, DEV, **kw)


def _out(rows, cols, dtype=BF16, **kw):
    """a result: the sentinel everywhere, the window included (a kernel that skips an element leaves it there)"""
    return SC.Guarded(rows, cols, dtype, SC.SENTINEL16 if dtype == BF16 else SC.SENTINEL32, DEV, **kw)


def _tickets(n):
    t = _out(1, n, I32)
    t.t.zero_()
    return t


def _assert_exact(got, ref64, what):
    g, w = SC.bits(got.cpu()), SC.bits(SC.expected(ref64))
    bad = g != w
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} results differ from the float64 reference rounded once; first at {i}: "
                             f"got {float(got.cpu()[i])} want {float(SC.expected(ref64)[i])} (reference {float(ref64[i])})")


def _assert_equal_f32(got, ref64, what):
    assert torch.equal(SC.bits(got.cpu()), SC.bits(ref64.float())), (what, got.cpu(), ref64)


# ------------------------------------------------------------------------------------------------ Y = X W^T
def _run_tn(c, bias, relu, tickets=None):
    """one forward product through pd_sgemm_tn_bf16 (the dispatcher picks the body by K) or, for the split cases, pd_sgemm_tn_splitk_bf16
    with an exact-size workspace; returns the result window's bits"""
    lib, L = _libs()
    x, w, b = SC.tn_operands(c)
    gx, gw, gy = _in(x, pad=8), _in(w, pad=16), _out(c.M, c.N, pad=24)
    gb = _in(b[None]) if bias else None
    assert len({gx.ld, gw.ld, gy.ld}) == 3 and gx.ld > c.K and gy.ld > c.N
    bp = gb.ptr if bias else None
    if c.form == "splitk":
        nf, nt = L.pd_sgemm_split_workspace_floats(c.M, c.N, c.K), L.pd_sgemm_split_tickets(c.M, c.N)
        ws, tk = _out(1, nf, F32), tickets if tickets is not None else _tickets(nt)
        assert tk.cols >= nt and nf == (c.K // 256) * nt * 32 * 128
        lib.check(L.pd_sgemm_tn_splitk_bf16(gx.ptr, gw.ptr, bp, gy.ptr, ws.ptr, nf, tk.ptr, c.M, c.N, c.K, gx.ld, gw.ld, gy.ld, int(relu), lib.current_stream()))
        torch.cuda.synchronize()
        assert ws.intact() and tk.intact() and not tk.t.any(), "split workspace overrun / tickets not back to zero"
    else:
        lib.check(L.pd_sgemm_tn_bf16(gx.ptr, gw.ptr, bp, gy.ptr, c.M, c.N, c.K, gx.ld, gw.ld, gy.ld, int(relu), lib.current_stream()))
        torch.cuda.synchronize()
    _assert_exact(gy.t, SC.ref_tn(x, w, b if bias else None, relu), f"{SC.case_id(c)} bias={bias} relu={relu}")
    assert gy.intact(), "a store outside [M, N]"
    return SC.bits(gy.t.cpu())


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("c", SC.TN, ids=SC.case_id)
def test_forward_is_exact(c, bias, relu):
    _run_tn(c, bias, relu)


# ------------------------------------------------------------------------------------------------ dX (+)= dY W
def _run_nn(c, acc, mask, tickets=None):
    lib, L = _libs()
    dy, w, base, h = SC.nn_operands(c)
    gdy, gw, gdx = _in(dy, pad=8), _in(w, pad=16), _out(c.M, c.K, pad=24)
    gh = _in(h, pad=24) if mask else None                       # relu_ref shares dX's leading dimension
    assert gh is None or gh.ld == gdx.ld
    if acc:
        gdx.t.copy_(base)
    hp = gh.ptr if mask else None
    if c.form == "splitn":
        nf, nt = L.pd_sgemm_split_workspace_floats(c.M, c.K, c.N), L.pd_sgemm_split_tickets(c.M, c.K)
        ws, tk = _out(1, nf, F32), tickets if tickets is not None else _tickets(nt)
        assert tk.cols >= nt
        lib.check(L.pd_sgemm_nn_splitn_bf16(gdy.ptr, gw.ptr, hp, gdx.ptr, ws.ptr, nf, tk.ptr, c.M, c.N, c.K, gdy.ld, gw.ld, gdx.ld, int(acc), lib.current_stream()))
        torch.cuda.synchronize()
        assert ws.intact() and tk.intact() and not tk.t.any(), "split workspace overrun / tickets not back to zero"
    else:
        lib.check(L.pd_sgemm_nn_bf16(gdy.ptr, gw.ptr, hp, gdx.ptr, c.M, c.N, c.K, gdy.ld, gw.ld, gdx.ld, int(acc), lib.current_stream()))
        torch.cuda.synchronize()
    _assert_exact(gdx.t, SC.ref_nn(dy, w, base if acc else None, h if mask else None), f"{SC.case_id(c)} accumulate={acc} mask={mask}")
    assert gdx.intact(), "a store outside [M, K]"
    return SC.bits(gdx.t.cpu())


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("acc", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("c", SC.NN, ids=SC.case_id)
def test_input_gradient_is_exact(c, acc, mask):
    _run_nn(c, acc, mask)


def test_two_split_shapes_share_one_ticket_array():
    """(33, 132, 512) then (65, 260, 768), back to back on the same tickets (the larger shape's count): every launch leaves them zero, both
    are exact, three repeats of each are bit-identical; the same for the input-gradient form"""
    _, L = _libs()
    for cases, run, cols in ((SC.TN[-2:], lambda c, tk: _run_tn(c, True, True, tk), lambda c: c.N),
                             (SC.NN[-2:], lambda c, tk: _run_nn(c, True, True, tk), lambda c: c.K)):
        tk = _tickets(max(L.pd_sgemm_split_tickets(c.M, cols(c)) for c in cases))
        first = None
        for _ in range(3):
            got = [run(c, tk) for c in cases]
            first = first or got
            assert all(torch.equal(a, b) for a, b in zip(first, got))


# ------------------------------------------------------------------------------------------------ dW = dY^T X, dB
def _wgrad_buffers(c, want_db=True, dw_pad=12):
    """dW's leading dimension is a multiple of 4 that is NOT one of 8: what the header accepts for the weight gradients"""
    dy, x = SC.wgrad_operands(c)
    gdy, gx, gdw = _in(dy, pad=8), _in(x, pad=16), _out(c.N, c.K, pad=dw_pad)
    gdb = _out(1, c.N, F32) if want_db else None
    return dy, x, gdy, gx, gdw, gdb


def _check_wgrad(c, dy, x, gdw, gdb, what):
    _assert_exact(gdw.t, SC.ref_wgrad(dy, x), what)
    assert gdw.intact(), "a store outside dW [N, K]"
    if gdb is not None:
        _assert_equal_f32(gdb.t[0], SC.ref_db(dy), what + " dB")
        assert gdb.intact(), "a store outside dB [N]"


@pytest.mark.parametrize("c", SC.WGRAD, ids=SC.case_id)
def test_weight_gradient_is_exact(c):
    """pd_sgemm_wgrad_bf16 (sgemm_wgrad); M = 0: dW and dB are exactly zero over the valid region only"""
    lib, L = _libs()
    dy, x, gdy, gx, gdw, gdb = _wgrad_buffers(c)
    assert gdw.ld % 8 == 4
    lib.check(L.pd_sgemm_wgrad_bf16(gdy.ptr, gx.ptr, gdw.ptr, gdb.ptr, c.M, c.N, c.K, gdy.ld, gx.ld, gdw.ld, lib.current_stream()))
    torch.cuda.synchronize()
    _check_wgrad(c, dy, x, gdw, gdb, SC.case_id(c))
    dy, x, gdy, gx, gdw, _ = _wgrad_buffers(c, want_db=False, dw_pad=8)
    lib.check(L.pd_sgemm_wgrad_bf16(gdy.ptr, gx.ptr, gdw.ptr, None, c.M, c.N, c.K, gdy.ld, gx.ld, gdw.ld, lib.current_stream()))
    torch.cuda.synchronize()
    _check_wgrad(c, dy, x, gdw, None, SC.case_id(c) + " without dB")


@pytest.mark.parametrize("want_db", [True, False], ids=["dB", "nodB"])
@pytest.mark.parametrize("c", SC.WGRAD_SPLIT, ids=SC.case_id)
def test_many_row_weight_gradient_is_exact(c, want_db):
    """pd_sgemm_wgrad_split_bf16 (sgemm_wgrad_split<2> for N % 64 == 0, <1> otherwise, then wgrad_reduce) with a workspace of exactly
    pd_sgemm_wgrad_split_workspace floats; run twice: equal"""
    lib, L = _libs()
    need = L.pd_sgemm_wgrad_split_workspace(c.M, c.N, c.K)
    assert need > 0 and need % (c.N * c.K + c.N) == 0
    if (c.M, c.N, c.K) == (257, 64, 136):
        assert need == 2 * (c.N * c.K + c.N)                   # two slices of the rows
    ws = _out(1, need, F32)
    runs = []
    for _ in range(2):
        dy, x, gdy, gx, gdw, gdb = _wgrad_buffers(c, want_db)
        lib.check(L.pd_sgemm_wgrad_split_bf16(gdy.ptr, gx.ptr, gdw.ptr, gdb.ptr if want_db else None, ws.ptr, c.M, c.N, c.K, gdy.ld, gx.ld, gdw.ld,
                                              lib.current_stream()))
        torch.cuda.synchronize()
        _check_wgrad(c, dy, x, gdw, gdb, SC.case_id(c))
        assert ws.intact(), "a store outside the workspace"
        runs.append((SC.bits(gdw.t.cpu()), SC.bits(gdb.t.cpu()) if want_db else None))
    assert torch.equal(runs[0][0], runs[1][0]) and (not want_db or torch.equal(runs[0][1], runs[1][1]))


def test_grouped_weight_gradients_are_exact_and_equal_the_single_launches():
    """smallgemm.WgradQueue (pd_sgemm_wgrad_grouped_bf16, sgemm_wgrad_grouped): problems of 6, 4 (M = 0 still has its blocks: they write zeros), 4, 1 and 4
    blocks in one table — the block_begin search meets a problem of one block between larger ones — with and without dB, one of them
    writing a row slice of a larger gradient buffer"""
    from partdistillation_amd.functions import smallgemm as sg
    cases = [SC.WGRAD[0], SC.WGRAD[3], SC.WGRAD[1], SC.WGRAD[2], SC.Case("wgrad", "grouped", 65, 36, 132, 320)]
    want_db = [False, True, True, True, False]
    q, bufs = sg.WgradQueue(), []
    packed = _out(3 * 36, 132, pad=8)                           # the last problem's dW is rows 36..71 of this
    g = torch.Generator().manual_seed(7)
    before = torch.randint(-100, 101, (3 * 36, 132), generator=g).to(BF16)
    packed.t.copy_(before)
    for i, (c, db) in enumerate(zip(cases, want_db)):
        dy, x, gdy, gx, gdw, gdb = _wgrad_buffers(c, db, dw_pad=8 + 4 * (i % 2))
        out = packed.t[36:72] if i == 4 else gdw.t
        assert q.add(gdy.t, gx.t, out=out, bias_out=gdb.t[0] if db else None) is out
        bufs.append((c, dy, x, gdy, gx, gdw, gdb))
    q.run()
    torch.cuda.synchronize()
    for i, (c, dy, x, gdy, gx, gdw, gdb) in enumerate(bufs):
        if i == 4:
            _assert_exact(packed.t[36:72], SC.ref_wgrad(dy, x), "row slice of a packed gradient")
            assert packed.intact() and torch.equal(packed.t[:36].cpu(), before[:36]) and torch.equal(packed.t[72:].cpu(), before[72:])
            assert gdw.untouched()                               # the buffer that was NOT handed over is untouched
            got = packed.t[36:72]
        else:
            _check_wgrad(c, dy, x, gdw, gdb, "grouped " + SC.case_id(c))
            got = gdw.t
        single_db = torch.full((c.N,), 7.0, device=DEV) if gdb is not None else None
        single = sg.wgrad(gdy.t, gx.t, bias_out=single_db)
        assert torch.equal(SC.bits(single.cpu()), SC.bits(got.cpu()))
        assert gdb is None or torch.equal(SC.bits(single_db.cpu()), SC.bits(gdb.t[0].cpu()))


def test_grouped_queue_longer_than_one_table():
    """130 problems of (5, 8, 8) with distinct operands: WgradQueue.run() cuts them into launches of MAXP = 128 and 2 that reuse the
    device table and take consecutive slots of the pinned ring; all 130 are exact"""
    from partdistillation_amd.functions import smallgemm as sg
    cases = SC.GROUPED_SMALL
    assert len(cases) == 130 > sg.WgradQueue.MAXP == 128
    ops = [SC.wgrad_operands(c) for c in cases]
    gdy = _in(torch.stack([o[0] for o in ops]), batch=130, gap=3)
    gx = _in(torch.stack([o[1] for o in ops]), batch=130, gap=3, pad=16)
    gdw, gdb = _out(8, 8, batch=130, gap=3), _out(1, 8, F32, batch=130, gap=1)
    q = sg.WgradQueue()
    for i in range(130):
        q.add(gdy.w[i], gx.w[i], out=gdw.w[i], bias_out=gdb.w[i][0])
    q.run()
    torch.cuda.synchronize()
    _assert_exact(torch.stack(gdw.w), torch.stack([SC.ref_wgrad(dy, x) for dy, x in ops]), "130 grouped problems")
    _assert_equal_f32(torch.stack([w[0] for w in gdb.w]), torch.stack([SC.ref_db(dy) for dy, _ in ops]), "130 grouped dB")
    assert gdw.intact() and gdb.intact()
    assert len({tuple(SC.bits(SC.expected(SC.ref_wgrad(dy, x))).flatten().tolist()) for dy, x in ops}) == 130      # distinct problems


def test_grouped_abi_skips_an_empty_problem_between_two_real_ones():
    lib, L = _libs()
    Desc = lib.struct("PdSgemmWgradDesc")
    real = [SC.WGRAD[1], SC.WGRAD[2]]
    a, b = (_wgrad_buffers(c, True, dw_pad=8) for c in real)
    empty_dy, empty_x, empty_dw, empty_db = _in(SC.ints((5, 8), 8, 1)), _in(SC.ints((5, 8), 8, 2)), _out(8, 8), _out(1, 8, F32)
    descs = (Desc * 3)()

    def fill(d, gdy, gx, gdw, gdb, M, N, K):
        d.dY, d.X, d.dW, d.dB = gdy.ptr, gx.ptr, gdw.ptr, gdb.ptr
        d.M, d.N, d.K, d.ldy, d.ldx, d.ldw = M, N, K, gdy.ld, gx.ld, gdw.ld
    fill(descs[0], *a[2:], real[0].M, real[0].N, real[0].K)
    fill(descs[1], empty_dy, empty_x, empty_dw, empty_db, 5, 0, 8)              # N = 0: no block, no table entry
    fill(descs[2], *b[2:], real[1].M, real[1].N, real[1].K)
    nbytes = L.pd_sgemm_wgrad_grouped_table_bytes(3)
    assert nbytes > 0 and L.pd_sgemm_wgrad_grouped_table_bytes(6) == 2 * nbytes
    host, table = torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lib.check(L.pd_sgemm_wgrad_grouped_bf16(ctypes.byref(descs), 3, host.data_ptr(), table.data_ptr(), lib.current_stream()))
    torch.cuda.synchronize()
    for c, (dy, x, gdy, gx, gdw, gdb) in zip(real, (a, b)):
        _check_wgrad(c, dy, x, gdw, gdb, "next to an empty problem: " + SC.case_id(c))
    assert empty_dw.untouched() and empty_db.untouched()


# ------------------------------------------------------------------------------------------------ batched and multi
def _single_tn(x_ptr, w_ptr, b_ptr, M, N, K, ldx, ldw):
    lib, L = _libs()
    gy = _out(M, N, pad=8)
    lib.check(L.pd_sgemm_tn_bf16(x_ptr, w_ptr, b_ptr, gy.ptr, M, N, K, ldx, ldw, gy.ld, 0, lib.current_stream()))
    torch.cuda.synchronize()
    assert gy.intact()
    return SC.bits(gy.t.cpu())


@pytest.mark.parametrize("batch", [3, 1])
def test_batched_products_with_gaps_between_the_problems(batch):
    """pd_sgemm_tn_batched_bf16 (sgemm_tn_k256 with blockIdx.z): batch strides larger than the matrices, leading dimensions larger than
    the width; the gaps are NaN between the inputs and guarded between the results"""
    lib, L = _libs()
    cases = SC.BATCHED[:batch]
    M, N, K = cases[0].M, cases[0].N, cases[0].K
    ops = [SC.tn_operands(c) for c in cases]
    gx = _in(torch.stack([o[0] for o in ops]), batch=batch, gap=8, pad=8) if batch > 1 else _in(ops[0][0], pad=8)
    gw = _in(torch.stack([o[1] for o in ops]), batch=batch, gap=24, pad=16) if batch > 1 else _in(ops[0][1], pad=16)
    gy = _out(M, N, batch=batch, gap=16, pad=24)
    assert gx.stride > M * gx.ld > M * K and gw.stride > N * gw.ld and gy.stride > M * gy.ld > M * N
    lib.check(L.pd_sgemm_tn_batched_bf16(gx.ptr, gw.ptr, gy.ptr, M, N, K, gx.ld, gw.ld, gy.ld, batch, gx.stride, gw.stride, gy.stride, lib.current_stream()))
    torch.cuda.synchronize()
    assert gy.intact(), "a store outside the results, or into the gap between two problems"
    for b, (x, w, _) in enumerate(ops):
        _assert_exact(gy.w[b], SC.ref_tn(x, w), f"problem {b} of {batch}")
        assert torch.equal(SC.bits(gy.w[b].cpu()), _single_tn(gx.w[b].data_ptr(), gw.w[b].data_ptr(), None, M, N, K, gx.ld, gw.ld))


def test_multi_problem_launch_is_exact_with_rows_0_to_200():
    """pd_sgemm_tn_multi_bf16 (sgemm_tn_k256_multi): four problems, the maximum, K = 192; rows 33, 0, 200, 7 and columns 132, 64, 516, 16: the 5 x 7
    grid of the largest covers the others, whose surplus workgroups must leave; bias on two; leading dimensions all above the width"""
    lib, L = _libs()
    Desc = lib.struct("PdSgemmTnDesc")
    descs, bufs = (Desc * 4)(), []
    for i, (c, bias) in enumerate(zip(SC.MULTI, SC.MULTI_BIAS)):
        x, w, b = SC.tn_operands(c)
        gx, gw, gy = _in(x, pad=8 + 8 * i), _in(w, pad=16 + 8 * i), _out(c.M, c.N, pad=24 + 8 * i)
        gb = _in(b[None]) if bias else None
        d = descs[i]
        d.X, d.W, d.bias, d.Y = gx.ptr, gw.ptr, (gb.ptr if bias else None), gy.ptr
        d.M, d.N, d.ldx, d.ldw, d.ldy = c.M, c.N, gx.ld, gw.ld, gy.ld
        bufs.append((c, x, w, b if bias else None, gx, gw, gb, gy))
    lib.check(L.pd_sgemm_tn_multi_bf16(ctypes.byref(descs), 4, 192, lib.current_stream()))
    torch.cuda.synchronize()
    for c, x, w, b, gx, gw, gb, gy in bufs:
        assert gy.intact(), SC.case_id(c)
        if c.M == 0:
            assert gy.untouched()
            continue
        _assert_exact(gy.t, SC.ref_tn(x, w, b), "multi " + SC.case_id(c))
        assert torch.equal(SC.bits(gy.t.cpu()), _single_tn(gx.ptr, gw.ptr, gb.ptr if gb else None, c.M, c.N, c.K, gx.ld, gw.ld))


# ------------------------------------------------------------------------------------------------ argument checks: nothing is launched
class _Buffers:
    def __init__(self, buffers):
        self.all = buffers

    def snapshot(self):
        torch.cuda.synchronize()
        return [g.snapshot() for g in self.all]

    def unchanged(self, snaps):
        torch.cuda.synchronize()
        return all(g.same_as(s) for g, s in zip(self.all, snaps))


class _Pool(_Buffers):
    """operands large enough for every shape used below (so that even an accepted call would stay inside them), all guarded"""

    def __init__(self):
        self.a, self.b, self.c = (_out(704, 1024, pad=8) for _ in range(3))       # bf16 matrices, ld = 1032
        self.bias = _out(1, 1024)
        self.ws, self.tk, self.db = _out(1, 1 << 16, F32), _tickets(64), _out(1, 1024, F32)
        super().__init__([self.a, self.b, self.c, self.bias, self.ws, self.tk, self.db])
        self.ld = self.a.ld


def _reject(fn, name, order, base, bad, pool):
    """the base call is accepted; each entry of `bad` (one argument changed) is PD_ERR_INVALID_ARG with the entry point's name in front of
    the message, and no byte of any buffer changes"""
    _, L = _libs()
    assert fn(*[base[k] for k in order]) == 0, (name, L.pd_last_error().decode())
    snaps = pool.snapshot()
    for what, change in bad.items():
        kw = dict(base, **change)
        assert fn(*[kw[k] for k in order]) == PD_ERR_INVALID_ARG, (name, what)
        assert L.pd_last_error().decode().startswith(name), (name, what, L.pd_last_error().decode())
    assert pool.unchanged(snaps), name


def test_product_entry_points_refuse_bad_arguments():
    lib, L = _libs()
    p, s = _Pool(), lib.current_stream()
    ld = p.ld
    tn_order = ["X", "W", "bias", "Y", "M", "N", "K", "ldx", "ldw", "ldy", "relu", "stream"]
    tn = dict(X=p.a.ptr, W=p.b.ptr, bias=p.bias.ptr, Y=p.c.ptr, M=16, N=64, K=64, ldx=ld, ldw=ld, ldy=ld, relu=1, stream=s)
    tn_bad = {"K % 64": dict(K=96), "N % 4": dict(N=18), "ldx % 8": dict(ldx=ld + 4), "ldw % 8": dict(ldw=ld + 4), "ldy % 8": dict(ldy=ld + 12),
              "X 2 bytes off": dict(X=p.a.ptr + 2), "W 2 bytes off": dict(W=p.b.ptr + 2), "Y 2 bytes off": dict(Y=p.c.ptr + 2),
              "bias 2 bytes off": dict(bias=p.bias.ptr + 2), "negative M": dict(M=-1), "negative N": dict(N=-4), "null X": dict(X=None), "null Y": dict(Y=None)}
    _reject(L.pd_sgemm_tn_bf16, "pd_sgemm_tn_bf16", tn_order, tn, tn_bad, p)

    nn_order = ["dY", "W", "relu_ref", "dX", "M", "N", "K", "ldy", "ldw", "ldx", "accumulate", "stream"]
    nn = dict(dY=p.a.ptr, W=p.b.ptr, relu_ref=None, dX=p.c.ptr, M=16, N=64, K=64, ldy=ld, ldw=ld, ldx=ld, accumulate=0, stream=s)
    nn_bad = {"N % 64": dict(N=96), "K % 4": dict(K=22), "ldy % 8": dict(ldy=ld + 4), "ldw % 8": dict(ldw=ld + 4), "ldx % 8": dict(ldx=ld + 12),
              "dY 2 bytes off": dict(dY=p.a.ptr + 2), "dX 2 bytes off": dict(dX=p.c.ptr + 2), "negative M": dict(M=-1), "negative K": dict(K=-4),
              "null W": dict(W=None), "null dX": dict(dX=None)}
    _reject(L.pd_sgemm_nn_bf16, "pd_sgemm_nn_bf16", nn_order, nn, nn_bad, p)

    need = L.pd_sgemm_split_workspace_floats(16, 64, 512)
    assert need == 2 * 32 * 128 and L.pd_sgemm_split_tickets(16, 64) == 1 and L.pd_sgemm_split_workspace_floats(0, 64, 512) == 0
    sk_order = ["X", "W", "bias", "Y", "workspace", "workspace_floats", "tickets", "M", "N", "K", "ldx", "ldw", "ldy", "relu", "stream"]
    sk = dict(tn, K=512, workspace=p.ws.ptr, workspace_floats=need, tickets=p.tk.ptr)
    sk_bad = dict(tn_bad, **{"K % 64": dict(K=576), "contraction 256": dict(K=256), "contraction 640": dict(K=640),
                             "workspace one float short": dict(workspace_floats=need - 1), "null tickets": dict(tickets=None), "null workspace": dict(workspace=None)})
    _reject(L.pd_sgemm_tn_splitk_bf16, "pd_sgemm_tn_splitk_bf16", sk_order, sk, sk_bad, p)
    assert not p.tk.t.any()

    sn_order = ["dY", "W", "relu_ref", "dX", "workspace", "workspace_floats", "tickets", "M", "N", "K", "ldy", "ldw", "ldx", "accumulate", "stream"]
    sn = dict(nn, N=512, workspace=p.ws.ptr, workspace_floats=need, tickets=p.tk.ptr)
    sn_bad = dict(nn_bad, **{"N % 64": dict(N=576), "contraction 256": dict(N=256), "contraction 640": dict(N=640),
                             "workspace one float short": dict(workspace_floats=need - 1), "null tickets": dict(tickets=None)})
    _reject(L.pd_sgemm_nn_splitn_bf16, "pd_sgemm_nn_splitn_bf16", sn_order, sn, sn_bad, p)
    assert not p.tk.t.any()

    bt_order = ["X", "W", "Y", "M", "N", "K", "ldx", "ldw", "ldy", "batch", "stride_x", "stride_w", "stride_y", "stream"]
    bt = dict(X=p.a.ptr, W=p.b.ptr, Y=p.c.ptr, M=16, N=64, K=64, ldx=ld, ldw=ld, ldy=ld, batch=2, stride_x=32 * ld, stride_w=128 * ld, stride_y=32 * ld, stream=s)
    bt_bad = {k: v for k, v in tn_bad.items() if "bias" not in k}
    bt_bad.update({"K = 320": dict(K=320), "batch = 65536": dict(batch=65536), "negative batch": dict(batch=-1), "stride_x % 8": dict(stride_x=32 * ld + 4),
                   "stride_w % 8": dict(stride_w=128 * ld + 4), "stride_y % 4": dict(stride_y=32 * ld + 2)})
    _reject(L.pd_sgemm_tn_batched_bf16, "pd_sgemm_tn_batched_bf16", bt_order, bt, bt_bad, p)


def test_multi_entry_point_refuses_bad_arguments():
    lib, L = _libs()
    p, s = _Pool(), lib.current_stream()
    Desc = lib.struct("PdSgemmTnDesc")
    good = dict(X=p.a.ptr, W=p.b.ptr, bias=p.bias.ptr, Y=p.c.ptr, M=16, N=64, ldx=p.ld, ldw=p.ld, ldy=p.ld)

    def call(count=2, K=64, descs="table", **change):
        table = (Desc * 5)()
        for i in range(5):
            for k, v in dict(good, **(change if i == 1 else {})).items():       # the SECOND descriptor carries the wrong field
                setattr(table[i], k, v)
        table[1].Y = p.c.ptr + 64 * p.ld * 2                                      # its own result rows
        if "Y" in change:
            table[1].Y = change["Y"]
        return L.pd_sgemm_tn_multi_bf16(ctypes.byref(table) if descs == "table" else None, count, K, s)
    order = ["count", "K", "descs", "change"]
    fn = lambda count, K, descs, change: call(count, K, descs, **change)
    base = dict(count=2, K=64, descs="table", change={})
    bad = {"count 0": dict(count=0), "count 5": dict(count=5), "negative count": dict(count=-1), "null table": dict(descs=None), "K = 320": dict(K=320),
           "K % 64": dict(K=96), "K = 0": dict(K=0)}
    for what, change in {"N % 4": dict(N=18), "ldx % 8": dict(ldx=p.ld + 4), "ldy % 8": dict(ldy=p.ld + 12), "X 2 bytes off": dict(X=p.a.ptr + 2),
                         "Y 2 bytes off": dict(Y=p.c.ptr + 2), "bias 2 bytes off": dict(bias=p.bias.ptr + 2), "negative M": dict(M=-1),
                         "null W": dict(W=None)}.items():
        bad["second descriptor: " + what] = dict(change=change)
    _reject(fn, "pd_sgemm_tn_multi_bf16", order, base, bad, p)


def test_weight_gradient_entry_points_refuse_bad_arguments():
    lib, L = _libs()
    p, s = _Pool(), lib.current_stream()
    ld = p.ld
    order = ["dY", "X", "dW", "dB", "M", "N", "K", "ldy", "ldx", "ldw", "stream"]
    base = dict(dY=p.a.ptr, X=p.b.ptr, dW=p.c.ptr, dB=p.db.ptr, M=16, N=64, K=64, ldy=ld, ldx=ld, ldw=ld + 4, stream=s)      # ldw % 4 is enough
    bad = {"N % 4": dict(N=18), "K % 4": dict(K=22), "ldy % 8": dict(ldy=ld + 4), "ldx % 8": dict(ldx=ld + 4), "ldw % 4": dict(ldw=ld + 2),
           "ldw odd": dict(ldw=ld + 1), "dY 2 bytes off": dict(dY=p.a.ptr + 2), "X 2 bytes off": dict(X=p.b.ptr + 2), "dW 2 bytes off": dict(dW=p.c.ptr + 2),
           "negative M": dict(M=-1), "negative N": dict(N=-4), "null dY": dict(dY=None), "null dW": dict(dW=None)}
    _reject(L.pd_sgemm_wgrad_bf16, "pd_sgemm_wgrad_bf16", order, base, bad, p)

    need = L.pd_sgemm_wgrad_split_workspace(16, 64, 64)
    assert need == 64 * 64 + 64 and L.pd_sgemm_wgrad_split_workspace(0, 64, 64) == 0
    sp_order = ["dY", "X", "dW", "dB", "workspace", "M", "N", "K", "ldy", "ldx", "ldw", "stream"]
    sp = dict(base, workspace=p.ws.ptr)
    sp_bad = dict(bad, **{"M = 0": dict(M=0), "null workspace": dict(workspace=None), "workspace 4 bytes off": dict(workspace=p.ws.ptr + 4)})
    sp_bad["null X"] = dict(X=None)
    _reject(L.pd_sgemm_wgrad_split_bf16, "pd_sgemm_wgrad_split_bf16", sp_order, sp, sp_bad, p)

    Desc = lib.struct("PdSgemmWgradDesc")
    nbytes = L.pd_sgemm_wgrad_grouped_table_bytes(2)
    host, table = torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def grouped(count=2, descs="table", host_ptr=host.data_ptr(), table_ptr=table.data_ptr(), **change):
        d = (Desc * 2)()
        for i in range(2):
            for k, v in dict(base, **(change if i == 1 else {})).items():
                if k != "stream":
                    setattr(d[i], k, v)
        if "dW" not in change:
            d[1].dW = p.c.ptr + 128 * ld * 2
        return L.pd_sgemm_wgrad_grouped_bf16(ctypes.byref(d) if descs == "table" else None, count, host_ptr, table_ptr, s)
    fn = lambda count, descs, host_ptr, table_ptr, change: grouped(count, descs, host_ptr, table_ptr, **change)
    g_order = ["count", "descs", "host_ptr", "table_ptr", "change"]
    g_base = dict(count=2, descs="table", host_ptr=host.data_ptr(), table_ptr=table.data_ptr(), change={})
    g_bad = {"negative count": dict(count=-1), "null descriptors": dict(descs=None), "null pinned table": dict(host_ptr=None), "null device table": dict(table_ptr=None)}
    for what, change in bad.items():
        g_bad["second descriptor: " + what] = dict(change=change)
    assert grouped(count=0) == 0 and grouped(count=0, descs=None, host_ptr=None, table_ptr=None) == 0       # count 0: nothing to do, no error
    _reject(fn, "pd_sgemm_wgrad_grouped_bf16", g_order, g_base, g_bad, p)


def test_decoder_head_refuses_bad_arguments():
    lib, L = _libs()
    s = lib.current_stream()
    R, B, C = 8, 2, 256
    g = torch.Generator(device=DEV).manual_seed(1)
    tgt, lw, lb = torch.randn(R, C, device=DEV, generator=g), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ws = [torch.zeros(C, C, device=DEV, dtype=BF16) for _ in range(3)]
    bs = [torch.zeros(C, device=DEV, dtype=BF16) for _ in range(3)]
    dec, mean, rstd, ef = _out(1, R * C, F32), _out(1, R, F32), _out(1, R, F32), _out(1, R * C, F32)
    outs = _Buffers([dec, mean, rstd, ef])
    order = ["tgt", "ln_w", "ln_b", "eps", "w1", "b1", "w2", "b2", "w3", "b3", "dec_out", "mean", "rstd", "ef", "ef_bf16", "R", "B", "C", "stream"]
    base = dict(tgt=tgt.data_ptr(), ln_w=lw.data_ptr(), ln_b=lb.data_ptr(), eps=1e-5, w1=ws[0].data_ptr(), b1=bs[0].data_ptr(), w2=ws[1].data_ptr(),
                b2=bs[1].data_ptr(), w3=ws[2].data_ptr(), b3=bs[2].data_ptr(), dec_out=dec.ptr, mean=mean.ptr, rstd=rstd.ptr, ef=ef.ptr, ef_bf16=0, R=R, B=B,
                C=C, stream=s)
    bad = {"C = 128": dict(C=128), "R % B": dict(R=7), "B = 0": dict(B=0), "negative R": dict(R=-2), "null ln_w": dict(ln_w=None), "null tgt": dict(tgt=None),
           "null mean": dict(mean=None), "ef without w1": dict(w1=None), "ef without b3": dict(b3=None)}
    _reject(L.pd_decoder_head_bf16, "pd_decoder_head_bf16", order, base, bad, outs)
    assert all(o.intact() for o in outs.all)


# ------------------------------------------------------------------------------------------------ decoder head, guarded outputs
@pytest.mark.parametrize("Q,B", [(100, 2), (37, 3), (7, 1)])
def test_decoder_head_writes_only_its_results(Q, B):
    """the three shapes of test_smallgemm_gpu.py's head test (R = 7 is a quarter of the 32-row workgroup) with dec_out, mean, rstd and ef as
    windows of guarded buffers: values as that test requires (same references, same tolerances), guards intact for the fp32 and bf16 ef"""
    import torch.nn.functional as F
    from partdistillation_amd.functions import smallgemm as sg
    lib, L = _libs()
    R, C = Q * B, 256
    g = torch.Generator(device=DEV).manual_seed(Q)
    tgt = torch.randn(R, C, device=DEV, generator=g) * 3 + 0.5
    lw, lb = torch.randn(C, device=DEV, generator=g) * 0.2 + 1, torch.randn(C, device=DEV, generator=g) * 0.1

    def r(shape, seed, scale):
        gg = torch.Generator(device=DEV).manual_seed(seed)
        return (torch.randn(shape, device=DEV, generator=gg) * scale).bfloat16()
    ws = [r((C, C), 20 + i, C ** -0.5) for i in range(3)]
    bs = [r((C,), 30 + i, 0.5) for i in range(3)]
    results = {}
    for ef_bf16 in (0, 1):
        dec, mean, rstd, ef = _out(1, R * C, F32), _out(1, R, F32), _out(1, R, F32), _out(1, R * C, BF16 if ef_bf16 else F32)
        lib.check(L.pd_decoder_head_bf16(tgt.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, ws[0].data_ptr(), bs[0].data_ptr(), ws[1].data_ptr(),
                                         bs[1].data_ptr(), ws[2].data_ptr(), bs[2].data_ptr(), dec.ptr, mean.ptr, rstd.ptr, ef.ptr, ef_bf16, R, B, C,
                                         lib.current_stream()))
        torch.cuda.synchronize()
        assert dec.intact() and mean.intact() and rstd.intact() and ef.intact(), f"ef_bf16={ef_bf16}: a store outside the results"
        d = dec.t.view(R, C)
        torch.testing.assert_close(d, F.layer_norm(tgt, (C,), lw, lb, 1e-5), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(mean.t[0], tgt.mean(1), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(rstd.t[0], (tgt.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-5, atol=1e-6)
        results[ef_bf16] = (d.clone(), ef.t.view(B, Q, C).clone())
    dec32, ef32 = results[0]
    e = sg.linear(sg.linear(sg.linear(dec32.bfloat16(), ws[0], bs[0], True), ws[1], bs[1], True), ws[2], bs[2])
    assert not torch.isnan(ef32).any()
    torch.testing.assert_close(ef32, e.view(Q, B, C).transpose(0, 1).float(), rtol=2e-2, atol=2e-2)
    assert torch.equal(results[1][0], dec32) and torch.equal(results[1][1].float(), ef32)
    dec, mean, rstd = _out(1, R * C, F32), _out(1, R, F32), _out(1, R, F32)       # the last head: no ef
    lib.check(L.pd_decoder_head_bf16(tgt.data_ptr(), lw.data_ptr(), lb.data_ptr(), 1e-5, None, None, None, None, None, None, dec.ptr, mean.ptr, rstd.ptr,
                                     None, 0, R, B, C, lib.current_stream()))
    torch.cuda.synchronize()
    assert dec.intact() and mean.intact() and rstd.intact() and torch.equal(dec.t.view(R, C), dec32)
