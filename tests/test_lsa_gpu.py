"""pd_lsa_batched (csrc/lsa.hip) against scipy.optimize.linear_sum_assignment on the float64 cast of the same fp32 matrix:
the lane-stride edges of its 64-lane column scan, the full small dimension, the documented size limits, ragged launches
with poisoned padding, non-finite costs, extreme magnitudes, the order of equal-cost pairs and degenerate calls.

Every comparison is exact.  An expectation is SciPy's answer (all -1 where SciPy raises), or follows from how the input
was built (the pair order of test_equal_pair_costs_keep_solved_row_order); none is taken from the kernel."""
import math

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _draw(rng, q, n, ties=False):
    c = rng.standard_normal((q, n)).astype(np.float32)
    return np.round(c * 2) / 2 if ties else c                             # half-integers: heavy ties


def _batch(problems, q, cmax, pad=0.0):
    """problems: list of [q, n_b] fp32 -> (cost [nb, q, cmax] with `pad` in the columns >= n_b, ncols list)"""
    cost = np.full((len(problems), q, cmax), pad, np.float32)
    for b, c in enumerate(problems):
        assert c.dtype == np.float32 and c.shape[0] == q and c.shape[1] <= cmax
        cost[b, :, : c.shape[1]] = c
    return cost, [c.shape[1] for c in problems]


def _solve(cost, ncols):
    """two launches on the same input; they must agree bit for bit"""
    from partdistillation_amd.functions import lsa
    ct, nt = torch.from_numpy(cost).to(DEV), torch.tensor(ncols, dtype=torch.int32)
    rows, cols = lsa.solve_batched(ct, nt)
    rows2, cols2 = lsa.solve_batched(ct, nt)
    assert torch.equal(rows, rows2) and torch.equal(cols, cols2), "two runs on the same input differ"
    assert rows.dtype == torch.int64 and cols.dtype == torch.int64 and rows.shape == cols.shape == (cost.shape[0], cost.shape[2])
    return rows.cpu().numpy(), cols.cpu().numpy()


def _scipy(c):
    """sorted (row, col) pairs of SciPy on the float64 cast, or None where SciPy raises (NaN, -inf, infeasible)"""
    try:
        r0, c0 = linear_sum_assignment(c.astype(np.float64))
    except ValueError:
        return None
    return sorted(zip(r0.tolist(), c0.tolist()))


def _check_problem(c, rows, cols, tag):
    """c: the problem's own [q, n] fp32 matrix; rows / cols: its full output rows (length ncols_max)"""
    q, n = c.shape
    k = min(q, n)
    want = _scipy(c)
    if want is None:
        assert (rows == -1).all() and (cols == -1).all(), f"{tag}: SciPy rejects this matrix, outputs must stay -1"
        return
    assert (rows[k:] == -1).all() and (cols[k:] == -1).all(), f"{tag}: entries past k={k} must be -1"
    r, cc = rows[:k], cols[:k]
    assert ((r >= 0) & (r < q)).all() and len(set(r.tolist())) == k, f"{tag}: rows not distinct / out of range: {r}"
    assert ((cc >= 0) & (cc < n)).all() and len(set(cc.tolist())) == k, f"{tag}: cols not distinct / not < ncols={n}: {cc}"
    c64 = c.astype(np.float64)
    total, total_ref = math.fsum(c64[r, cc].tolist()), math.fsum(c64[i, j] for i, j in want)
    assert total == total_ref, f"{tag}: total cost {total!r} != SciPy's {total_ref!r}"
    assert sorted(zip(r.tolist(), cc.tolist())) == want, f"{tag}: pairs differ from SciPy's (tie-breaking)"
    assert (np.diff(c[r, cc]) >= 0).all(), f"{tag}: pair costs not in ascending order: {c[r, cc]}"


def _run(problems, q, cmax, pad=0.0):
    cost, ncols = _batch(problems, q, cmax, pad)
    rows, cols = _solve(cost, ncols)
    for b, c in enumerate(problems):
        _check_problem(c, rows[b], cols[b], f"problem {b} ({q}x{c.shape[1]})")
    return rows, cols


# ----------------------------------------------------------------------------- 1. lane-stride edges of the column scan
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("large", [63, 64, 65, 127, 128, 129, 191])
def test_lane_stride_edges(large, transposed, ties):
    """the solved problem has `large` columns: a lane's share of the todo list is empty, one short or full, and n_todo
    shrinks across a multiple of 64 while a path grows"""
    q, n = (large, 5) if transposed else (5, large)
    rng = np.random.default_rng(1000 * large + 10 * transposed + ties)
    _run([_draw(rng, q, n, ties) for _ in range(8)], q, n)


# ----------------------------------------------------------------------------- 2. the full small dimension
@pytest.mark.parametrize("shape", [(64, 64), (300, 64), (64, 300), (65, 64), (64, 63)])
def test_full_small_dimension(shape):
    q, n = shape
    rng = np.random.default_rng(q * 1000 + n)
    _run([_draw(rng, q, n, b % 4 == 1) for b in range(8)], q, n)


# ----------------------------------------------------------------------------- 3. size limits
@pytest.mark.parametrize("shape", [(4096, 64), (4096, 1), (64, 4096), (1558, 3), (1559, 3), (2000, 8)])
def test_size_limits_solve(shape):
    """the documented maximum in both orientations, and the shapes around 64 KB of LDS (the old carve crossed it at 1559)"""
    q, n = shape
    rng = np.random.default_rng(q * 100 + n)
    _run([_draw(rng, q, n, b % 4 == 1) for b in range(4)], q, n)


@pytest.mark.parametrize("shape", [(4097, 2), (65, 65)])
def test_size_limits_refuse(shape):
    from partdistillation_amd import lib
    from partdistillation_amd.functions import lsa
    q, n = shape
    cost = torch.zeros((2, q, n), dtype=torch.float32, device=DEV)
    with pytest.raises(lib.PdHipError, match="exceeds"):
        lsa.solve_batched(cost, torch.full((2,), n, dtype=torch.int32))
    torch.cuda.synchronize()                                              # nothing was launched, nothing is pending


# ----------------------------------------------------------------------------- 4. ragged launch
RAGGED = [0, 1, 7, 39, 40, 41, 64, 3]                                     # both orientations around nrows = 40, and an empty problem


def _ragged_problems():
    rng = np.random.default_rng(404)
    return [_draw(rng, 40, n, b % 4 == 1) for b, n in enumerate(RAGGED)]


def test_ragged_launch_ignores_padding():
    problems = _ragged_problems()
    rows0, cols0 = _run(problems, 40, 64, pad=0.0)
    for pad in (np.nan, -1e30):                                           # a padding column that is read poisons or wins the problem
        rows, cols = _run(problems, 40, 64, pad=pad)
        assert np.array_equal(rows, rows0) and np.array_equal(cols, cols0), f"padding {pad} changed the result"


def test_ragged_launch_through_solve_ragged():
    from partdistillation_amd.functions import lsa
    problems = _ragged_problems()
    out = lsa.solve_ragged([torch.from_numpy(c).to(DEV) for c in problems])
    assert len(out) == len(problems)
    for b, (c, (r, cc)) in enumerate(zip(problems, out)):
        k = min(40, c.shape[1])
        assert r.shape == (k,) and cc.shape == (k,)
        r, cc = r.cpu().numpy(), cc.cpu().numpy()
        assert sorted(zip(r.tolist(), cc.tolist())) == _scipy(c), f"problem {b}"
        assert (np.diff(c[r, cc]) >= 0).all(), f"problem {b}"


# ----------------------------------------------------------------------------- 5. non-finite costs
@pytest.mark.parametrize("shape", [(6, 30), (30, 6), (70, 5)])
def test_non_finite_costs(shape):
    """+inf is legal where a finite assignment exists; a NaN, a -inf or an infeasible matrix makes SciPy raise and leaves the
    problem's outputs at -1, without touching the other problems of the launch"""
    q, n = shape
    rng = np.random.default_rng(q * 50 + n)
    problems = [_draw(rng, q, n, b % 4 == 1) for b in range(8)]
    some_inf, blocked, has_nan, has_ninf = 1, 3, 4, 6
    problems[some_inf][rng.random((q, n)) < 0.2] = np.inf
    if q <= n:
        problems[blocked][q // 2, :] = np.inf                             # a row of the solved problem with no finite entry
    else:
        problems[blocked][:, n // 2] = np.inf
    problems[has_nan][q // 3, n // 2] = np.nan
    problems[has_ninf][q - 1, 0] = -np.inf
    assert np.isinf(problems[some_inf]).any() and _scipy(problems[some_inf]) is not None   # feasible for SciPy itself
    for b in (blocked, has_nan, has_ninf):
        assert _scipy(problems[b]) is None                                # SciPy raises on each of them
    rows, cols = _run(problems, q, n + 2)
    for b in (blocked, has_nan, has_ninf):
        assert (rows[b] == -1).all() and (cols[b] == -1).all()
    for b in (0, some_inf, 2, 5, 7):
        assert (rows[b, : min(q, n)] >= 0).all()


# ----------------------------------------------------------------------------- 6. extreme magnitudes
@pytest.mark.parametrize("shape", [(70, 6), (6, 70), (9, 9), (130, 64)])
def test_extreme_magnitudes_and_constant_costs(shape):
    q, n = shape
    rng = np.random.default_rng(q * 77 + n)
    problems = [
        _draw(rng, q, n) * np.float32(1e30),
        _draw(rng, q, n) * np.float32(1e-30),
        np.full((q, n), 1.5, np.float32),                                 # every assignment is optimal: SciPy's scan order decides
        _draw(rng, q, n, ties=True) * np.float32(1e30),
        np.zeros((q, n), np.float32),
        np.full((q, n), -3.25e30, np.float32),
        _draw(rng, q, n, ties=True) * np.float32(1e-30),
        _draw(rng, q, n),
    ]
    for c in problems:
        assert np.isfinite(c).all()
    _run(problems, q, n)


# ----------------------------------------------------------------------------- 7. output order with equal pair costs
@pytest.mark.parametrize("shape", [(64, 64), (20, 6), (6, 20), (300, 64)])
def test_equal_pair_costs_keep_solved_row_order(shape):
    """the optimum is planted: solved row s (a target when there are more queries than targets, else a query) is paired
    with partner[s] at a cost from {0.25, 0.5, 0.75}, everything else costs >= 100, so no other assignment can win.
    Pairs come out by ascending cost, and pairs of equal cost by ascending solved row (the stable insertion sort)."""
    q, n = shape
    tr = n < q
    R, C = (n, q) if tr else (q, n)
    problems, orders = [], []
    for b in range(8):
        rng = np.random.default_rng(q * 31 + n * 7 + b)
        partner = rng.permutation(C)[:R]
        vals = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=R)
        if b == 1:
            vals[:] = 0.5                                                 # one run of k equal costs
        solved = (100.0 + np.abs(rng.standard_normal((R, C)))).astype(np.float32)
        solved[np.arange(R), partner] = vals
        problems.append(np.ascontiguousarray(solved.T) if tr else solved)
        order = sorted(range(R), key=lambda s: (vals[s], s))
        orders.append([(int(partner[s]), s) if tr else (s, int(partner[s])) for s in order])
    rows, cols = _run(problems, q, n)                                     # pair set == SciPy's, costs ascending
    for b, want in enumerate(orders):
        assert sorted(want) == _scipy(problems[b])                        # the planted optimum is SciPy's, too
        got = list(zip(rows[b, :R].tolist(), cols[b, :R].tolist()))
        assert got == want, f"problem {b}: equal-cost pairs out of solved-row order"


# ----------------------------------------------------------------------------- 8. degenerate calls
def test_degenerate_calls():
    from partdistillation_amd.functions import lsa
    rows, cols = lsa.solve_batched(torch.zeros((0, 5, 3), device=DEV), torch.zeros((0,), dtype=torch.int32))
    assert rows.shape == cols.shape == (0, 3) and rows.dtype == cols.dtype == torch.int64
    rows, cols = lsa.solve_batched(torch.zeros((3, 5, 0), device=DEV), torch.zeros((3,), dtype=torch.int32))
    assert rows.shape == cols.shape == (3, 0) and rows.dtype == cols.dtype == torch.int64
    rows, cols = lsa.solve_batched(torch.zeros((3, 0, 4), device=DEV), torch.tensor([4, 2, 0], dtype=torch.int32))
    assert rows.shape == cols.shape == (3, 4)
    assert (rows == -1).all() and (cols == -1).all()                      # no rows: k = 0 pairs in every problem
    with pytest.raises(RuntimeError):
        lsa.solve_batched(torch.zeros((2, 5, 3)), torch.full((2,), 3, dtype=torch.int32))
