"""The window-rule restatement and the inputs of tests/test_msda_windows_gpu.py (tests/msda_window_oracle.py), checked where no GPU
is needed: the tiling, the miss count on a hand-computed example, the exactness of the fixed-point inputs, and — for every seed
the GPU tests use — that the C oracle in fp32 meets itself in fp64 at the GPU tests' tolerances with NO element left out."""
import numpy as np
import pytest
import torch

import msda_window_oracle as W
from oracle import msda as omsda

ALL_SHAPES = [c[0] for c in W.BRANCH_CASES] + list(W.TILED_LEVELS.values()) + [W.NONFINITE_SHAPES, [(64, 64), (32, 32), (16, 16)],
                                                                              [(32, 32), (16, 16), (8, 8)], [(128, 128), (64, 64), (32, 32)]]


@pytest.mark.parametrize("shapes", ALL_SHAPES, ids=lambda s: "-".join(f"{h}x{w}" for h, w in s))
def test_every_query_belongs_to_exactly_one_tile(shapes):
    tile, claims = W.query_tiles(shapes)
    assert (claims == 1).all() and (tile >= 0).all() and (tile < W.grid(shapes) ** 2).all()


def test_grid_and_window_by_hand():
    assert W.grid([(16, 16), (8, 8), (4, 4)]) == 1 and W.grid([(24, 20), (12, 10), (6, 5)]) == 2
    assert W.grid([(272, 4), (136, 2), (68, 1)]) == 16 and W.grid([(128, 128), (64, 64), (32, 32)]) == 8
    # 128 cells in 8 tiles: tile 3 owns [48, 64), its window is [43, 69); the first and last windows are cut by the map
    assert W.window(128, 3, 8) == (43, 26) and W.window(128, 0, 8) == (0, 21) and W.window(128, 7, 8) == (107, 21)
    # G capped at 16 on 272 cells: tile 0 owns 17 cells, 17 + 5 = 22 fit; tile 1 owns [17, 34): 12 .. 39 is 27 cells, clipped to 26
    assert W.window(272, 0, 16) == (0, 22) and W.window(272, 1, 16) == (12, 26)
    assert W.windows_fit([(64, 64), (32, 32), (16, 16)]) and W.windows_fit([(64, 64), (32, 32), (16, 16)], W.HALO9, W.WIN9, W.CELLS9)
    assert not W.windows_fit([(40, 40), (40, 40), (40, 40)])


@pytest.mark.parametrize("shapes", [[(64, 64), (32, 32), (16, 16)], [(32, 32), (16, 16), (8, 8)], [(16, 16), (8, 8), (4, 4)]])
def test_zero_offsets_give_zero_misses(shapes):
    case = W.aimed_case(shapes, 2, 3, "home", 1)
    loc, _ = W.loc_attn(case)
    N, S, M, D, L, P = case["dims"]
    assert W.count_misses(shapes, loc.numpy()) == (0, N * S * M * L * P)


def test_hand_computed_32x32_example():
    """one level of 32 x 32 (and two of 1 x 1, which every sample hits): G = 2; tile 0 owns rows / columns [0, 16) with the window
    [0, 21), tile 1 owns [16, 32) with [11, 32).  A footprint at low corner c covers c and c + 1: inside tile 0's window for
    c <= 19, inside tile 1's for c >= 11."""
    shapes = [(32, 32), (1, 1), (1, 1)]
    S = 1026
    loc = np.full((1, S, 1, 3, 4, 2), 0.5, dtype=np.float32)          # levels 1 and 2: the centre of their only pixel: in range, inside
    at = lambda c: (c + 0.75) / 32.0                                    # low corner c, a quarter cell past its centre

    def q(y, x):
        return y * 32 + x
    # query (0, 0) of tile (0, 0): low corners (y, x) = (19, 19) in; (20, 3) out (rows 20, 21); (3, 20) out; (25, 25) out
    loc[0, q(0, 0), 0, 0] = [[at(19), at(19)], [at(3), at(20)], [at(20), at(3)], [at(25), at(25)]]
    # query (20, 5) of tile (1, 0): rows from 11, columns to 20: (11, 19) in; (10, 19) out; (30, 0) in; (11, 20) out
    loc[0, q(20, 5), 0, 0] = [[at(19), at(11)], [at(19), at(10)], [at(0), at(30)], [at(20), at(11)]]
    # every other query of level 0: own pixel (clamped inside) -> in; the two queries of the 1 x 1 levels belong to tile (1, 1)
    # (rows [1 * 1 / 2, 2 * 1 / 2) = [0, 1)): low corner (20, 20) -> in
    for y in range(32):
        for x in range(32):
            if (y, x) not in ((0, 0), (20, 5)):
                loc[0, q(y, x), 0, 0, :] = [at(min(x, 30)), at(min(y, 30))]
    loc[0, 1024:, 0, 0, :] = [at(20), at(20)]
    assert W.query_tiles(shapes)[0][[q(0, 0), q(20, 5), 1024, 1025]].tolist() == [0, 2, 3, 3]
    assert W.count_misses(shapes, loc) == (3 + 2, S * 12)
    # a sample outside the map is looked at but is no miss; NaN likewise
    loc[0, q(0, 0), 0, 0, 0] = [7.0, -3.0]
    loc[0, q(0, 0), 0, 0, 1] = np.nan
    assert W.count_misses(shapes, loc) == (3 + 2 - 1, S * 12)
    cells = W.touched_cells(shapes, loc, np.arange(S) == q(20, 5))
    want = {(y + dy) * 32 + x + dx for (y, x) in ((11, 19), (10, 19), (30, 0), (11, 20)) for dy in (0, 1) for dx in (0, 1)} | {1024, 1025}
    assert set(np.flatnonzero(cells[0]).tolist()) == want
    # two images, two heads: the second head of image 1 sends that query to low corner (2, 1); selection by several queries
    loc2 = np.tile(loc, (2, 1, 2, 1, 1, 1))
    loc2[1, q(20, 5), 1, 0, :] = [at(1), at(2)]
    head1 = W.touched_cells(shapes, loc2, np.arange(S) == q(20, 5), head=1)
    assert set(np.flatnonzero(head1[0]).tolist()) == want and set(np.flatnonzero(head1[1]).tolist()) == {65, 66, 97, 98, 1024, 1025}
    both = W.touched_cells(shapes, loc2, np.isin(np.arange(S), [q(20, 5), q(3, 3)]))
    assert set(np.flatnonzero(both[1]).tolist()) == want | {65, 66, 97, 98} | {3 * 32 + 3, 3 * 32 + 4, 4 * 32 + 3, 4 * 32 + 4}


@pytest.mark.parametrize("name", W.FIXED_POINT_CASES)
def test_fixed_point_inputs_have_an_exact_reference(name):
    """the fp32 oracle's grad_value IS the exact sum: fp64 gives the same numbers bit for bit; and the case is what it says"""
    case, loc, attn = W.fixed_point_case(name)
    gv32 = omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])[0]
    gv64 = omsda.msda_backward(case["value"].double(), case["shapes"], case["lvl"], loc.double(), attn.double(), case["gout"].double())[0]
    assert torch.equal(gv32.double(), gv64)
    S = case["dims"][1]
    peak = {"a3": None, "unit12": 4 * S, "eq768": S, "eq768_wide": S, "onehot336": S, "mixed": None}[name]
    assert S == (768 if name.startswith("eq768") else 336)
    if peak is not None:        # the weights on the one cell (5, 9) of level 0
        assert attn.abs().sum().item() >= peak and gv64[0, 5 * 16 + 9].abs().max().item() >= 0.9 * peak * case["gout"].abs().max().item() * 0.9
    amax, asum = W.precondition(attn)
    assert amax == {"a3": 3.0, "mixed": 0.125}.get(name, 1.0)
    # which side of the kernels' precondition (every |a| <= 1 and sum |a| <= 511 per tile and head) the case is on
    inside = amax <= 1.0 and asum <= 511.0
    assert inside == (name in ("onehot336", "mixed")), (name, amax, asum)
    if name == "mixed":
        assert (attn < 0).any() and asum > 100.0


def _all_random_cases():
    for i, (shapes, N, M) in enumerate(W.BRANCH_CASES):
        for spread, r in W.REGIMES:
            yield shapes, N, M, spread, W.case_seed(i, r)
    for j, (L, shapes) in enumerate(sorted(W.TILED_LEVELS.items())):
        for spread, r in W.REGIMES:
            yield shapes, 2, 3, spread, W.case_seed(20 + j, r)
    for spread, r in W.REGIMES:
        yield W.NONFINITE_SHAPES, 1, 3, spread, W.case_seed(40, r)


@pytest.mark.parametrize("shapes,N,M,spread,seed", list(_all_random_cases()),
                         ids=lambda v: "-".join(f"{h}x{w}" for h, w in v) if isinstance(v, list) else str(v))
def test_seeds_leave_nothing_out_between_the_fp32_and_the_fp64_oracle(shapes, N, M, spread, seed):
    case = W.random_case(shapes, N, M, spread, seed)
    loc, attn = W.loc_attn(case)
    g32 = omsda.msda_backward(case["value"], case["shapes"], case["lvl"], loc, attn, case["gout"])
    g64 = omsda.msda_backward(case["value"].double(), case["shapes"], case["lvl"], loc.double(), attn.double(), case["gout"].double())
    for name, a, b in zip(("grad_value", "grad_loc", "grad_attn"), g32, g64):
        assert W.grad_misses(name, a.double(), b) == 0.0, name
    # the regimes do what they are for: locations leave [0, 1], and at 12 cells samples leave their windows (where there are any)
    assert ((loc < 0) | (loc > 1)).any()
