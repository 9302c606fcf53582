"""pd_poly_crossings_i32 (include/pd_poly.h) on the device against the literal restatement of pycocotools' rasteriser
(tests/poly_oracle.py): the tables are int32 and every comparison is exact equality.  Then the tables through pd_rle_sample_groups_u8
into planes."""
import functools

import numpy as np
import pytest
import torch

import poly_oracle as P
from partdistillation_amd.functions.polygon import LDS_ENTRIES     # PD_POLY_LDS_ENTRIES: longer tables are sorted in global memory

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_tables(polys, h, w, garbage=-7):
    """one launch for all polygons -> list of int32 tables; the output is pre-filled with garbage, every entry must be overwritten"""
    from partdistillation_amd.functions.polygon import poly_crossings, polygon_tables
    xy, vo, to = polygon_tables(polys, h, w)
    d_xy, d_vo, d_to = (torch.from_numpy(a).to(DEV) for a in (xy, vo, to))
    starts = torch.full((int(to[-1]) + 3,), garbage, dtype=torch.int32, device=DEV)
    poly_crossings(d_xy, d_vo, len(polys), h, w, d_to, starts)
    out = starts.cpu().numpy()
    assert (out[int(to[-1]):] == garbage).all()                            # nothing past the last table
    return [out[a:b] for a, b in zip(to[:-1], to[1:])]


def _check(polys, h, w):
    got = _device_tables(polys, h, w)
    want = [P.table(p, h, w) for p in polys]
    for i, (g, t) in enumerate(zip(got, want)):
        assert g.dtype == t.dtype == np.int32 and np.array_equal(g, t), (i, h, w, np.asarray(polys[i]).tolist())
    return want


def test_integer_rectangle():
    tab, = _check([[2, 3, 2, 9, 11, 9, 11, 3]], 12, 15)
    want = np.zeros((12, 15), dtype=bool)
    want[3:9, 2:11] = True
    assert np.array_equal(P.table_mask(tab, 12, 15), want)


def test_random_polygons_float_integer_and_half_integer():
    """200 seeded polygons, 20 per launch on ten canvases with sides 1..39 (1 included): floats, integers (every vertex on a pixel
    corner, every edge through exact ties) and half-integers (vertices on pixel centres), coordinates in [-8, 48]"""
    rng = np.random.RandomState(200)
    total = 0
    for h, w in ((1, 1), (1, 39), (39, 1), (2, 2), (7, 13), (24, 24), (39, 39), (16, 31), (33, 5), (20, 38)):
        polys = []
        for i in range(20):
            k = rng.randint(3, 9)
            kind = i % 3
            poly = rng.uniform(-8, 48, 2 * k) if kind == 0 else (rng.randint(-8, 49, 2 * k).astype(np.float64) if kind == 1
                                                                  else rng.randint(-16, 97, 2 * k) / 2.0)
            polys.append(poly)
        total += sum(len(t) - 1 for t in _check(polys, h, w))
    assert total > 4000                                                    # the cases are not all empty


def test_polygons_outside_the_canvas():
    left, right = [-9, 2, -3, 2, -3, 8, -9, 9], [14, 2, 19, 2, 19, 8]
    above, below = [1, -9, 8, -9, 8, -2], [1, 12, 8, 12, 8, 19, 2, 17]
    tabs = _check([left, right, above, below], 10, 12)
    assert tabs[0].tolist() == [0] and tabs[1].tolist() == [0]             # no column is crossed
    for tab in tabs[2:]:                                                   # the columns are crossed with the row clamped: every position twice
        assert len(tab) > 1 and not P.table_mask(tab, 10, 12).any()
    assert set(tabs[2][1:] % 10) == {0} and set(tabs[3][1:] % 10) == {0} and tabs[3][1:].min() >= 10     # row 0 / the marker below the last row


def test_polygon_covering_the_canvas_uses_the_marker_below_the_last_row():
    h, w = 20, 30
    tab, = _check([[-5, -5, 60, -5, 60, 60, -5, 60]], h, w)
    assert tab.tolist() == [0] + sorted([x * h for x in range(w)] + [(x + 1) * h for x in range(w)])
    assert tab[-1] == h * w and P.table_mask(tab, h, w).all()


def test_repeated_vertices():
    closed, point = [1, 1, 8, 1, 8, 8, 1, 1], [3, 3, 3, 3, 3, 3]
    tabs = _check([closed, point, [1, 1, 1, 1, 8, 2, 8, 2, 4, 9]], 10, 10)
    assert np.array_equal(tabs[0], P.table([1, 1, 8, 1, 8, 8], 10, 10)) and tabs[1].tolist() == [0]


def test_no_polygons_and_many_polygons():
    from partdistillation_amd.functions.polygon import rasterize_polygons
    assert _device_tables([], 9, 9) == []                                  # n = 0: PD_OK without a launch
    starts, offsets = rasterize_polygons([], 9, 9, DEV)
    assert starts.numel() == 0 and offsets.tolist() == [0]
    rng = np.random.RandomState(1)
    tris = [rng.uniform(0, 12, 2) + rng.uniform(-2, 2, 6).reshape(3, 2) for _ in range(300)]
    _check([t.reshape(-1) for t in tris], 13, 14)                          # 300 tiny triangles, one workgroup each
    # more polygons than the launch has workgroups: a workgroup takes a second polygon and reuses its buffer
    base = [t.reshape(-1) for t in tris[:41]]
    got = _device_tables(base * 101, 13, 14)
    want = [P.table(p, 13, 14) for p in base]
    assert len(got) == 4141 and all(np.array_equal(g, want[i % 41]) for i, g in enumerate(got))


def test_no_fused_multiply_add():
    """hipcc contracts start + slope * t into an fma by default; the serial original rounds twice.  The four triangles are cases where the
    fused form lands on another row: the device must equal the unfused tables"""
    for tri in P.CONTRACTION_TRIANGLES:
        poly = (np.asarray(tri, dtype=np.float64) / 5).reshape(-1)
        unfused, fused = P.table(poly, 24, 24), P.table(poly, 24, 24, fused=True)
        assert not np.array_equal(unfused, fused)
        got, = _device_tables([poly], 24, 24)
        assert np.array_equal(got, unfused), tri


def _comb(lengths):
    """a comb on a 128 x 200 canvas: a spine between x = 1 and 2 and one horizontal tooth of `length` columns per entry.  A tooth is crossed
    twice per column and the spine's two ends once each: 2 * sum(lengths) + 2 boundary positions, as unsorted as they get (the walk emits
    them tooth by tooth, the table is ordered column by column)"""
    assert len(lengths) <= 20 and max(lengths) <= 197
    pts = [(1, 1), (2, 1)]
    for i, n in enumerate(lengths):
        y = 4 + 6 * i
        pts += [(2, y), (2 + n, y), (2 + n, y + 3), (2, y + 3)]
    pts += [(2, 126), (1, 126)]
    return np.asarray(pts, dtype=np.float64).reshape(-1)


@functools.lru_cache(maxsize=None)
def _comb_cases():
    """table sizes around every threshold of the kernel: the LDS capacity (at it, just above it, far above it with a size that is no
    power of two), one workgroup of sorting threads (256 pairs = 512 entries), one wave of lanes per edge (64 crossings)"""
    cases = {LDS_ENTRIES: [197] * 10 + [77], LDS_ENTRIES + 2: [197] * 10 + [78], 7882: [197] * 20, 512: [197, 58], 514: [197, 59],
             256: [127], 258: [128], 128: [63], 130: [64], 132: [65]}
    return [(count, _comb(lengths)) for count, lengths in cases.items()]


def test_comb_tables_around_the_lds_capacity_and_the_other_thresholds():
    from partdistillation_amd.functions.polygon import polygon_tables
    polys = [p for _, p in _comb_cases()]
    assert np.diff(polygon_tables(polys, 128, 200)[2]).tolist() == [c + 1 for c, _ in _comb_cases()]
    tabs = _check(polys, 128, 200)                                         # LDS and global polygons in one launch
    assert len(tabs[1]) - 1 > LDS_ENTRIES >= len(tabs[0]) - 1
    for poly, tab in zip(polys[:2], tabs[:2]):
        inside, dist = P.even_odd(poly, 128, 200)
        assert np.array_equal(P.table_mask(tab, 128, 200)[dist > 1], inside[dist > 1]) and inside.sum() > 4000
    for poly in (polys[1], polys[2], polys[3]):                            # each on its own, and one wide edge per wave count
        _check([poly], 128, 200)
    wide = [[1, 2, 1 + c, 3, 1, 9] for c in (62, 63, 64, 65, 127, 128, 129, 130)]
    _check(wide, 12, 140)


@pytest.mark.parametrize("w", [5, 63, 64, 65, 257])
def test_tables_through_rle_sample_groups(w):
    """two overlapping polygons ORed in one plane, each alone, an empty group; identity index tables; odd pitches"""
    from partdistillation_amd.functions.input_pipeline import rle_sample_groups
    from partdistillation_amd.functions.polygon import rasterize_polygons
    h = 9
    a = np.asarray([0.2, 0.6, 0.7 * w, 1.3, 0.55 * w, 8.4, 0.1 * w, 6.0])
    b = np.asarray([0.4 * w, 2.5, w + 3.0, 0.5, 0.9 * w, 7.7])
    c = np.asarray([-2.0, 4.0, w / 2.0, -3.0, w + 2.0, 4.0, w / 2.0, 12.0])                 # leaves the canvas on all four sides
    polys = [a, b, c]
    masks = [P.mask(p, h, w) for p in polys]
    assert (masks[0] & masks[1]).any() and all(m.any() and not m.all() for m in masks)
    starts, offsets = rasterize_polygons(polys, h, w, DEV)
    assert starts.dtype == torch.int32 and offsets.dtype == torch.int32 and offsets.tolist()[-1] == starts.numel()
    sx, sy = (torch.arange(n, dtype=torch.int32, device=DEV) for n in (w, h))
    groups = [[0, 1], [], [0], [1], [2], [2, 0, 1]]
    g_off = np.concatenate(([0], np.cumsum([len(g) for g in groups])))
    planes, m_area, g_area = rle_sample_groups(starts, offsets, h, w, sx, sy, g_off, [m for g in groups for m in g])
    want = np.stack([np.any([masks[m] for m in g], axis=0) if g else np.zeros((h, w), dtype=bool) for g in groups])
    assert planes.dtype == torch.uint8 and np.array_equal(planes.cpu().numpy(), want.astype(np.uint8))
    assert m_area.tolist() == [int(m.sum()) for m in masks] and g_area.tolist() == want.reshape(len(groups), -1).sum(1).tolist()
