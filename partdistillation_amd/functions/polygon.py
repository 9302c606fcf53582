"""Polygon rasterisation on the device (include/pd_poly.h, csrc/polygon.hip): pycocotools' rleFrPoly restated (parity with pycocotools
itself is UNPINNED: it is not available to test against).  The host does what is integer bookkeeping — the (int)(5 x + .5) upsample of
the vertices, the EXACT number of boundary positions of every polygon (a closed form of the upsampled end points of its edges) and the
CSR offsets that follow — so the kernel needs no count pass and nothing is read back; the device computes and sorts the positions.  A
polygon's table is in the run-starts format of include/pd_input.h: `rle_sample_groups` (functions/input_pipeline.py) turns tables into planes,
a group of several polygons into their OR.  GPU only; there is no fallback."""
import numpy as np
import torch

from .. import lib as _lib

SCALE = 5                        # rleFrPoly's upsampling factor
COORD_LIMIT = 2 ** 30            # |5 x + .5| at or above this is refused: the walk's integers would overflow
LDS_ENTRIES = 4096               # PD_POLY_LDS_ENTRIES: longer tables are sorted in global memory (slower, same result)


def upsample(xy):
    """float64 [..., 2] -> int64: C's (int)(5 * x + .5), truncation toward zero"""
    return np.trunc(SCALE * np.asarray(xy, dtype=np.float64) + .5).astype(np.int64)


def crossing_counts(x0, x1, w):
    """boundary positions of the edges with upsampled end columns x0 -> x1: the columns X in [0, w - 1] with
    min(x0, x1) <= 5 X + 2 <= max(x0, x1) - 1 (the upsampled column moves monotonically and by at most one per step of the walk)"""
    lo, hi = np.minimum(x0, x1), np.maximum(x0, x1)
    n_lo = np.maximum(0, (lo + 2) // SCALE)                              # ceil((lo - 2) / 5)
    n_hi = np.minimum(w - 1, (hi - 3) // SCALE)
    return np.maximum(0, n_hi - n_lo + 1)


def polygon_tables(polys, h, w):
    """polys: flat [x0, y0, x1, y1, ...] (or [k, 2]) float polygons, already transformed to the h x w canvas
    -> (xy float64 [sum k, 2], vert_offsets int32 [n + 1], table_offsets int32 [n + 1]): polygon i's table has
    table_offsets[i + 1] - table_offsets[i] = 1 + its exact number of boundary positions.
    ValueError: an odd number of coordinates or fewer than 6 (detectron2's PolygonMasks), a non-finite value, |5 x + .5| >= 2^30."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"polygon_tables: canvas {h} x {w}")
    arrays, counts = [], []
    for p in polys:
        a = np.asarray(p, dtype=np.float64).reshape(-1)
        if a.size % 2 != 0 or a.size < 6:
            raise ValueError(f"Cannot create a polygon from {a.size} coordinates.")
        if not np.isfinite(a).all():
            raise ValueError("polygon_tables: non-finite polygon coordinate")
        if (np.abs(SCALE * a + .5) >= COORD_LIMIT).any():
            raise ValueError(f"polygon_tables: polygon coordinate out of range (|5 x + .5| >= 2^30)")
        arrays.append(a.reshape(-1, 2))
        counts.append(a.size // 2)
    vert_offsets = np.concatenate(([0], np.cumsum(counts, dtype=np.int64))).astype(np.int64)
    xy = np.concatenate(arrays) if arrays else np.zeros((0, 2), dtype=np.float64)
    table_len = np.ones(len(arrays), dtype=np.int64)
    if len(arrays):
        X = upsample(xy)[:, 0]
        nxt = np.arange(len(X)) + 1
        nxt[vert_offsets[1:] - 1] = vert_offsets[:-1]                     # the loop closes on the polygon's first vertex
        table_len += np.add.reduceat(crossing_counts(X, X[nxt], w), vert_offsets[:-1])
    table_offsets = np.concatenate(([0], np.cumsum(table_len)))
    if table_offsets[-1] > 0x7fffffff or vert_offsets[-1] > 0x7fffffff:
        raise ValueError("polygon_tables: the tables do not fit int32 offsets")
    return np.ascontiguousarray(xy), vert_offsets.astype(np.int32), table_offsets.astype(np.int32)


def poly_crossings(xy, vert_offsets, n, h, w, table_offsets, starts):
    """pd_poly_crossings_i32 on device tensors (xy float64, the offsets int32 [n + 1], starts int32 with room for table_offsets[n])"""
    if n and not (xy.is_cuda and vert_offsets.is_cuda and table_offsets.is_cuda and starts.is_cuda):
        raise RuntimeError("poly_crossings: GPU only (no CPU fallback in partdistillation_amd)")
    assert xy.dtype == torch.float64 and vert_offsets.dtype == torch.int32 and table_offsets.dtype == torch.int32 and starts.dtype == torch.int32
    assert vert_offsets.numel() >= n + 1 and table_offsets.numel() >= n + 1
    _lib.check(_lib.load().pd_poly_crossings_i32(xy.data_ptr() if n else None, vert_offsets.data_ptr() if n else None, n, int(h), int(w),
                                                 table_offsets.data_ptr() if n else None, starts.data_ptr() if n else None,
                                                 _lib.current_stream()))
    return starts


def rasterize_polygons(polys, h, w, device="cuda", extra=()):
    """polys (see polygon_tables) -> device (starts int32, offsets int32 [n + 1]) ready for `rle_sample_groups` with H = h, W = w:
    one upload (vertices and both offset vectors in one buffer), one launch, no synchronisation.  `extra`: int32 host arrays that ride
    in the same upload (a caller's index and group tables); with it the result is (starts, offsets, [their device views])"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rasterize_polygons: GPU only (no CPU fallback in partdistillation_amd)")
    xy, vert_offsets, table_offsets = polygon_tables(polys, h, w)
    ints = [vert_offsets, table_offsets] + [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in extra]
    blob = np.concatenate([xy.reshape(-1).view(np.uint8)] + [a.view(np.uint8) for a in ints])
    d = torch.from_numpy(blob).to(device, non_blocking=True)
    at = xy.size * 8                                                       # the doubles first: every view is aligned
    views = [d[:at].view(torch.float64)]
    for a in ints:
        views.append(d[at:at + 4 * a.size].view(torch.int32))
        at += 4 * a.size
    starts = torch.empty(int(table_offsets[-1]), dtype=torch.int32, device=device)
    poly_crossings(views[0], views[1], len(vert_offsets) - 1, h, w, views[2], starts)
    return (starts, views[2], views[3:]) if len(extra) else (starts, views[2])
