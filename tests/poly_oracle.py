"""Test helper (not collected): pycocotools' polygon rasteriser (rleFrPoly) restated literally in Python — C doubles are Python floats,
`(int)` is int() (truncation toward zero), the walk over every point of every edge is a plain loop — and the reference's PartImageNet mapper
(data/dataset_mappers/part_imagenet_mapper.py) composed from it and from the Pillow-exact image chain of gt_part_oracle.py.  pycocotools
and detectron2 are absent: parity with them is UNPINNED; what is pinned is this restatement against an independent even-odd test
(test_part_imagenet_mapper_cpu.py) and the device against this restatement."""
import math
from fractions import Fraction

import numpy as np

import gt_part_oracle as G

SCALE = 5.0
# upsampled integer vertices (divide by 5) of triangles whose table on a 24 x 24 canvas changes when `start + slope * t` is fused
CONTRACTION_TRIANGLES = (((36, 68), (4, 60), (76, 0)), ((3, 104), (103, 14), (89, 35)), ((17, 74), (98, 25), (80, 8)), ((8, 65), (86, 0), (4, 32)))


# ------------------------------------------------------------------------------------------------ the rasteriser, step by step
def upsample(poly):
    """step 1: flat [x0, y0, ...] -> closed integer lists X, Y of k + 1 entries"""
    xy = [float(v) for v in np.asarray(poly, dtype=np.float64).reshape(-1)]
    k = len(xy) // 2
    X = [int(SCALE * xy[2 * j] + .5) for j in range(k)]
    Y = [int(SCALE * xy[2 * j + 1] + .5) for j in range(k)]
    return X + X[:1], Y + Y[:1]


def _unfused(start, s, t):
    return int(start + s * t + .5)


def _fused(start, s, t):
    """int(fma(s, t, start) + .5): the product and the first sum rounded ONCE (exact rational arithmetic, then one rounding to double)"""
    return int(float(Fraction(s) * t + start) + .5)


def boundary_points(poly, fused=False):
    """step 2: the dense (u, v) points along the outline, edge after edge, in the original direction of every edge; a zero-length edge
    (0 / 0 in the original, one point that can never take part in a crossing) contributes nothing"""
    X, Y = upsample(poly)
    point = _fused if fused else _unfused
    u, v = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        if dx == 0 and dy == 0:
            continue
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(point(ys, s, t))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(point(xs, s, t))
    return u, v


def crossings(poly, h, w, fused=False):
    """step 3: the boundary positions a = x * h + y, in the order of the walk (unsorted)"""
    u, v = boundary_points(poly, fused)
    out = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j - 1])
            xd = (xd + .5) / SCALE - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / SCALE - .5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            out.append(int(xd) * h + int(yd))
    return out


def table(poly, h, w, fused=False):
    """step 4 as a run-starts table (include/pd_input.h): [0] + sorted(a), int32"""
    return np.asarray([0] + sorted(crossings(poly, h, w, fused)), dtype=np.int32)


def table_mask(tab, h, w):
    """pixel p of the column-major flattening is set iff the number of a <= p is odd (the leading 0 of the table is not an a)"""
    a = np.asarray(tab[1:], dtype=np.int64)
    parity = np.searchsorted(np.sort(a), np.arange(h * w), side="right") % 2 == 1
    return parity.reshape(w, h).T


def mask(poly, h, w, fused=False):
    return table_mask(table(poly, h, w, fused), h, w)


def run_merge_counts(poly, h, w):
    """the original's ending: append h * w, sort, difference, then merge the zero-length runs -> COCO run lengths (first run = zeros)"""
    a = sorted(crossings(poly, h, w) + [h * w])
    p, d = 0, []
    for t in a:
        d.append(t - p)
        p = t
    b, j = [d[0]], 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j])
            j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]
                j += 1
    return b


def counts_mask(counts, h, w):
    """COCO run lengths -> bool [h, w]"""
    flat = np.zeros(h * w, dtype=bool)
    pos, val = 0, False
    for c in counts:
        if val:
            flat[pos:pos + c] = True
        pos += c
        val = not val
    return flat[:h * w].reshape(w, h).T


# ------------------------------------------------------------------------------------------------ an independent test to pin it against
def even_odd(poly, h, w):
    """even-odd point-in-polygon of the continuous polygon at the pixel centres (x + .5, y + .5) — where the rasteriser's column 5 x + 2.5
    and its row rounding sit — and the distance of every centre to the outline -> (inside bool [h, w], distance float [h, w])"""
    pts = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64) + .5
    inside = np.zeros((h, w), dtype=bool)
    dist = np.full((h, w), np.inf)
    for j in range(len(pts)):
        (x0, y0), (x1, y1) = pts[j], pts[(j + 1) % len(pts)]
        cond = (y0 > ys) != (y1 > ys)
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = x0 + (ys - y0) * (x1 - x0) / (y1 - y0)
        inside ^= cond & (xs < xi)
        ex, ey = x1 - x0, y1 - y0
        L2 = ex * ex + ey * ey
        t = np.clip(((xs - x0) * ex + (ys - y0) * ey) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(xs)
        dist = np.minimum(dist, np.hypot(xs - (x0 + t * ex), ys - (y0 + t * ey)))
    return inside, dist


# ------------------------------------------------------------------------------------------------ the mapper
def correct_path(file_name):
    """dir/n0123_456.JPEG -> (dir/n0123/n0123_456.JPEG, n0123)"""
    parts = file_name.split("/")
    code = parts[-1].split("_")[0]
    return "/".join(parts[:-1] + [code, parts[-1]]), code


def draw(rng, h, w, sizes, max_size, style, is_train):
    """[ResizeShortestEdge, RandomFlip (train)].get_transform in list order"""
    return G.draw(rng, h, w, sizes, max_size, style, is_train, None)


def identity_params(h, w):
    return {"in_h": h, "in_w": w, "resize": (h, w), "flip": False, "crop": (0, 0, w, h)}


def transform_polygon(poly, p):
    pts = np.array(poly, dtype=np.float64).reshape(-1, 2)
    rh, rw = p["resize"]
    pts[:, 0] = pts[:, 0] * (rw * 1.0 / p["in_w"])
    pts[:, 1] = pts[:, 1] * (rh * 1.0 / p["in_h"])
    if p["flip"]:
        pts[:, 0] = rw - pts[:, 0]
    return pts


def forward(record, image, p, merged, class_map, identity=False):
    """the reference's _forward_with_aug for drawn parameters p (identity: the empty list, the image untouched) -> dict of numpy
    results, or None when there is no annotation with iscrowd == 0 (no gt_masks field)"""
    annos = [a for a in record["annotations"] if a.get("iscrowd", 0) == 0]
    if not annos:
        return None
    rh, rw = p["resize"]
    file_name, code = correct_path(record["file_name"])
    parts = []                                                             # (class, polygons, float32 box)
    for a in annos:
        polys = [transform_polygon(q, p) for q in a["segmentation"]]
        for q in polys:
            if q.size % 2 != 0 or q.size < 6:
                raise ValueError(f"Cannot create a polygon from {q.size} coordinates.")
        lo = np.min([q.astype(np.float32).min(axis=0) for q in polys], axis=0)
        hi = np.max([q.astype(np.float32).max(axis=0) for q in polys], axis=0)
        box = np.asarray([lo[0], lo[1], hi[0], hi[1]], dtype=np.float32)
        if (box[2] - box[0]) > np.float32(1e-5) and (box[3] - box[1]) > np.float32(1e-5):
            parts.append((int(a["category_id"]), polys, box))
    masks = [np.any([mask(q.reshape(-1), rh, rw) for q in polys], axis=0) for _, polys, _ in parts]
    classes = [c for c, _, _ in parts]
    if merged:
        uniq = sorted(set(classes))
        part_masks = [np.sum([m for m, c in zip(masks, classes) if c == u], axis=0).astype(bool) for u in uniq]
        part_classes, boxes = uniq, None
    else:
        part_masks, part_classes = masks, classes
        boxes = np.stack([b for _, _, b in parts]) if parts else np.zeros((0, 4), dtype=np.float32)
    stack = lambda ms: np.stack(ms) if len(ms) else np.zeros((0, rh, rw), dtype=bool)
    obj = np.sum(part_masks, axis=0).astype(bool)[None] if part_masks else np.zeros((1, rh, rw), dtype=bool)
    img = image if identity else G.chain_image(image, p)
    return {"image": img.transpose(2, 0, 1), "size": (rh, rw), "file_name": file_name, "class_code": code,
            "obj_masks": obj, "obj_classes": [class_map[code]], "part_masks": stack(part_masks), "part_classes": part_classes,
            "part_boxes": boxes, "n_parts": len(parts)}


def call(record, image, rng, is_train, sizes, max_size, style, merged, class_map, num_repeats=20):
    """the reference's __call__ -> (forward's dict or None, attempts made, True when the pass with the empty list was taken)"""
    h, w = image.shape[:2]
    if not is_train:
        return forward(record, image, draw(rng, h, w, sizes, max_size, style, False), merged, class_map), 0, False
    for attempt in range(num_repeats):
        out = forward(record, image, draw(rng, h, w, sizes, max_size, style, True), merged, class_map)
        if out is None:
            raise ValueError("no annotation: the reference crashes here")
        if out["n_parts"] > 0:
            return out, attempt + 1, False
    return forward(record, image, identity_params(h, w), merged, class_map, identity=True), num_repeats, True
