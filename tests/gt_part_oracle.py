"""Test helper (not collected): the reference's ground-truth part mappers (data/dataset_mappers/voc_parts_mapper.py and
cityscapes_part_mapper.py) composed from the pinned pieces of oracle/input_pipeline_ref.py — `resize_bilinear_u8`, `resize_nearest`,
`rle_decode` — as resize -> `[:, ::-1]` -> slice on dense arrays, followed by the reference's filtering and merging written as its plain
per-object, per-class loops.  detectron2 is absent: the draws, ResizeShortestEdge.get_output_shape and the box arithmetic are restated from
detectron2 0.6 (draw order UNPINNED, as in oracle/input_pipeline_ref.py; box coordinates in float64)."""
import numpy as np

from oracle import input_pipeline_ref as R

FLAVOURS = {"voc": dict(num_repeats=100, min_parts=2, by_box=True, class_key="orig_part_category_id"),
            "city": dict(num_repeats=20, min_parts=1, by_box=False, class_key="part_category_id")}


def output_shape(h, w, size, max_size):
    scale = size * 1.0 / min(h, w)
    newh, neww = (size * 1.0, scale * w) if h < w else (scale * h, size * 1.0)
    if max(newh, neww) > max_size:
        s = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * s, neww * s
    return int(newh + 0.5), int(neww + 0.5)


def draw(rng, h, w, sizes, max_size, style, flip, crop):
    """[ResizeShortestEdge, RandomFlip?, RandomCrop?].get_transform in list order; crop = (type, size) or None"""
    size = rng.randint(sizes[0], sizes[1] + 1) if style == "range" else rng.choice(sizes)
    rh, rw = (h, w) if size == 0 else output_shape(h, w, size, max_size)
    p = {"in_h": h, "in_w": w, "resize": (rh, rw), "flip": bool(flip and rng.uniform() < 0.5), "crop": (0, 0, rw, rh)}
    if crop is not None:
        kind, cs = crop
        if kind == "relative":
            ch, cw = int(rh * cs[0] + 0.5), int(rw * cs[1] + 0.5)
        elif kind == "relative_range":
            c32 = np.asarray(cs, dtype=np.float32)
            chf, cwf = c32 + rng.rand(2) * (1 - c32)
            ch, cw = int(rh * chf + 0.5), int(rw * cwf + 0.5)
        else:
            assert kind == "absolute"
            ch, cw = min(cs[0], rh), min(cs[1], rw)
        y0 = rng.randint(rh - ch + 1)
        x0 = rng.randint(rw - cw + 1)
        p["crop"] = (int(x0), int(y0), int(cw), int(ch))
    return p


def chain_image(img, p):
    """uint8 [H, W, 3] -> uint8 [ch, cw, 3]"""
    rh, rw = p["resize"]
    out = R.resize_bilinear_u8(img, rh, rw)
    if p["flip"]:
        out = out[:, ::-1]
    x0, y0, cw, ch = p["crop"]
    return out[y0:y0 + ch, x0:x0 + cw]


def chain_mask(mask, p):
    """bool [H, W] -> bool [ch, cw]"""
    rh, rw = p["resize"]
    out = R.resize_nearest(mask, rh, rw)
    if p["flip"]:
        out = out[:, ::-1]
    x0, y0, cw, ch = p["crop"]
    return out[y0:y0 + ch, x0:x0 + cw]


def decode(seg):
    counts = seg["counts"]
    counts = R.rle_string_to_counts(counts) if isinstance(counts, (str, bytes)) else np.asarray(counts, dtype=np.int64)
    return R.rle_decode(counts, int(seg["size"][0]), int(seg["size"][1]))


def box_ref(box, p):
    """one XYXY box corner by corner: resize scale, flip w - x, crop offset, min / max of the four corners, clip to the output"""
    (rh, rw), (cx, cy, cw, ch) = p["resize"], p["crop"]
    xs, ys = [], []
    for x, y in ((box[0], box[1]), (box[2], box[1]), (box[0], box[3]), (box[2], box[3])):
        x, y = float(x) * (rw * 1.0 / p["in_w"]), float(y) * (rh * 1.0 / p["in_h"])
        if p["flip"]:
            x = rw - x
        xs.append(x - cx)
        ys.append(y - cy)
    lo_x, lo_y, hi_x, hi_y = max(min(xs), 0.0), max(min(ys), 0.0), max(max(xs), 0.0), max(max(ys), 0.0)
    return [min(lo_x, float(cw)), min(lo_y, float(ch)), min(hi_x, float(cw)), min(hi_y, float(ch))]


def _nonempty_box(b):
    return (b[2] - b[0]) > 1e-5 and (b[3] - b[1]) > 1e-5


def forward(record, image, flavour, p, merged):
    """the reference's _forward_with_aug for drawn parameters p -> dict of numpy results"""
    F = FLAVOURS[flavour]
    objs = [(i, o) for i, o in enumerate(record["annotations"]) if o.get("iscrowd", 0) == 0]
    keep_objs = []
    for i, o in objs:                                                      # _transform_annotations + filter_empty_instances
        m = chain_mask(decode(o["segmentation"]), p)
        b = box_ref(o["bbox"], p)
        if m.any() and (_nonempty_box(b) or not F["by_box"]):
            keep_objs.append((i, o, m, b))
    parts_list = [record["part_annotations"][i] for i, _, _, _ in keep_objs]
    flat = [(oid, part) for oid, parts in enumerate(parts_list) for part in parts]
    kept = []                                                              # (obj_mapping, part_mapping, class, mask)
    for k, (oid, part) in enumerate(flat):
        m = chain_mask(decode(part["segmentation"]), p)
        if m.any() and (not F["by_box"] or _nonempty_box(box_ref(part["bbox"], p))):
            kept.append((oid, k, int(part[F["class_key"]]), m))
    x0, y0, cw, ch = p["crop"]
    if merged:
        planes, classes = [], []
        for oid in sorted(set(k[0] for k in kept)):
            mine = [k for k in kept if k[0] == oid]
            for pid in sorted(set(k[2] for k in mine)):
                planes.append(np.sum([k[3] for k in mine if k[2] == pid], axis=0).astype(bool))
                classes.append(pid)
    else:
        planes, classes = [k[3] for k in kept], [k[2] for k in kept]
    stack = lambda ms: np.stack(ms) if len(ms) else np.zeros((0, ch, cw), dtype=bool)
    return {"image": chain_image(image, p).transpose(2, 0, 1), "size": (ch, cw),
            "obj_masks": stack([k[2] for k in keep_objs]), "obj_classes": [int(k[1]["category_id"]) for k in keep_objs],
            "obj_boxes": np.asarray([k[3] for k in keep_objs], dtype=np.float64).reshape(-1, 4), "obj_mapping": [k[0] for k in keep_objs],
            "part_masks": stack(planes), "part_classes": classes, "part_obj_mapping": [k[0] for k in kept],
            "part_mapping": [k[1] for k in kept], "orig_part_maps": [flat[k[1]][1]["segmentation"] for k in kept]}


def call(record, image, flavour, rng, is_train, sizes, max_size, style, crop, merged, num_repeats=None):
    """the reference's __call__: train = up to num_repeats attempts with the crop, then one pass without it; test = one pass.
    -> (forward's dict, attempts made with the crop (0 in test mode), True when the pass without the crop was taken)"""
    F = FLAVOURS[flavour]
    h, w = image.shape[:2]
    if not is_train:
        return forward(record, image, flavour, draw(rng, h, w, sizes, max_size, style, False, None), merged), 0, False
    repeats = F["num_repeats"] if num_repeats is None else num_repeats
    for attempt in range(repeats):
        out = forward(record, image, flavour, draw(rng, h, w, sizes, max_size, style, True, crop), merged)
        if len(out["part_classes"]) >= F["min_parts"]:
            return out, attempt + 1, False
    return forward(record, image, flavour, draw(rng, h, w, sizes, max_size, style, True, None), merged), repeats, True


# ------------------------------------------------------------------------------------------------ scenes
def tight_box(mask):
    """XYXY of the first / last set column and row — a one-pixel-wide mask has zero width (the Pascal-Part registration's boxes)"""
    ys, xs = np.nonzero(mask)
    return [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]


def encode(mask):
    from partdistillation_amd.utils import rle
    return rle.encode(np.asarray(mask, dtype=bool))


def record(obj_masks, obj_classes, part_masks, part_classes, flavour, **extra):
    """obj_masks [n] bool planes, part_masks / part_classes: one list per object -> dataset record (without the image)"""
    key = FLAVOURS[flavour]["class_key"]
    annos, parts = [], []
    for m, c, pms, pcs in zip(obj_masks, obj_classes, part_masks, part_classes):
        annos.append({"segmentation": encode(m), "bbox": tight_box(m), "bbox_mode": 0, "category_id": int(c)})
        plist = []
        for pm, pc in zip(pms, pcs):
            part = {"segmentation": encode(pm), key: int(pc)}
            if flavour == "voc":
                part.update(bbox=tight_box(pm), bbox_mode=0)
            plist.append(part)
        parts.append(plist)
    h, w = obj_masks[0].shape
    out = {"file_name": "x.png", "image_id": 7, "height": h, "width": w, "annotations": annos, "part_annotations": parts}
    out.update(extra)
    return out


def scene(rng, H, W, n_obj=3, n_parts=4, n_classes=3):
    """n_obj side-by-side elliptical objects, each cut into n_parts Voronoi cells whose classes repeat (so merging has work to do)"""
    ys, xs = np.mgrid[0:H, 0:W]
    obj_masks, obj_classes, part_masks, part_classes = [], [], [], []
    for o in range(n_obj):
        cx, cy, rx, ry = (o + 0.5) * W / n_obj, H * (0.4 + 0.2 * rng.rand()), 0.45 * W / n_obj, H * (0.25 + 0.15 * rng.rand())
        obj = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 < 1.0
        seeds = np.stack([cy + (rng.rand(n_parts) - 0.5) * 2 * ry, cx + (rng.rand(n_parts) - 0.5) * 2 * rx], axis=1)
        lab = np.argmin((ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2, axis=0)
        cells = [(lab == k) & obj for k in range(n_parts)]
        cells = [c for c in cells if c.any()]
        obj_masks.append(obj)
        obj_classes.append(int(rng.randint(0, 5)))
        part_masks.append(cells)
        part_classes.append([int(c) for c in rng.randint(0, n_classes, len(cells))])
    return obj_masks, obj_classes, part_masks, part_classes
