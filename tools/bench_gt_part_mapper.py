"""Measurement of the ground-truth part mapper: a decoded Pascal-sized image (500 x 375) with 3 objects x 6 parts (COCO
RLE, tight boxes) goes through ResizeShortestEdge(640) -> RandomFlip -> RandomCrop(relative_range 0.9) and the merge to one mask per
(object, part class).  Device path = partdistillation_amd.data.DeviceVOCPartsMapper (host draws + tables, 3 kernels per attempt, one
readback of the counts); host path = the same steps with Pillow (what detectron2's transforms call), a numpy RLE decode and the reference's
per-object, per-class loops, one process, one core — the baseline (the parent commit has no device route).  The two routes run in
alternated windows; the median and the range of the windows are reported.  Prints one JSON line; `--out FILE` also writes it."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image
from partdistillation_amd import lib
from partdistillation_amd.data import DeviceVOCPartsMapper
from partdistillation_amd.data.gt_part_mapper import boxes_nonempty, transform_boxes
from partdistillation_amd.utils import rle

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=1000, help="timed device images per window (the host path times a fifth of them)")
ap.add_argument("--repeats", type=int, default=3, help="timed windows per path; the median is reported, all are listed")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_gt_part_mapper: needs a GPU (nothing is measured without one)")
lib.load()

H, W, SHORT, MAX, N_OBJ, N_PART, N_CLS = 375, 500, 640, 1333, 3, 6, 4
CROP = ("relative_range", (0.9, 0.9))
rng = np.random.RandomState(0)


def tight_box(m):
    ys, xs = np.nonzero(m)
    return [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]


records = []
for i in range(16):
    ys, xs = np.mgrid[0:H, 0:W]
    annos, parts = [], []
    for o in range(N_OBJ):
        cx, cy, rx, ry = (o + 0.5) * W / N_OBJ, H * (0.4 + 0.2 * rng.rand()), 0.45 * W / N_OBJ, H * (0.25 + 0.15 * rng.rand())
        obj = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 < 1.0
        seeds = np.stack([cy + (rng.rand(N_PART) - 0.5) * 1.4 * ry, cx + (rng.rand(N_PART) - 0.5) * 1.4 * rx], axis=1)
        lab = np.argmin((ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2, axis=0)
        annos.append({"segmentation": rle.encode(obj), "bbox": tight_box(obj), "bbox_mode": 0, "category_id": o})
        cells = [(lab == k) & obj for k in range(N_PART)]
        parts.append([{"segmentation": rle.encode(c), "bbox": tight_box(c), "bbox_mode": 0, "orig_part_category_id": int(rng.randint(N_CLS))}
                      for c in cells if c.any()])
    records.append({"file_name": f"{i}.jpg", "image_id": i, "height": H, "width": W, "annotations": annos, "part_annotations": parts,
                    "image": rng.randint(0, 256, (H, W, 3)).astype(np.uint8)})
mapper = DeviceVOCPartsMapper(True, (SHORT,), MAX, "choice", *CROP, use_merged_gt=True, rng=np.random.RandomState(1))


def device_pass(n):
    for i in range(n):
        out = mapper(records[i % 16])
    torch.cuda.synchronize()
    return out


def host_masks(segs, p):
    (rh, rw), (x0, y0, cw, ch) = p["resize"], p["crop"]
    out = []
    for s in segs:
        m = np.asarray(Image.fromarray(rle.decode(s).astype(np.uint8)).resize((rw, rh), Image.NEAREST))
        if p["flip"]:
            m = m[:, ::-1]
        out.append(m[y0:y0 + ch, x0:x0 + cw].astype(bool))
    return out


def host_one(rec, p):
    (rh, rw), (x0, y0, cw, ch) = p["resize"], p["crop"]
    img = np.asarray(Image.fromarray(rec["image"]).resize((rw, rh), Image.BILINEAR))
    if p["flip"]:
        img = img[:, ::-1]
    img = img[y0:y0 + ch, x0:x0 + cw]
    om = host_masks([a["segmentation"] for a in rec["annotations"]], p)
    ok = boxes_nonempty(transform_boxes([a["bbox"] for a in rec["annotations"]], p))
    keep = [i for i in range(len(om)) if ok[i] and om[i].any()]
    flat = [(k, part) for k, i in enumerate(keep) for part in rec["part_annotations"][i]]
    pm = host_masks([part["segmentation"] for _, part in flat], p)
    pok = boxes_nonempty(transform_boxes([part["bbox"] for _, part in flat], p)) if flat else []
    kept = [(k, part["orig_part_category_id"], m) for (k, part), m, b in zip(flat, pm, pok) if b and m.any()]
    merged, classes = [], []
    for oid in sorted(set(k[0] for k in kept)):
        mine = [k for k in kept if k[0] == oid]
        for pid in sorted(set(k[1] for k in mine)):
            merged.append(np.sum([k[2] for k in mine if k[1] == pid], axis=0).astype(bool))
            classes.append(pid)
    return (torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1))), torch.as_tensor(np.stack([om[i] for i in keep])) if keep else None,
            torch.as_tensor(np.stack(merged)) if merged else None, classes)


def host_pass(n, seed):
    draws = DeviceVOCPartsMapper(True, (SHORT,), MAX, "choice", *CROP, device="cpu", rng=np.random.RandomState(seed))
    for i in range(n):
        for attempt in range(draws.num_repeats + 1):                       # the mapper's loop: retry while fewer than two part masks
            out = host_one(records[i % 16], draws.draw(H, W, crop=attempt < draws.num_repeats))
            if len(out[3]) >= draws.min_parts or attempt == draws.num_repeats:
                break
    return out


torch.set_num_threads(1)
device_pass(32)                                                            # code objects, allocator
host_pass(4, 1)
t_dev, t_host = [], []
for r in range(args.repeats):                                              # alternate the two paths: other work shares the host
    t0 = time.perf_counter(); device_pass(args.images); t_dev.append((time.perf_counter() - t0) / args.images)
    n = max(args.images // 5, 1)
    t0 = time.perf_counter(); host_pass(n, 1 + r); t_host.append((time.perf_counter() - t0) / n)
dev, host = float(np.median(t_dev)), float(np.median(t_host))
line = json.dumps({"workload": f"ground-truth part mapper (Pascal flavour, train): {W}x{H} image, {N_OBJ} objects x {N_PART} parts as RLE, short edge "
                               f"{SHORT} -> flip -> crop relative_range 0.9, merged per (object, class)",
                   "device_ms_per_image": dev * 1e3, "device_images_per_s": 1 / dev, "device_ms_per_image_windows": [t * 1e3 for t in t_dev],
                   "device_ms_per_image_range": [min(t_dev) * 1e3, max(t_dev) * 1e3],
                   "host_pillow_numpy_ms_per_image_one_core": host * 1e3, "host_images_per_s_one_core": 1 / host,
                   "host_ms_per_image_windows": [t * 1e3 for t in t_host], "host_ms_per_image_range": [min(t_host) * 1e3, max(t_host) * 1e3],
                   "baseline": "host_pillow_numpy_ms_per_image_one_core", "device_over_host_speedup": host / dev,
                   "timed_images": {"device": args.images, "host": max(args.images // 5, 1)},
                   "timing": "host clock around the whole per-image call, device synchronised at the end of each window; an attempt with fewer than two part masks is retried, in both paths"})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
