"""Measurement of the PartImageNet mapper: a decoded ImageNet-sized image (500 x 375) whose record has 6 parts x 2
polygons x 60 vertices goes through ResizeShortestEdge(640) -> RandomFlip and the merge to one mask per part class.  Device path =
partdistillation_amd.data.DevicePartImageNetMapper (host draws, vertex transform and table offsets, one upload, the two resample kernels,
pd_poly_crossings_i32, pd_rle_sample_groups_u8, no synchronisation).  Beside it, FOR SCALE ONLY, the serial rasteriser restated in Python
(tests/poly_oracle.py, the CPU oracle of the tests) on the same record's polygons at the same output size: it is an interpreter loop, not
pycocotools' C, so the ratio says nothing about the reference.  No threshold is set.  Prints one JSON line; `--out FILE` also writes it."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from partdistillation_amd import lib
from partdistillation_amd.data import DevicePartImageNetMapper
from partdistillation_amd.data.gt_part_mapper import get_output_shape

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=1000, help="timed device images per window")
ap.add_argument("--repeats", type=int, default=3, help="timed windows; the median is reported, all are listed")
ap.add_argument("--oracle-images", type=int, default=2, help="images the Python oracle rasterises (slow; for scale only)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_part_imagenet_mapper: needs a GPU (nothing is measured without one)")
lib.load()

H, W, SHORT, MAX, N_PART, N_POLY, N_VERT, N_CLS = 375, 500, 640, 1333, 6, 2, 60, 4
rng = np.random.RandomState(0)


def blob(cx, cy, r):
    """a star-shaped polygon of N_VERT vertices around (cx, cy)"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, N_VERT))
    rad = r * rng.uniform(0.6, 1.0, N_VERT)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).reshape(-1).tolist()


records = []
for i in range(16):
    annos = []
    for part in range(N_PART):
        cx, cy = W * (0.2 + 0.6 * rng.rand()), H * (0.2 + 0.6 * rng.rand())
        annos.append({"category_id": int(rng.randint(N_CLS)), "bbox": [0.0, 0.0, 1.0, 1.0], "bbox_mode": 1,
                      "segmentation": [blob(cx + 30 * k, cy + 20 * k, 40 + 30 * rng.rand()) for k in range(N_POLY)]})
    records.append({"file_name": f"val/n0123_{i}.JPEG", "image_id": i, "height": H, "width": W, "annotations": annos,
                    "image": rng.randint(0, 256, (H, W, 3)).astype(np.uint8)})
mapper = DevicePartImageNetMapper(True, (SHORT,), MAX, "choice", use_merged_gt=True, rng=np.random.RandomState(1),
                                  class_code_to_class_id={"n0123": 0})


def device_pass(n):
    for i in range(n):
        out = mapper(records[i % 16])
    torch.cuda.synchronize()
    return out


def oracle_pass(n):
    import poly_oracle as P
    p = {"in_h": H, "in_w": W, "resize": get_output_shape(H, W, SHORT, MAX), "flip": False}
    for i in range(n):
        for a in records[i % 16]["annotations"]:
            for q in a["segmentation"]:
                P.mask(P.transform_polygon(q, p).reshape(-1), *p["resize"])


device_pass(32)                                                            # code objects, allocator
t_dev = []
for r in range(args.repeats):
    t0 = time.perf_counter(); device_pass(args.images); t_dev.append((time.perf_counter() - t0) / args.images)
t0 = time.perf_counter(); oracle_pass(args.oracle_images); t_oracle = (time.perf_counter() - t0) / max(args.oracle_images, 1)
dev = float(np.median(t_dev))
line = json.dumps({"workload": f"PartImageNet mapper (train, merged): {W}x{H} image, {N_PART} parts x {N_POLY} polygons x {N_VERT} vertices, short edge "
                               f"{SHORT} -> flip, rasterised at the output size",
                   "device_ms_per_image": dev * 1e3, "device_images_per_s": 1 / dev, "device_ms_per_image_windows": [t * 1e3 for t in t_dev],
                   "device_ms_per_image_range": [min(t_dev) * 1e3, max(t_dev) * 1e3],
                   "python_oracle_rasteriser_ms_per_image_for_scale_only": t_oracle * 1e3,
                   "timed_images": {"device": args.images, "python_oracle": args.oracle_images},
                   "timing": "host clock around the whole per-image call, device synchronised at the end of each window; the oracle figure covers "
                             "the polygon rasterisation alone (no image resize), in an interpreter loop"})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
