"""Measurement of the part-distillation input pipeline: a decoded ImageNet-sized image (500 x 375) is resized to the base
size of the pseudo-labels (640, padded square with 128), then LSJ-augmented to 1024^2 (flip, crop, scale 0.1-2.0, crop, pad) together with 8
labelled part masks (COCO RLE at 640^2).  Device path = partdistillation_amd.data.DevicePartDistillationMapper (host draws + tables, 5
kernels: the base resize once per image, the augmentation per attempt); host path = the same steps with Pillow (what detectron2's transforms
call) and a numpy RLE decode, one process, one core — the baseline.  Prints one JSON line; `--out FILE` also writes it."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image
from partdistillation_amd import lib
from partdistillation_amd.data import DevicePartDistillationMapper
from partdistillation_amd.utils import rle

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=2000, help="timed device images (the host path times a fifth of them)")
ap.add_argument("--repeats", type=int, default=3, help="timed windows per path; the median is reported, all are listed")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_part_distillation_input: needs a GPU (nothing is measured without one)")
lib.load()

S, BASE, H, W, N = 1024, 640, 375, 500, 8
AUG = (S, 0.1, 2.0, "relative_range", (0.9, 0.9))
rng = np.random.RandomState(0)
imgs, annos = [], []
for i in range(16):
    ys, xs = np.mgrid[0:BASE, 0:BASE]
    seeds = rng.rand(N, 2) * [BASE * H / W, BASE]                          # inside the resized image (the top 480 rows of the canvas)
    lab = np.argmin((ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2, axis=0)
    inside = ((ys - 240) ** 2 / (0.17 * 480 * 480) + (xs - 320) ** 2 / (0.12 * 640 * 640)) < 1.0
    imgs.append(rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
    annos.append([{"segmentation": rle.encode((lab == k) & inside), "category_id": k} for k in range(N)])
mapper = DevicePartDistillationMapper(*AUG, rng=np.random.RandomState(1), base_size=BASE, square_base=True)


def device_pass(n):
    for i in range(n):
        out = mapper({"image": imgs[i % 16], "pseudo_annotations": annos[i % 16]})
    torch.cuda.synchronize()
    return out


def host_one(img, ann, p):
    scale = min(BASE / img.shape[0], BASE / img.shape[1])
    bh, bw = int(np.round(img.shape[0] * scale)), int(np.round(img.shape[1] * scale))
    canvas = np.full((BASE, BASE, 3), 128, np.uint8)
    canvas[:bh, :bw] = np.asarray(Image.fromarray(img).resize((bw, bh), Image.BILINEAR))
    img = canvas
    masks = np.stack([rle.decode(a["segmentation"]) for a in ann]).astype(np.uint8)
    if p["flip"]:
        img, masks = img[:, ::-1], masks[:, :, ::-1]
    x0, y0, cw, ch = p["crop1"]
    img, masks = img[y0:y0 + ch, x0:x0 + cw], masks[:, y0:y0 + ch, x0:x0 + cw]
    rh, rw = p["resize"]
    img = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((rw, rh), Image.BILINEAR))
    masks = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(m)).resize((rw, rh), Image.NEAREST)) for m in masks])
    ox, oy = p["crop2"]
    img, masks = img[oy:oy + S, ox:ox + S], masks[:, oy:oy + S, ox:ox + S]
    out = np.full((S, S, 3), 128, np.uint8)
    out[:img.shape[0], :img.shape[1]] = img
    om = np.zeros((N, S, S), bool)
    om[:, :masks.shape[1], :masks.shape[2]] = masks
    area = om.reshape(N, -1).sum(1)
    keep = np.nonzero(area)[0]
    return torch.as_tensor(np.ascontiguousarray(out.transpose(2, 0, 1))), torch.as_tensor(om[keep])


def host_pass(n, seed):
    draws = DevicePartDistillationMapper(*AUG, device="cpu", rng=np.random.RandomState(seed), base_size=BASE, square_base=True)
    for i in range(n):
        for attempt in range(draws.num_repeats + 1):                       # the mapper's loop: retry while no mask survives
            out = host_one(imgs[i % 16], annos[i % 16], draws.draw(BASE, BASE, weak=attempt == draws.num_repeats))
            if len(out[1]) or attempt == draws.num_repeats:
                break
    return out


torch.set_num_threads(1)
device_pass(32)                                                            # every shape class of the window: code objects, allocator
host_pass(4, 1)
t_dev, t_host = [], []
for r in range(args.repeats):                                              # alternate the two paths: other work shares the host
    t0 = time.perf_counter(); device_pass(args.images); t_dev.append((time.perf_counter() - t0) / args.images)
    n = max(args.images // 5, 1)
    t0 = time.perf_counter(); host_pass(n, 1 + r); t_host.append((time.perf_counter() - t0) / n)
dev, host = float(np.median(t_dev)), float(np.median(t_host))
line = json.dumps({"workload": f"part-distillation input: {W}x{H} image -> base {BASE} square -> {S}^2 (flip, crop, scale 0.1-2.0, crop, pad), "
                               f"{N} labelled RLE masks at {BASE}^2",
                   "device_ms_per_image": dev * 1e3, "device_images_per_s": 1 / dev, "device_ms_per_image_windows": [t * 1e3 for t in t_dev],
                   "host_pillow_numpy_ms_per_image_one_core": host * 1e3, "host_images_per_s_one_core": 1 / host,
                   "host_ms_per_image_windows": [t * 1e3 for t in t_host], "baseline": "host_pillow_numpy_ms_per_image_one_core",
                   "device_over_host_speedup": host / dev, "timed_images": {"device": args.images, "host": max(args.images // 5, 1)},
                   "timing": "host clock around the whole per-image call, device synchronised at the end of each window; an attempt that keeps no mask is retried, in both paths"})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
