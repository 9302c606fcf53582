"""Times the Cityscapes-Part record builder (data/cityscapes_part_record.py) next to the host route it replaces, in one process:
    python tools/bench_cityscapes_part_record.py [--calls 5] [--warmup 2] [--objects 20]

One JSON line: wall clock per image of `load_object_and_parts(record, tif_path)` at 1024 x 2048 with `--objects` RLE objects (device idle
before and after, the TIFF decode and the host string step included) and of the reference's function restated in numpy
(tests/cityscapes_part_oracle.py: TIFF decode, uid table, np.where / np.unique and one encode per object and part) on this machine's CPU,
the two routes alternating in 3 rounds of `calls` calls: median, and min / max over the rounds.  The results of both routes are compared
before anything is timed.  The objects are ellipses (cars, persons, riders, trucks, buses and a few of other classes) over a uid map
whose part ids change in blocks of 16 x 16 pixels."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cityscapes_part_oracle as O  # noqa: E402
from partdistillation_amd.data.cityscapes_part_record import load_object_and_parts  # noqa: E402
from partdistillation_amd.utils import rle  # noqa: E402

H, W = 1024, 2048


def scene(rng, n_obj):
    ys, xs = np.mgrid[0:H, 0:W]
    annos = []
    for i in range(n_obj):
        cx, cy, rx, ry = rng.uniform(0.1, 0.9) * W, rng.uniform(0.3, 0.8) * H, rng.uniform(30, 200), rng.uniform(30, 150)
        m = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 < 1.0
        cat = int(rng.randint(0, 5)) if i % 7 else 6
        annos.append({"category_id": cat, "iscrowd": 0, "bbox": [cx - rx, cy - ry, cx + rx, cy + ry], "bbox_mode": 0, "segmentation": rle.encode(m)})
    block = (ys // 16) * 131 + xs // 16
    sid, iid, pid = 24 + block % 5, block % 1000, block % 6
    uids = np.where(block % 4 == 0, sid, np.where(block % 4 == 1, sid * 1000 + iid, sid * 100000 + iid * 100 + pid)).astype(np.int32)
    return {"file_name": "bench_leftImg8bit.png", "image_id": "bench", "height": H, "width": W, "annotations": annos}, uids


def wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--objects", type=int, default=20)
    args = ap.parse_args()
    record, uids = scene(np.random.RandomState(0), args.objects)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench_gtFinePanopticParts.tif")
        Image.fromarray(uids).save(path)

        def device():
            return load_object_and_parts(record, path, "cuda")

        def host():
            return O.load_object_and_parts(record, np.array(Image.open(path)))
        got, want = device(), host()
        assert got == want, "the device record differs from the oracle's"
        for _ in range(args.warmup):
            device()
        t = {"device": [], "host": []}
        for _ in range(3):
            t["device"].append(wall(device, args.calls))
            t["host"].append(wall(host, max(1, args.calls // 2)))
    out = {"case": "load_object_and_parts", "shape": [H, W], "objects": len(got[0]), "parts": sum(len(p) for p in got[1])}
    for k, v in t.items():
        out[f"{k}_wall_ms"], out[f"{k}_wall_ms_min_max"] = round(float(np.median(v)), 3), [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
