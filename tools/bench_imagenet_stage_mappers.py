"""Measurement of the two ImageNet stage mappers at the shipped shape: a decoded 500 x 375 image on the 640 canvas
(resized to 480 x 640), one Detic object mask for DeviceProposalGenerationMapper and 8 saved part masks for
DeviceImagenetPartRankingMapper.  Beside the ranking mapper's mask route (run-length parse, one upload, ONE
pd_rle_sample_groups_canvas_u8 launch) the composition that was available before that entry existed: functions.rle.decode_masks of the n
parts + any(0) + a zero canvas + a slice copy.  The two routes alternate in one process on the same inputs, `--repeats` windows each after
a warm-up; per window the host clock (device synchronised at the end) and the time between two device events around the window.  No
threshold is set.  Prints one JSON line; `--out FILE` also writes it."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from partdistillation_amd import lib
from partdistillation_amd.data import DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper
from partdistillation_amd.functions.input_pipeline import base_canvas, rle_sample_groups, to_device
from partdistillation_amd.functions import rle as device_rle
from partdistillation_amd.utils import rle

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=300, help="timed images per window")
ap.add_argument("--repeats", type=int, default=5, help="timed windows per route; the median is reported, all are listed")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_imagenet_stage_mappers: needs a GPU (nothing is measured without one)")
lib.load()

H, W, S, N_PART, N_REC = 375, 500, 640, 8, 16
rng = np.random.RandomState(0)
ranking = DeviceImagenetPartRankingMapper(S, {"n0123": 0}, rng=np.random.RandomState(1))
generation = DeviceProposalGenerationMapper(S, True, rng=np.random.RandomState(1))
(BH, BW), _ = base_canvas(H, W, S, True)


def part_masks(n):
    """n disjoint Voronoi cells inside an ellipse at the resized size: what stage 1 saves"""
    ys, xs = np.mgrid[0:BH, 0:BW]
    seeds = rng.rand(n, 2) * [BH, BW]
    lab = np.argmin((ys[None] - seeds[:, 0, None, None]) ** 2 + (xs[None] - seeds[:, 1, None, None]) ** 2, axis=0)
    inside = ((ys - BH / 2) ** 2 / (0.17 * BH * BH) + (xs - BW / 2) ** 2 / (0.12 * BW * BW)) < 1.0
    return np.stack([(lab == i) & inside for i in range(n)])


def segs(masks):
    return [{"segmentation": rle.encode(m)} for m in masks]


rank_records, gen_records = [], []
for i in range(N_REC):
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    parts = part_masks(N_PART)
    rank_records.append({"file_name": f"n0123/{i}.JPEG", "class_code": "n0123", "image": image, "pseudo_annotations": segs(parts)})
    gen_records.append({"file_path": f"n0123/{i}.JPEG", "file_name": f"{i}.JPEG", "class_code": "n0123", "image": image,
                        "pseudo_annotations": segs(parts.any(0)[None])})


def new_route(record):
    s = [a["segmentation"] for a in record["pseudo_annotations"]]
    table, cuts = ranking.tables(s, BH, BW)
    starts, offsets, sx, sy, d_go, d_gm = torch.tensor_split(to_device(table, "cuda"), cuts.tolist())
    return rle_sample_groups(starts, offsets, BH, BW, sx, sy, [0, len(s)], np.arange(len(s)), uploaded=(d_go, d_gm), canvas=(S, S))[0]


def parent_route(record):
    union = device_rle.decode_masks(record["pseudo_annotations"], (BH, BW), "cuda").any(0)
    canvas = torch.zeros((1, S, S), dtype=torch.bool, device="cuda")
    canvas[0, :BH, :BW] = union
    return canvas


def window(fn, records, n):
    """-> (host seconds per image, device-event seconds per image)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(n):
        fn(records[i % N_REC])
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, e0.elapsed_time(e1) * 1e-3 / n


for r in rank_records:                                                     # the two routes agree before anything is timed
    assert torch.equal(new_route(r).view(torch.bool), parent_route(r))
runs = {"ranking_mapper": (ranking, rank_records), "generation_mapper": (generation, gen_records), "mask_route_new": (new_route, rank_records),
        "mask_route_parent": (parent_route, rank_records)}
for fn, recs in runs.values():                                             # code objects, allocator
    window(fn, recs, 32)
times = {k: [] for k in runs}
for _ in range(args.repeats):                                              # the same order in every repeat: the routes alternate
    for k, (fn, recs) in runs.items():
        times[k].append(window(fn, recs, args.images))


def summary(ts):
    host, dev = [t[0] * 1e3 for t in ts], [t[1] * 1e3 for t in ts]
    return {"host_ms_per_image_median": float(np.median(host)), "host_ms_per_image_windows": host,
            "device_event_ms_per_image_median": float(np.median(dev)), "device_event_ms_per_image_windows": dev}


res = {k: summary(v) for k, v in times.items()}
parent = res["mask_route_parent"]["host_ms_per_image_windows"]
line = json.dumps({"workload": f"ImageNet stage mappers: {W}x{H} image on the {S} canvas (resized {BW}x{BH}), {N_PART} part masks (ranking), "
                               "1 object mask (generation)", **res,
                   "mask_route_parent_host_spread_ms": max(parent) - min(parent),
                   "timed_images_per_window": args.images, "windows": args.repeats,
                   "timing": "host clock around the whole per-image calls of a window, device synchronised at its end; device-event time = between "
                             "two events recorded around the same window (it includes the host's gaps between launches); the mask routes "
                             "include the run-length parse and the upload"})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
