"""Times the device COCO-RLE codec (functions/rle.py) next to the route it replaces, in one process:
    python tools/bench_rle_codec.py [--calls 10] [--warmup 3]

One JSON line per case; wall clock per image (host string step included, device idle before and after; the two routes alternate in 5 rounds
of `calls` calls: median, and min / max over the rounds) and device-event time of the kernels alone (the C entry called on prepared buffers):
  encode_masks      8 masks at 1024^2      new: encode_masks(masks)            parent: masks_to_coco_json(masks.cpu())
  encode_label_map  one 1024^2 label map   new: encode_label_map(labels)       parent: ProposalGenerationModel._result's ATen chain (transpose
                                                                               copy, compare, nonzero, diff, cat, one read) + runs_to_coco_json
  decode_label_map  5 masks at 640^2       new: decode_label_map(segs)         parent: rle.decode of every mask + the numpy cmask + its upload
The parent's rle.decode here already runs on the vectorised string_to_counts, so its time is a lower bound of what the parent commit took.
bus_bytes: what crosses between host and device per image on either route.  The masks are smooth blobs (a coarse random field, upsampled
and thresholded)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from partdistillation_amd import lib as _lib  # noqa: E402
from partdistillation_amd.functions import rle as device_rle  # noqa: E402
from partdistillation_amd.utils import rle  # noqa: E402


def wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def wall_pair(new, parent, calls, warmup, rounds=5):
    """the two routes in alternating rounds of `calls` calls -> {median, min and max over the rounds} of each"""
    for _ in range(warmup):
        new()
        parent()
    t = {"new": [], "parent": []}
    for _ in range(rounds):
        t["new"].append(wall(new, calls))
        t["parent"].append(wall(parent, calls))
    out = {}
    for k, v in t.items():
        out[f"{k}_wall_ms"], out[f"{k}_wall_ms_min_max"] = float(np.median(v)), [round(min(v), 3), round(max(v), 3)]
    return out


def events(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def field(n, size, g, cells=24):
    coarse = torch.rand((n, 1, cells, cells), generator=g)
    return torch.nn.functional.interpolate(coarse, size=(size, size), mode="bicubic", align_corners=False)[:, 0]


def runs_kernels(planes, binary, total):
    """the three launches of pd_rle_plane_runs on buffers that hold the whole table"""
    lib = _lib.load()
    n, H, W = planes.shape
    work = torch.empty(lib.pd_rle_runs_workspace_bytes(n, H, W), dtype=torch.uint8, device="cuda")
    starts = torch.empty(total, dtype=torch.int32, device="cuda")
    values = torch.empty(total, dtype=torch.uint8, device="cuda")
    offsets, nonzero = torch.empty(n + 1, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    st = _lib.current_stream()
    return lambda: _lib.check(lib.pd_rle_plane_runs(planes.data_ptr(), H * W, n, H, W, int(binary), total, starts.data_ptr(), values.data_ptr(),
                                                    offsets.data_ptr(), nonzero.data_ptr(), work.data_ptr(), st))


def aten_chain(labels):
    """the run table of a label map the way ProposalGenerationModel._result formed it before the codec"""
    flat = labels.t().contiguous().flatten()
    starts = torch.cat([flat.new_zeros(1, dtype=torch.long), (flat[1:] != flat[:-1]).nonzero().flatten() + 1])
    lengths = torch.diff(starts, append=starts.new_tensor([flat.numel()]))
    runs = torch.cat([flat[starts].long(), lengths]).cpu().numpy()
    return runs[:runs.size // 2].astype("uint8"), runs[runs.size // 2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    c, w = args.calls, args.warmup

    # ---- 8 masks at 1024^2
    masks = (field(8, 1024, g) > 0.5).cuda()
    segs, _ = device_rle.encode_masks(masks)
    assert segs == rle.masks_to_coco_json(masks.cpu())
    offsets = device_rle.plane_runs(masks, True)[0]
    total = int(offsets[-1])
    out = {"case": "encode_masks", "shape": [8, 1024, 1024], "runs_per_mask": total // 8,
           **wall_pair(lambda: device_rle.encode_masks(masks), lambda: rle.masks_to_coco_json(masks.cpu()), c, w),
           "kernels_ms": events(runs_kernels(masks.view(torch.uint8), True, total), c, w),
           "bus_bytes_new": 5 * total + 12 * 8 + 4, "bus_bytes_parent": masks.numel()}
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}), flush=True)

    # ---- one 1024^2 label map with 4 labels inside an object
    f = field(2, 1024, g)
    labels = (torch.where(f[0] > 0.45, (f[1] * 4).clamp(0, 3).long() + 1, 0)).to(torch.uint8).cuda()
    segs, counts = device_rle.encode_label_map(labels)
    present = [int(l) for l in np.flatnonzero(counts[1:]) + 1]
    assert segs == rle.labels_to_coco_json(labels.cpu().numpy(), present)
    total = int(device_rle.plane_runs(labels[None], False)[0][-1])

    def parent_label_map():
        values, lengths = aten_chain(labels)
        return rle.runs_to_coco_json(values, lengths, (1024, 1024), present)
    assert parent_label_map() == segs
    out = {"case": "encode_label_map", "shape": [1024, 1024], "runs": total,
           **wall_pair(lambda: device_rle.encode_label_map(labels), parent_label_map, c, w),
           "kernels_ms": events(runs_kernels(labels[None], False, total), c, w), "parent_device_ms": events(lambda: aten_chain(labels), c, w),
           "bus_bytes_new": 5 * total + 16, "bus_bytes_parent": 16 * total}
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}), flush=True)

    # ---- 5 masks at 640^2 -> label map
    m5 = (field(5, 640, g) > 0.55).numpy()
    segs = rle.masks_to_coco_json(m5)

    def parent_decode():
        bmask = np.stack([rle.decode(m["segmentation"]) for m in segs])
        cmask = (bmask.astype(np.int64) * (np.arange(5, dtype=np.int64) + 1)[:, None, None]).sum(0)
        return torch.from_numpy(cmask).cuda()
    assert torch.equal(parent_decode(), device_rle.decode_label_map(segs, (640, 640), "cuda").long())
    starts, offs = rle.segmentations_to_starts([s["segmentation"] for s in segs], (640, 640))
    st_d, off_d = torch.from_numpy(starts).cuda(), torch.from_numpy(offs).cuda()
    lab = torch.empty((640, 640), dtype=torch.int32, device="cuda")
    lib, stream = _lib.load(), _lib.current_stream()
    out = {"case": "decode_label_map", "shape": [5, 640, 640], "runs_per_mask": len(starts) // 5,
           **wall_pair(lambda: device_rle.decode_label_map(segs, (640, 640), "cuda"), parent_decode, c, w),
           "kernels_ms": events(lambda: _lib.check(lib.pd_rle_decode(st_d.data_ptr(), off_d.data_ptr(), 5, 640, 640, lab.data_ptr(), None, stream)),
                                c, w),
           "bus_bytes_new": 4 * (len(starts) + len(offs)), "bus_bytes_parent": 8 * 640 * 640}
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}), flush=True)


if __name__ == "__main__":
    main()
