"""Times the evaluation post-processing of SupervisedModel per image at a resized output, kernel route against dense torch route, in one
process:  python tools/bench_supervised_inference.py [--calls 50] [--warmup 5]

  kernel: pd_masks_resize_u8 (G + 1 masks) + pd_mask_assign_resized + pd_assign_histogram            (what inference_fused enqueues)
  dense : F.interpolate x 2 of [K, H, W] fp32, object mask, sigmoid, score multiply, argmax, max > 0, bincount x (G + 2), plus
          F.interpolate(masks.float()) != 0 for the G + 1 masks                                        (what the dense route enqueues)
Device events around `calls` calls after a warm-up; prints one JSON line per size with microseconds per image and the bytes each route
moves through memory (reads + writes of every tensor it touches, as if nothing stayed in cache)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from partdistillation_amd.functions import mask_assign as A  # noqa: E402
from partdistillation_amd.functions import pixel_grouping as G  # noqa: E402

SIZES = [((683, 1024), (704, 1024), (1365, 2048)), ((768, 1024), (768, 1024), (512, 683))]      # (image, padded, output)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gt", type=int, default=8)
    args = ap.parse_args()
    dev, g = "cuda", torch.Generator().manual_seed(0)
    for (Hi, Wi), (Hp, Wp), (H, W) in SIZES:
        for K in (100, 200):
            h, w, Gn = Hp // 4, Wp // 4, args.gt
            logits = (torch.randn((K, h, w), generator=g) * 2).to(dev)
            scores = torch.rand((K,), generator=g).to(dev)
            ys, xs = torch.meshgrid(torch.arange(Hp) / Hi, torch.arange(Wp) / Wi, indexing="ij")
            obj_p = (((ys - 0.5) ** 2 / 0.17 + (xs - 0.5) ** 2 / 0.12) < 1.0)[None].to(dev)
            gt_p = (torch.rand((Gn, Hp, Wp), generator=g) < 0.3).to(dev) & obj_p

            def kernel():
                (tm, _), (to, _) = G.masks_resize([(gt_p, (Hi, Wi), (H, W)), (obj_p, (Hi, Wi), (H, W))])
                (arg, obj, _, _), = A.mask_assign_resized([(logits, scores, to[0], None, (Hp, Wp), (Hi, Wi), (H, W))])
                return A.assign_histogram([(arg, obj, tm, K)])

            def dense():
                tm = F.interpolate(gt_p[None, :, :Hi, :Wi].float(), size=(H, W), mode="bilinear", align_corners=False)[0] != 0
                to = F.interpolate(obj_p[None, :, :Hi, :Wi].float(), size=(H, W), mode="bilinear", align_corners=False)[0] != 0
                d = F.interpolate(logits[None], size=(Hp, Wp), mode="bilinear", align_corners=False)[0]
                v = F.interpolate(d[None, :, :Hi, :Wi], size=(H, W), mode="bilinear", align_corners=False)[0] * to
                objmap = v.max(0)[0] > 0
                arg = (scores[:, None, None] * v.sigmoid()).argmax(0)
                out = [torch.bincount(arg.flatten(), minlength=K), torch.bincount(arg[objmap], minlength=K)]
                return out + [torch.bincount(arg[objmap & t], minlength=K) for t in tm]
            tk, td = timed(kernel, args.calls, args.warmup), timed(dense, args.calls, args.warmup)
            masks = (Gn + 1) * (Hp * Wp + H * W)
            kb = masks + 4 * K * h * w + H * W * (1 + 2 + 1) + H * W * (2 + 1 + Gn)
            # dense: [K, Hp, Wp] written + read, [K, H, W] written, x object (r + w), max (r), sigmoid (r + w), x scores (r + w), argmax (r);
            # masks as float images (w + r) and bool (w); int64 arg map and its G + 2 masked copies
            db = 4 * K * (h * w + 2 * Hp * Wp) + 4 * K * H * W * 8 + (Gn + 1) * (Hp * Wp + 9 * H * W) + 8 * H * W * (2 * (Gn + 2) + 1)
            print(json.dumps({"image": [Hi, Wi], "output": [H, W], "K": K, "G": Gn, "kernel_us_per_image": round(tk, 1), "dense_us_per_image": round(td, 1),
                              "kernel_MB": round(kb / 1e6, 1), "dense_MB": round(db / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
