"""Per-image cost of PixelGroupingModel's full-resolution work at BASELINE config-4 size: K = 4 score maps at 128 x 128 (R50 res3 + res4
features of a 1024^2 padded image), one elliptical object (~35 % of the image), G ground-truth part masks, output resized by the data
mapper to 1365 x 2048 and to 512 x 683.

Compares, on the same device in the same process,
  labels: pd_scores_argmax_resized_u8        vs  F.interpolate -> crop -> F.interpolate -> argmax -> where   (the route it replaces),
          (label map + label counts)             timed once as it stands and once followed by the `bincount` of the label map, which
                                                 the kernel's counts replace
  masks:  pd_masks_resize_u8 (G + 1 masks)   vs  F.interpolate(masks.float()) != 0
each as a batch of --batch images per call (the kernels are one launch per batch), device events around --iters calls after a warm-up.

  python tools/bench_pixel_grouping.py [--batch 4] [--gts 4] [--iters 50] [--out FILE]
prints one JSON line (microseconds per image)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--gts", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from partdistillation_amd.functions import pixel_grouping as G
    dev = "cuda"
    K, h, w, Hp, Wp = 4, 128, 128, 1024, 1024
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(0)
    scores = [F.interpolate(torch.randn((1, K, 8, 8), generator=g, device=dev), size=(h, w), mode="bicubic", align_corners=False)[0].contiguous()
              + 0.1 * torch.randn((K, h, w), generator=g, device=dev) for _ in range(B)]
    res = {"K": K, "low": [h, w], "padded": [Hp, Wp], "batch": B, "gts": args.gts, "device": torch.cuda.get_device_name(0), "cases": {}}
    for (Hi, Wi), (H, W) in (((683, 1024), (1365, 2048)), ((768, 1024), (512, 683))):
        ys, xs = torch.meshgrid(torch.arange(Hi, device=dev) / Hi, torch.arange(Wi, device=dev) / Wi, indexing="ij")
        obj = (((ys - 0.5) ** 2 / 0.13 + (xs - 0.5) ** 2 / 0.085) < 1.0)
        parts = torch.stack([obj & ((xs * args.gts).long() == k) for k in range(args.gts)])
        masks = torch.cat([obj[None], parts]).contiguous()                                 # the object mask and the G part masks, [G + 1, Hi, Wi]
        obj_out = G.masks_resize([(masks[:1], (Hi, Wi), (H, W))])[0][0][0]
        items = [(s, obj_out, (Hp, Wp), (Hi, Wi)) for s in scores]
        zero = torch.zeros((), dtype=torch.uint8, device=dev)

        def labels_kernel():
            return G.scores_argmax_resized(items)

        def labels_torch(counts=False):
            out = []
            for s in scores:
                up = F.interpolate(s[None], size=(Hp, Wp), mode="bilinear", align_corners=False)[:, :, :Hi, :Wi]
                up = F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0]
                lab = torch.where(obj_out, up.argmax(0).to(torch.uint8) + 1, zero)
                out.append((lab, torch.bincount(lab.flatten().long(), minlength=K + 1) if counts else None))
            return out

        def masks_kernel():
            return G.masks_resize([(masks, (Hi, Wi), (H, W))] * B)

        def masks_torch():
            return [F.interpolate(masks[None].float(), size=(H, W), mode="bilinear", align_corners=False)[0] != 0 for _ in range(B)]

        # same answers before timing them
        lk, lt = labels_kernel(), labels_torch(counts=True)
        diff = max(float((a != b[0]).float().mean()) for a, b in zip(lk[0], lt))
        assert diff < 1e-3, diff
        assert all(torch.equal(c[:K + 1].long(), torch.bincount(a.flatten().long(), minlength=K + 1)) for a, c in zip(lk[0], lk[1]))
        assert all(torch.equal(a[0], b) for a, b in zip(masks_kernel(), masks_torch()))
        t = {"labels_kernel_us": timed(labels_kernel, args.iters) / B, "labels_torch_us": timed(labels_torch, args.iters) / B,
             "labels_torch_with_bincount_us": timed(lambda: labels_torch(counts=True), args.iters) / B,
             "masks_kernel_us": timed(masks_kernel, args.iters) / B, "masks_torch_us": timed(masks_torch, args.iters) / B,
             "label_pixels_that_differ": diff, "object_share": float(obj_out.float().mean())}
        t["labels_speedup"] = t["labels_torch_us"] / t["labels_kernel_us"]
        t["labels_speedup_with_bincount"] = t["labels_torch_with_bincount_us"] / t["labels_kernel_us"]
        t["masks_speedup"] = t["masks_torch_us"] / t["masks_kernel_us"]
        res["cases"][f"{Hi}x{Wi}->{H}x{W}"] = {k: round(v, 4) for k, v in t.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
