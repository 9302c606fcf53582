"""Per-image cost of the device evaluators (partdistillation_amd/evaluation/, include/pd_eval.h) on synthetic 1024^2 images:
P = 200 proposals and G = 16 ground-truth masks made of overlapping ellipses.

Reports, per image: the time of each kernel (pack, intersections, greedy cover, confusion table) and of a whole
ProposalEvaluator.process / mIOU_Evaluator.process (device events around many images, after a warm-up); the algorithmic bytes
(the mask bytes read once plus the packed planes written and read back) and the share of the HBM peak they reach; and, for scale,
a numpy restatement of the reference's host path on the same masks (copy to the host, run-length encoding of every mask, dense IoUs,
label maps painted mask by mask and np.bincount), timed on this host.

  python tools/bench_evaluation.py [--size 1024] [--proposals 200] [--gts 16] [--iters 20] [--cpu-images 1] [--out FILE]
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E (spec)


def ellipses(n, H, W, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    ys = torch.arange(H, device=device, dtype=torch.float32)[None, :, None]
    xs = torch.arange(W, device=device, dtype=torch.float32)[None, None, :]
    c = torch.rand((n, 2), generator=g, device=device) * torch.tensor([H, W], device=device, dtype=torch.float32)
    r = (torch.rand((n, 2), generator=g, device=device) * 0.25 + 0.03) * torch.tensor([H, W], device=device, dtype=torch.float32)
    return ((ys - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((xs - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2 < 1


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                           # us per call


def reference_host_path(pred, scores, gt, pred_cls, gt_cls, n):
    """numpy restatement of the reference evaluators' host work for one image (for scale; pycocotools' C RLE code is not used)"""
    t = {}
    t0 = time.perf_counter()
    pm, gm = pred.cpu().numpy(), gt.cpu().numpy()
    t["copy_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rles = []
    for m in list(pm) + list(gm):
        f = np.asfortranarray(m).reshape(-1, order="F")
        edges = np.flatnonzero(np.diff(f.astype(np.int8))) + 1
        rles.append(np.diff(np.concatenate([[0], edges, [f.size]])))
    t["rle_encode_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    order = np.argsort(-scores.cpu().numpy(), kind="stable")[:200]
    a = pm.reshape(len(pm), -1)[order].astype(np.float32)
    b = gm.reshape(len(gm), -1).astype(np.float32)
    inter = (a @ b.T).astype(np.float64)
    union = a.sum(1)[:, None] + b.sum(1)[None, :] - inter
    _ = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
    t["iou_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pd = np.full(pm.shape[1:], n, dtype=np.int64)
    for m, c in zip(pm, pred_cls.cpu().numpy()):
        pd[np.where(m)] = c
    g = np.full(gm.shape[1:], n, dtype=np.int64)
    for m, c in zip(gm, gt_cls.cpu().numpy()):
        g[np.where(m)] = c
    np.bincount((n + 1) * pd.reshape(-1) + g.reshape(-1), minlength=(n + 1) ** 2)
    t["label_maps_bincount_ms"] = (time.perf_counter() - t0) * 1e3
    t["total_ms"] = sum(t.values())
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--proposals", type=int, default=200)
    ap.add_argument("--gts", type=int, default=16)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluation.py measures the device evaluators: it needs a GPU")
    from partdistillation_amd.compat import Instances
    from partdistillation_amd.evaluation import ProposalEvaluator, mIOU_Evaluator
    from partdistillation_amd.functions import eval_metrics as E
    dev, H = "cuda", args.size
    W, P, G, n = H, args.proposals, args.gts, args.classes
    pred, gt = ellipses(P, H, W, 1, dev).contiguous(), ellipses(G, H, W, 2, dev).contiguous()
    g = torch.Generator(device=dev).manual_seed(3)
    scores = torch.rand(P, generator=g, device=dev)
    pred_cls = torch.randint(0, n, (P,), generator=g, device=dev)
    gt_cls = torch.randint(0, n, (G,), generator=g, device=dev)
    slot = torch.tensor([5], device=dev)
    order = torch.sort(scores, descending=True, stable=True)[1][:E.MAX_ROWS].contiguous()
    hw, words = H * W, E.words_of(H * W)

    (pb, pa), (gb, ga) = E.pack_masks([pred, gt])
    inter = E.intersections([(pb, order, gb)])[0]
    thr = E.thresholds(dev)
    hits = torch.zeros((5, 10), dtype=torch.int64, device=dev)
    num_pos = torch.zeros(5, dtype=torch.int64, device=dev)
    conf = torch.zeros((16, n + 1, n + 1), dtype=torch.int64, device=dev)
    it = args.iters
    res = {"size": [H, W], "proposals": P, "gts": G, "classes": n}
    k = {}
    k["pack_us"] = timed(lambda: E.pack_masks([pred, gt]), it)
    k["intersect_us"] = timed(lambda: E.intersections([(pb, order, gb)]), it)
    k["recall_us"] = timed(lambda: E.recall_add([(inter, order, pa, ga)], thr, hits, num_pos), it)
    k["confusion_us"] = timed(lambda: E.confusion_add([(pb, pred_cls, gb, gt_cls, slot, hw)], n, conf), it)

    p, gi = Instances((H, W)), Instances((H, W))
    p.pred_masks, p.scores, p.pred_classes = pred, scores, pred_cls
    gi.gt_masks, gi.gt_classes = gt, gt_cls
    pe = ProposalEvaluator(distributed=False)
    me = mIOU_Evaluator([f"c{i}" for i in range(n)], n, distributed=False, num_object_classes=16)
    k["proposal_process_us"] = timed(lambda: pe.process(None, [{"proposals": p, "gt_masks": gi}]), it)
    k["miou_process_us"] = timed(lambda: me.process(None, [{"predictions": p, "gt_instances": gi, "gt_object_label": slot}]), it)
    res["device_us_per_image"] = {key: round(v, 1) for key, v in k.items()}

    mask_bytes = (P + G) * hw
    plane_bytes = (P + G) * words * 8
    algo = {"pack": mask_bytes + plane_bytes,                                            # masks read once, planes written
            "intersect": (min(P, E.MAX_ROWS) + G) * words * 8,                             # every plane word read once
            "confusion": (P + G) * words * 8,                                              # upper bound: every plane word
            "proposal_process": mask_bytes + plane_bytes + (min(P, E.MAX_ROWS) + G) * words * 8}
    res["algorithmic_bytes"] = algo
    res["hbm_peak_share"] = {key: round(algo[key] / (k[key + "_us"] * 1e-6) / HBM_PEAK, 3) for key in algo}

    cpu = [reference_host_path(pred, scores, gt, pred_cls, gt_cls, n) for _ in range(max(args.cpu_images, 0))]
    if cpu:
        res["reference_host_path_ms_per_image"] = {key: round(float(np.mean([c[key] for c in cpu])), 1) for key in cpu[0]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
