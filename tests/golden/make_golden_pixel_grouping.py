"""Generate tests/golden/pixel_grouping.pt: the REAL reference PixelGroupingModel (imported from the reference checkout through
ref_shim.py) with a stub backbone that returns the seeded features and sklearn KMeans(random_state=0), run on CPU over the images of
pixel_grouping_inputs.py, and the REAL reference ProposalEvaluator over its outputs.

Run in the build container only:   python tests/golden/make_golden_pixel_grouping.py
Stored per configuration and image: the sklearn centroids, pred_masks, gt_masks and the resized object mask (masks bit-packed with
numpy.packbits, as in make_golden_eval.py), and the evaluator's result over the set.

The reference does not raise on the image without an object (it returns no proposals), so that case is kept.

Three properties are asserted here so that the GPU tests can be strict:
 (a) the tap indices and the `l1 == 0` pattern of every mask-resize axis used are the same in plain fp32 and with the source index
     rounded once from its exact value (a fused multiply-add): the boolean resize cannot depend on how a compiler contracts it;
 (b) fewer than 1e-3 of the object's pixels have a reference top-2 score gap below 1e-4 (half the model test's 2e-3 allowance);
 (c) every reference IoU of a proposal with a ground-truth mask is at least 0.01 away from each threshold 0.50 : 0.05 : 0.95, so a few
     near-tie pixels cannot move a recall and the end-to-end AR can be compared exactly."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_eval as E  # noqa: E402
import pixel_grouping_inputs as PG  # noqa: E402
import ref_shim  # noqa: E402


def assert_sizes_insensitive(cfg):
    for H, W, oh, ow, _ in cfg["images"]:
        for n_in, n_out in ((H, oh), (W, ow)):
            a, b = PG.axis_taps(n_in, n_out, False), PG.axis_taps(n_in, n_out, True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"mask-resize axis {n_in} -> {n_out} is sensitive to rounding: pick another size"


def as_ref_inputs(inputs):
    ns = types.SimpleNamespace
    return [{"image": i["image"], "height": i["height"], "width": i["width"],
             # float 0 / 1 masks: the reference resizes them bilinearly
             "part_instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["part_masks"].float()), gt_classes=_i["part_labels"])),
             "instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["object_mask"].float()), gt_classes=torch.tensor([7])))}
            for i in inputs]


def main():
    cfg = PG.PIXGROUP
    assert_sizes_insensitive(cfg)
    mods = E.install()
    M = importlib.import_module("part_distillation.pixel_grouping_model")
    from sklearn.cluster import KMeans
    feats, inputs = PG.make_pixel_grouping_inputs(cfg)
    model = object.__new__(M.PixelGroupingModel)
    torch.nn.Module.__init__(model)
    model.backbone = lambda x: feats
    model.size_divisibility = cfg["size_div"]
    model.register_buffer("pixel_mean", torch.tensor(PG.PIXEL_MEAN).view(-1, 1, 1), False)
    model.register_buffer("pixel_std", torch.tensor(PG.PIXEL_STD).view(-1, 1, 1), False)
    model.num_test_iterations, model.wandb_vis_period = 0, 100
    model.wandb_visualize = lambda *a, **k: None
    model.backbone_feature_key_list = ["res3", "res4"]
    model.num_superpixel_clusters = cfg["K"]
    model.eval()
    thresholds = np.arange(0.5, 0.95 + 1e-5, 0.05)
    out = {}
    for tag, metric, norm in PG.CONFIGS:
        model.distance_metric, model.feature_normalize = metric, norm
        model.kmeans_module = KMeans(n_clusters=cfg["K"], random_state=0)
        captured, gaps = [], []
        orig_gen, orig_dist = M.PixelGroupingModel.generate_part_segments, M.PixelGroupingModel.measure_distance

        def dist(self, A, B, _orig=orig_dist):
            d = _orig(self, A, B)
            if d.shape[1] >= 2 and d.shape[0]:
                top2 = d.topk(2, dim=1)[0]
                gaps.append(top2[:, 0] - top2[:, 1])
            return d

        def gen(self, inp, f, fr, om, omr, _orig=orig_gen):
            r = _orig(self, inp, f, fr, om, omr)
            captured.append({"centroids": self.get_pixel_grouping(f, om).float(), "object_mask_resized": E.pack(omr), "n_points": int(om.sum())})
            return r
        model.measure_distance = types.MethodType(dist, model)
        model.generate_part_segments = types.MethodType(gen, model)
        results = model.forward(as_ref_inputs(inputs))
        assert len(results) == len(captured) == len(inputs)
        g = torch.cat(gaps)
        near = float((g < 1e-4).float().mean())
        assert near < 1e-3, f"{tag}: {near:.2e} of the object's pixels are near-ties"                                     # (b)
        imgs = []
        for cap, r, (_, _, _, _, kind) in zip(captured, results, cfg["images"]):
            pm, gm = r["proposals"].pred_masks, r["gt_masks"].gt_masks
            assert pm.dtype == gm.dtype == torch.bool and bool(r["proposals"].scores.all()) and r["proposals"].scores.shape[0] == pm.shape[0]
            assert (kind == "ellipse") == (cap["n_points"] > cfg["K"]) and (kind == "empty") == (cap["n_points"] == 0)
            assert pm.shape[0] == {"ellipse": pm.shape[0], "tiny": 1, "empty": 0}[kind]
            if pm.shape[0] and gm.shape[0]:
                a, b = pm.flatten(1).double(), gm.flatten(1).double()
                inter = a @ b.t()
                iou = (inter / (a.sum(1)[:, None] + b.sum(1)[None] - inter).clamp_min(1)).numpy()
                clear = np.abs(iou[..., None] - thresholds).min()
                assert clear >= 0.01, f"{tag}: an IoU lies {clear:.4f} from a threshold"                                  # (c)
            cap.update(pred_masks=E.pack(pm), gt_masks=E.pack(gm))
            imgs.append({"pred": pm, "scores": r["proposals"].scores, "gt": gm})
        out[tag] = {"images": captured, "result": E.run_proposal(mods, imgs), "near_tie_share": near}
        print(tag, "P =", [tuple(c["pred_masks"]["shape"]) for c in captured], "near ties", near, out[tag]["result"])
    path = os.path.join(HERE, "pixel_grouping.pt")
    torch.save(out, path)
    print(f"wrote pixel_grouping.pt  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
