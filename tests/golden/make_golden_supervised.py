"""Generate tests/golden/supervised.pt: the REAL reference SupervisedModel (imported from the reference checkout through ref_shim.py)
and the REAL reference Supervised_mIOU_Evaluator, run on CPU.

Run in the build container only:   python tests/golden/make_golden_supervised.py
Stored (tensors only, masks bit-packed with numpy.packbits as in make_golden_eval.py):
  eval[tag][image]   the evaluation branch (supervised_model.py:201-451) on the stubbed decoder outputs of supervised_inputs.py, for
                     class-agnostic / classification x per-pixel-unique / plain thresholding: pred_masks, scores, pred_classes,
                     gt_masks, gt_classes, the best IoU of every candidate mask;
  evaluator[tag]     the reference evaluator over those outputs: its confusion matrix, measure_mIOU's dict and evaluate()'s result;
  train[name]        the train branch through the model's own __init__ around the real head / criterion and the stub backbone of
                     common.py (as make_golden.gen_meta): state_dict keys, prepared targets, weighted losses (class-agnostic, 8 classes).

Three properties are asserted here so that the GPU tests can be strict:
 (a) the tap indices and the `l1 == 0` pattern of every mask-resize axis used are the same in plain fp32 and with the source index
     rounded once (a fused multiply-add): the boolean resize cannot depend on how a compiler contracts it;
 (b) fewer than 1e-3 of the pixels have a reference top-2 gap of score * sigmoid below 1e-4 (half the model test's 2e-3 allowance);
 (c) every reference best IoU is at least 0.01 away from the 0.001 foreground threshold.  (The `nomatch` image is exempt: its parts and
     its object are disjoint, so every IoU is exactly 0 whichever pixels a near-tie moves; that is asserted instead.)
A seed of supervised_inputs.py that violates one of these is replaced by another; among the seeds that pass, 8128 has the largest
smallest predicted class area (the evaluator test divides its pixel allowance by the smallest class areas)."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import common as C  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_eval as E  # noqa: E402
import pixel_grouping_inputs as PG  # noqa: E402
import ref_shim  # noqa: E402
import supervised_inputs as S  # noqa: E402

ns = types.SimpleNamespace


def assert_sizes_insensitive(cfg):
    for H, W, oh, ow, _ in cfg["images"]:
        for n_in, n_out in ((H, oh), (W, ow)):
            a, b = PG.axis_taps(n_in, n_out, False), PG.axis_taps(n_in, n_out, True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"mask-resize axis {n_in} -> {n_out} is sensitive to rounding: pick another size"


def as_ref_inputs(inputs):
    return [{"image": i["image"], "height": i["height"], "width": i["width"],
             "part_instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["part_masks"]), gt_classes=_i["part_labels"])),
             "instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["object_mask"])))} for i in inputs]


def near_tie_share(model, M, outputs, inputs, images, agnostic):
    """(b): share of output pixels whose top-2 gap of score * sigmoid(masked logit) is below 1e-4, on the reference's own dense maps"""
    near, total = 0, 0
    dense_all = F.interpolate(outputs["pred_masks"], size=tuple(images.tensor.shape[-2:]), mode="bilinear", align_corners=False)
    for cls, dense, inp, size in zip(outputs["pred_logits"], dense_all, inputs, images.image_sizes):
        dense = ref_shim.sem_seg_postprocess(dense, size, inp["height"], inp["width"])
        obj = ref_shim.sem_seg_postprocess(inp["object_mask"].float(), size, inp["height"], inp["width"]).bool()
        scores = cls.softmax(-1)[:, :-1]
        if agnostic:
            scores, idx = scores.flatten().topk(model.test_topk_per_image, sorted=False)
        else:
            scores, idx = scores.flatten(0, 1).topk(model.test_topk_per_image, sorted=False)
            idx = torch.div(idx, model.num_classes, rounding_mode="floor")
        top2 = (scores[:, None, None] * (dense[idx] * obj.sum(0, keepdim=True).bool()).sigmoid()).topk(2, dim=0)[0]
        near += int(((top2[0] - top2[1]) < 1e-4).sum())
        total += top2[0].numel()
    return near / total


def gen_eval(M, EV):
    cfg = S.SUP
    assert_sizes_insensitive(cfg)                                                                                            # (a)
    outputs, inputs = S.make_supervised_inputs(cfg)
    model = object.__new__(M.SupervisedModel)
    torch.nn.Module.__init__(model)
    model.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    model.num_queries, model.apply_masking_with_object_mask, model.class_agnostic_inference = cfg["Q"], True, False
    model.eval()
    batched = as_ref_inputs(inputs)
    images = ref_shim._ImageList.from_tensors([i["image"] for i in inputs], cfg["size_div"])
    out, evaluator = {}, {}
    for tag, (agnostic, unique) in S.CONFIGS.items():
        kind = "agnostic" if agnostic else "classes"
        model.class_agnostic_learning, model.use_unique_per_pixel_label = agnostic, unique
        model.num_classes = 1 if agnostic else cfg["num_classes"]
        model.test_topk_per_image = model.wandb_vis_topk = cfg["topk"][kind]
        ious = []
        orig = M.get_iou_all_cocoapi

        def iou(a, b, _orig=orig):
            r = _orig(a, b)
            ious.append(r.topk(1, dim=1)[0].flatten().double())
            return r
        M.get_iou_all_cocoapi = iou
        targets = model.prepare_targets(batched, images)
        res = model.inference(batched, targets, images, outputs[kind], vis=False)
        M.get_iou_all_cocoapi = orig
        assert len(ious) == len(res) == len(inputs)
        share = near_tie_share(model, M, outputs[kind], inputs, images, agnostic)
        if unique:
            assert share < 1e-3, f"{tag}: {share:.2e} of the pixels are near-ties"                                            # (b)
        recs = []
        for r, best, (_, _, _, _, k) in zip(res, ious, cfg["images"]):
            assert r["predictions"] is r["proposals"] and r["gt_instances"] is r["gt_masks"]
            assert float((best - 0.001).abs().min()) >= 0.01 or k == "nomatch", f"{tag}: a best IoU lies near the foreground threshold"   # (c)
            if k == "nomatch":
                assert float(best.max()) == 0.0 and r["predictions"].pred_masks.shape[0] == 1 and not bool(r["predictions"].pred_masks.any())
            p, g = r["predictions"], r["gt_instances"]
            recs.append({"pred_masks": E.pack(p.pred_masks), "scores": p.scores, "pred_classes": p.pred_classes, "gt_masks": E.pack(g.gt_masks),
                         "gt_classes": g.gt_classes, "best_ious": best})
        out[tag] = {"images": recs, "near_tie_share": share}
        E.META.clear()
        E.META["thing_classes"] = [f"part{i}" for i in range(cfg["num_classes"])]
        ev = EV.Supervised_mIOU_Evaluator("d", num_classes=cfg["num_classes"], distributed=True)
        ev.reset()
        ev.process(None, res)
        result = ev.evaluate()
        with np.errstate(invalid="ignore", divide="ignore"):
            table = ev.measure_mIOU(ev._conf_matrix)
        evaluator[tag] = {"conf": torch.from_numpy(ev._conf_matrix.copy()), "measure": {k: float(v) for k, v in table.items()},
                          "result": {k: float(v) for k, v in result.items()}}
        print(tag, "P =", [r["pred_masks"]["shape"][0] for r in recs], "near ties", share, evaluator[tag]["result"])
    return out, evaluator


def gen_train(M):
    """as make_golden.gen_meta: the model through its own __init__ on the ragged META batch (part_instances = the parts, instances =
    their union)"""
    class Meta(dict):                                       # MetadataCatalog.get(name): the constructor asks for .get("part_classes")
        __getattr__ = dict.get
    M.MetadataCatalog = ns(get=lambda name: Meta(thing_classes=["a"]))
    inputs = C.make_meta_inputs(C.META)
    bw = C.stub_backbone_weights(C.META)
    out = {}
    for name, agnostic, nc in (("agnostic", True, 1), ("classes", False, 8)):
        cfg = dict(C.META, num_classes=nc)
        shapes = {f"res{i + 2}": MG.L.ShapeSpec(channels=c, stride=s) for i, (c, s) in enumerate(zip(cfg["channels"], (4, 8, 16, 32)))}
        head = MG.L.head.MaskFormerHead(shapes, num_classes=nc, pixel_decoder=MG.build_pixel_decoder(cfg), transformer_predictor=MG.build_decoder(cfg),
                                        transformer_in_feature="multi_scale_pixel_decoder")
        table = MG.load_seeded(head, 111)
        model = M.SupervisedModel(backbone=lambda x: C.stub_backbone(x, bw), sem_seg_head=head, criterion=MG.build_criterion(cfg),
                                  num_queries=cfg["queries"], num_classes=nc, size_divisibility=32, pixel_mean=S.PIXEL_MEAN, pixel_std=S.PIXEL_STD,
                                  test_topk_per_image=10, dataset_name="none", use_wandb=False, class_agnostic_learning=agnostic)
        model.train()
        batched = [{"image": i["image"], "height": i["height"], "width": i["width"],
                    "part_instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["masks"]), gt_classes=_i["gt_classes"])),
                    "instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["masks"].any(0, keepdim=True))))} for i in inputs]
        captured = {}
        orig = model.prepare_targets

        def prep(inp, images, _orig=orig):
            t = _orig(inp, images)
            captured["targets"] = t
            return t
        model.prepare_targets = prep
        with MG.patched_rand(9300) as rr:
            losses = model(batched)
            ncalls = rr.calls
        out[name] = {"table": table, "state_dict_keys": sorted(model.state_dict().keys()), "rand_calls": torch.tensor(ncalls),
                     "losses": {k: v.detach().double() for k, v in losses.items()}, "total": sum(losses.values()).detach().double(),
                     "labels": [t["labels"] for t in captured["targets"]]}
        print("train", name, "total", float(out[name]["total"]))
    return out


def main():
    E.install()
    M = importlib.import_module("part_distillation.supervised_model")
    spec = importlib.util.spec_from_file_location("pd_ref_supervised_miou_evaluator",
                                                  f"{ref_shim.REF_ROOT}/part_distillation/evaluation/supervised_miou_evaluator.py")
    EV = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(EV)
    ev, evaluator = gen_eval(M, EV)
    out = {"eval": ev, "evaluator": evaluator, "train": gen_train(M)}
    path = os.path.join(HERE, "supervised.pt")
    torch.save(out, path)
    print(f"wrote supervised.pt  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
