"""Generate tests/golden/eval.pt: the REAL reference evaluators (ProposalEvaluator, mIOU_Evaluator, mIOU_Matcher, imported from
the reference checkout through ref_shim.py) run on CPU over deterministic cases, plus the reference's evaluation-branch outputs already
stored in infer.pt / infer_pd.pt, and the reference PartDistillationModel's match -> evaluate protocol.

Run in the build container only:   python tests/golden/make_golden_eval.py
The inputs are stored with the results (masks bit-packed with numpy.packbits); the tests read only eval.pt."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import common as C  # noqa: E402
import ref_shim  # noqa: E402

META = {"thing_classes": ["a"]}


def install():
    ref_shim.install()
    ref_shim.install_inference_standins()
    comm = sys.modules["detectron2.utils.comm"]
    comm.all_gather = lambda x: [x]
    comm.gather = lambda x, dst=0: [x]
    comm.is_main_process = lambda: True
    comm.synchronize = lambda: None

    class DatasetEvaluator:
        pass

    class SemSegEvaluator(DatasetEvaluator):
        pass
    ref_shim._mod("detectron2.evaluation", DatasetEvaluator=DatasetEvaluator, SemSegEvaluator=SemSegEvaluator)
    ref_shim._mod("detectron2.evaluation.evaluator", DatasetEvaluator=DatasetEvaluator)
    ref_shim._mod("detectron2.evaluation.sem_seg_evaluation", SemSegEvaluator=SemSegEvaluator)
    ref_shim._mod("detectron2.utils.logger", create_small_table=lambda d: str(d))

    def get(name):
        ns = types.SimpleNamespace(thing_classes=list(META["thing_classes"]))
        if "part_classes" in META:
            ns.part_classes = list(META["part_classes"])
        return ns
    sys.modules["detectron2.data"].MetadataCatalog = types.SimpleNamespace(get=get)
    mods = {}
    for name in ("proposal_evaluator", "miou_evaluator", "miou_matcher"):
        spec = importlib.util.spec_from_file_location("pd_ref_" + name, f"{ref_shim.REF_ROOT}/part_distillation/evaluation/{name}.py")
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


def pack(m):
    m = torch.as_tensor(m).bool()
    return {"bits": torch.from_numpy(np.packbits(m.numpy().reshape(-1))), "shape": tuple(m.shape)}


def inst(**kw):
    return ref_shim._Instances(None, **kw)


# ----------------------------------------------------------------------------------------------------------------------- cases
def ellipses(n, H, W, g, scale=0.35):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    c = torch.rand((n, 2), generator=g, dtype=torch.float64) * torch.tensor([H, W])
    r = (torch.rand((n, 2), generator=g, dtype=torch.float64) * scale + 0.05) * torch.tensor([H, W])
    return ((ys[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((xs[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2 < 1


def random_masks(n, H, W, g, p=0.3):
    return torch.rand((n, H, W), generator=g) < p


def exact_iou_image():
    """IoUs of exactly 0.5, 0.75, 0.8, 0.6, 0.55, 0.85: the last four lie BELOW their float32 thresholds in float64 and reach them
    once rounded to float32 (the reference stores the recorded overlap in a float32 tensor)"""
    H, W = 10, 40
    gts, preds = [], []
    for k, (inter, union) in enumerate(((4, 8), (3, 4), (4, 5), (3, 5), (11, 20), (17, 20))):
        gt = torch.zeros(H, W, dtype=torch.bool)
        pr = torch.zeros(H, W, dtype=torch.bool)
        gt.view(-1)[k * 60:k * 60 + union] = True          # gt = union, pred = inter pixels of it
        pr.view(-1)[k * 60:k * 60 + inter] = True
        gts.append(gt)
        preds.append(pr)
    return torch.stack(preds), torch.stack(gts)


def tie_image(g):
    H, W = 24, 30
    base = ellipses(6, H, W, g)
    gts = torch.stack([base[0], base[0], base[1], base[2]])           # two identical gts
    preds = torch.stack([base[3], base[0], base[0], base[1] | base[4], base[5], base[2], base[2]])   # identical proposals
    return preds, gts


def proposal_cases():
    g = torch.Generator().manual_seed(7100)
    cases = {}

    def img(pred, gt, scores=None):
        if scores is None:
            scores = torch.randperm(max(pred.shape[0], 1), generator=g)[:pred.shape[0]].float() / max(pred.shape[0], 1) + 0.01
        return {"pred": pred, "scores": scores.float(), "gt": gt}
    cases["random"] = [img(random_masks(30, 37, 45, g), random_masks(5, 37, 45, g, 0.4)) for _ in range(3)]
    cases["ellipses"] = [img(ellipses(60, 64, 80, g), ellipses(8, 64, 80, g)) for _ in range(2)]
    cases["exact"] = [img(*exact_iou_image())]
    cases["ties"] = [img(*tie_image(g)), img(*tie_image(g))]
    cases["many"] = [img(ellipses(230, 33, 41, g, 0.3), ellipses(12, 33, 41, g)),
                     img(ellipses(201, 20, 20, g, 0.3), ellipses(3, 20, 20, g))]
    z = torch.zeros((2, 16, 20), dtype=torch.bool)
    gz = ellipses(4, 16, 20, g)
    gz[1] = False                                                                 # a gt of zero area
    cases["edge"] = [img(ellipses(0, 16, 20, g), ellipses(3, 16, 20, g)),        # no proposals: adds nothing
                     img(ellipses(5, 16, 20, g), ellipses(0, 16, 20, g)),        # no gt
                     img(ellipses(7, 16, 20, g), gz),
                     img(z[:1], ellipses(2, 16, 20, g)),                          # the all-zero placeholder proposal
                     img(ellipses(1, 16, 20, g), gz[1:2])]                       # only a zero-area gt: num_pos += 0
    return cases


def miou_cases():
    g = torch.Generator().manual_seed(7200)
    cases = {}

    def images(n_img, H, W, pred_n, gt_classes, objects, n_pred=(3, 7), n_gt=(2, 6)):
        out = []
        for i in range(n_img):
            P = int(torch.randint(n_pred[0], n_pred[1] + 1, (1,), generator=g))
            G = int(torch.randint(n_gt[0], n_gt[1] + 1, (1,), generator=g))
            pm = ellipses(P, H, W, g, 0.45)
            gm = ellipses(G, H, W, g, 0.45)
            pc = torch.randint(0, pred_n, (P,), generator=g)
            gc = torch.tensor(gt_classes)[torch.randint(0, len(gt_classes), (G,), generator=g)]
            out.append({"pred": pm, "pred_classes": pc, "gt": gm, "gt_classes": gc, "object": int(objects[i % len(objects)])})
        return out
    # 6 gt part classes (part_classes), 5 thing_classes names, classes 3 and 5 never in the ground truth
    cases["basic"] = {"thing_classes": [f"t{i}" for i in range(5)], "part_classes": [f"p{i}" for i in range(6)], "pred_n": 6,
                      "images": images(7, 29, 35, 6, [0, 1, 2, 4], [3, 7, 12])}
    cases["matcher_wide"] = {"thing_classes": [f"t{i}" for i in range(4)], "pred_n": 9,
                             "images": images(5, 40, 33, 9, [0, 1, 2, 3], [0, 5])}
    cases["one_object"] = {"thing_classes": [f"t{i}" for i in range(3)], "pred_n": 3,
                           "images": images(3, 17, 23, 3, [0, 1, 2], [2], n_pred=(1, 3), n_gt=(1, 2))}
    return cases


# ----------------------------------------------------------------------------------------------------------------------- runners
def run_proposal(M, imgs):
    ev = M["proposal_evaluator"].ProposalEvaluator(distributed=True)
    ev.reset()
    for im in imgs:
        pm = im["pred"]
        if pm.shape[0] == 0:              # torch.split of an empty tensor yields one empty piece, which the reference cannot index
            pm = types.SimpleNamespace(split=lambda n: [])
        ev.process(None, [{"proposals": inst(pred_masks=pm, scores=im["scores"]), "gt_masks": inst(gt_masks=im["gt"])}])
    return ev.evaluate()


def run_miou(M, case, which):
    META.clear()
    META["thing_classes"] = case["thing_classes"]
    if "part_classes" in case:
        META["part_classes"] = case["part_classes"]
    if which == "eval":
        ev = M["miou_evaluator"].mIOU_Evaluator("d", distributed=True)
    else:
        ev = M["miou_matcher"].mIOU_Matcher("d", num_classes=case["pred_n"], distributed=True)
    ev.reset()
    for im in case["images"]:
        ev.process(None, [{"predictions": inst(pred_masks=im["pred"], pred_classes=im["pred_classes"]),
                           "gt_instances": inst(gt_masks=im["gt"], gt_classes=im["gt_classes"]),
                           "gt_object_label": torch.tensor([im["object"]])}])
    res = ev.evaluate()
    return {int(k): v.tolist() for k, v in res.items()} if which == "match" else {k: float(v) for k, v in res.items()}


def pd_chain(M):
    """reference PartDistillationModel: mode "match" -> mIOU_Matcher -> update_majority_vote_mapping -> mode "eval" -> mIOU_Evaluator
    on the INFER inputs (the setup of make_golden.gen_infer_pd)"""
    PDM = importlib.import_module("part_distillation.part_distillation_model")
    cfg = C.INFER
    outputs, inputs = C.make_infer_inputs(cfg)
    K = C.INFER_PD_CLASSES
    outputs = dict(outputs, pred_logits=C.seeded((len(inputs), cfg["Q"], K + 1), 5300) * 2)
    model = object.__new__(PDM.PartDistillationModel)
    torch.nn.Module.__init__(model)
    model.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    model.test_topk_per_image, model.wandb_vis_topk = cfg["topk"] * 2, cfg["topk"] * 2
    model.num_classes, model.num_queries, model.fg_score_threshold = K, cfg["Q"], 0.1
    model.min_pseudo_mask_ratio, model.apply_masking_with_object_mask = 0.02, True
    model.use_unique_per_pixel_label, model.min_pseudo_mask_score, model.use_oracle_classifier = True, -1.0, False
    model.majority_vote_mapping = {}
    ns = types.SimpleNamespace
    batched = [{"image": i["image"], "height": i["height"], "width": i["width"],
                "part_instances": ns(to=lambda d, _i=i: ns(gt_masks=ns(tensor=_i["part_masks"]), gt_classes=_i["part_labels"])),
                "instances": ns(to=lambda d, _i=i, _b=b: ns(gt_masks=ns(tensor=_i["object_mask"]), gt_classes=torch.tensor([3 + _b])))}
               for b, i in enumerate(inputs)]
    images = ref_shim._ImageList.from_tensors([i["image"] for i in inputs], cfg["size_div"])
    model.eval()
    META.clear()
    META.update(thing_classes=[f"part{i}" for i in range(K)])

    def run(ev):
        ev.reset()
        targets = model._prepare_gt_targets(batched, images)
        ev.process(batched, model.inference(batched, targets, images, outputs, vis=False))
        return ev.evaluate()
    model.mode = "match"
    mapping = run(M["miou_matcher"].mIOU_Matcher("d", num_classes=K, distributed=True))
    model.majority_vote_mapping = {int(k): v for k, v in mapping.items()}
    model.mode = "eval"
    res = run(M["miou_evaluator"].mIOU_Evaluator("d", distributed=True))
    return {int(k): v.tolist() for k, v in mapping.items()}, {k: float(v) for k, v in res.items()}


def main():
    M = install()
    out = {"proposal": {}, "miou": {}}
    for name, imgs in proposal_cases().items():
        out["proposal"][name] = {"images": [{"pred": pack(i["pred"]), "scores": i["scores"], "gt": pack(i["gt"])} for i in imgs],
                                 "result": run_proposal(M, imgs)}
    for name, case in miou_cases().items():
        rec = {k: v for k, v in case.items() if k != "images"}
        rec["images"] = [{"pred": pack(i["pred"]), "pred_classes": i["pred_classes"], "gt": pack(i["gt"]), "gt_classes": i["gt_classes"],
                          "object": i["object"]} for i in case["images"]]
        rec["match"] = run_miou(M, case, "match")
        if case["pred_n"] <= len(case.get("part_classes", case["thing_classes"])):
            rec["eval"] = run_miou(M, case, "eval")
        out["miou"][name] = rec
    # the reference's own evaluation-branch outputs (infer.pt / infer_pd.pt) through its evaluators
    infer, infer_pd = (torch.load(os.path.join(HERE, f), weights_only=False) for f in ("infer.pt", "infer_pd.pt"))
    out["infer"] = {tag: run_proposal(M, [{"pred": r["pred_masks"], "scores": r["scores"], "gt": r["gt_masks"]} for r in infer[tag]])
                    for tag in ("unique_1", "unique_0")}
    K = C.INFER_PD_CLASSES
    out["infer_pd"] = {}
    for tag in ("eval_1", "eval_0"):
        case = {"thing_classes": [f"part{i}" for i in range(K)], "pred_n": K,
                "images": [{"pred": r["pred_masks"], "pred_classes": r["pred_classes"], "gt": g["gt_masks"], "gt_classes": g["gt_classes"],
                            "object": int(r["gt_object_label"].reshape(-1)[0])} for r, g in zip(infer_pd[tag], infer["unique_1"])]}
        out["infer_pd"][tag] = run_miou(M, case, "eval")
    mapping, res = pd_chain(M)
    out["pd_chain"] = {"mapping": mapping, "eval": res}
    path = os.path.join(HERE, "eval.pt")
    torch.save(out, path)
    print(f"wrote eval.pt  {os.path.getsize(path) / 1024:.1f} KiB")
    for k in ("infer", "infer_pd", "pd_chain"):
        print(k, out[k])


if __name__ == "__main__":
    main()
