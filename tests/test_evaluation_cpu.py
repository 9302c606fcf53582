"""Host half of the device evaluators (partdistillation_amd/evaluation/metrics.py) against the REAL reference evaluators
(tests/golden/eval.pt, made by make_golden_eval.py): the count tables of every golden case, restated in numpy (eval_oracle.py), fed to
the AR / mIoU / majority-vote code must give the reference's result dicts; the tables merge over two gloo ranks with one all_reduce."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval.pt")
PROPOSAL_CASES = ["random", "ellipses", "exact", "ties", "many", "edge"]
MIOU_CASES = ["basic", "matcher_wide", "one_object"]


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLDEN, weights_only=False)


@pytest.mark.parametrize("name", PROPOSAL_CASES)
def test_proposal_metrics_from_counts_equal_reference(gold, name):
    from partdistillation_amd.evaluation.metrics import proposal_metrics
    case = gold["proposal"][name]
    hits, num_pos = O.recall_counts(O.proposal_images(case))
    O.assert_same_dict({"box_proposals": proposal_metrics(hits, num_pos, len(case["images"]))}, dict(case["result"]))


def test_exact_iou_case_counts_float32_rounding(gold):
    """IoU 0.8 / 0.6 / 0.55 / 0.85 lie below their float32 thresholds in float64; the reference rounds the recorded value to float32 first"""
    hits, num_pos = O.recall_counts(O.proposal_images(gold["proposal"]["exact"]))
    thr = O.thresholds()
    ious = np.array([0.5, 0.75, 0.8, 0.6, 0.55, 0.85])
    assert num_pos[-1] == 6
    assert list(hits[-1]) == [int((ious.astype(np.float32) >= t).sum()) for t in thr]
    assert list(hits[-1]) != [int((ious >= float(t)).sum()) for t in thr]


@pytest.mark.parametrize("tag", ["unique_1", "unique_0"])
def test_proposal_metrics_on_reference_inference_outputs(gold, tag):
    infer = torch.load(os.path.join(ROOT, "tests", "golden", "infer.pt"), weights_only=False)[tag]
    from partdistillation_amd.evaluation.metrics import proposal_metrics
    hits, num_pos = O.recall_counts([(r["pred_masks"], r["scores"], r["gt_masks"]) for r in infer])
    O.assert_same_dict({"box_proposals": proposal_metrics(hits, num_pos, len(infer))}, dict(gold["infer"][tag]))


@pytest.mark.parametrize("name", MIOU_CASES)
def test_miou_and_majority_vote_from_counts_equal_reference(gold, name):
    from partdistillation_amd.evaluation.metrics import majority_voting, miou_metrics, seen_slots
    case = gold["miou"][name]
    gt_n, pred_n = O.gt_num_classes(case), case["pred_n"]
    imgs = O.miou_images(case)
    n = max(gt_n, pred_n)
    conf = O.confusion(imgs, n, 16)
    got = {k: majority_voting(conf[k], pred_n, gt_n).tolist() for k in seen_slots(conf)}
    assert got == case["match"]
    if "eval" in case:
        conf = O.confusion(imgs, gt_n, 16)
        O.assert_same_dict(miou_metrics(conf, case["thing_classes"], gt_n), case["eval"], rel=1e-12)


@pytest.mark.parametrize("tag", ["eval_1", "eval_0"])
def test_miou_on_reference_inference_outputs(gold, tag):
    import common as C
    from partdistillation_amd.evaluation.metrics import miou_metrics
    g = os.path.join(ROOT, "tests", "golden")
    pd = torch.load(os.path.join(g, "infer_pd.pt"), weights_only=False)[tag]
    gt = torch.load(os.path.join(g, "infer.pt"), weights_only=False)["unique_1"]
    K = C.INFER_PD_CLASSES
    conf = O.confusion([(r["pred_masks"], r["pred_classes"], t["gt_masks"], t["gt_classes"], int(r["gt_object_label"].reshape(-1)[0]))
                        for r, t in zip(pd, gt)], K, 8)
    O.assert_same_dict(miou_metrics(conf, [f"part{i}" for i in range(K)], K), gold["infer_pd"][tag], rel=1e-12)


def test_inference_on_dataset_loop_contract():
    from partdistillation_amd.evaluation import inference_on_dataset

    class Model(torch.nn.Module):
        def forward(self, x):
            assert not self.training and not torch.is_grad_enabled()
            return [v * 2 for v in x]

    class Ev:
        def reset(self):
            self.seen = []

        def process(self, inputs, outputs):
            self.seen.append((inputs, outputs))

        def evaluate(self):
            return {"n": len(self.seen)}
    m, ev = Model().train(), Ev()
    assert inference_on_dataset(m, [[1, 2], [3]], ev) == {"n": 2}
    assert m.training and ev.seen[1] == ([3], [6])
    assert inference_on_dataset(m.eval(), [[1]], None) == {} and not m.training


# ----------------------------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merge_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import eval_oracle as Ow
    from partdistillation_amd.evaluation import ProposalEvaluator, mIOU_Evaluator, mIOU_Matcher
    gold = torch.load(GOLDEN, weights_only=False)
    out = {}
    # proposal counters: every rank counts its share of the images (the device counters, held on the host here)
    imgs = Ow.proposal_images(gold["proposal"]["ellipses"]) + Ow.proposal_images(gold["proposal"]["ties"])
    mine = imgs[rank::world]
    hits, num_pos = Ow.recall_counts(mine)
    ev = ProposalEvaluator(distributed=True)
    ev._counts = torch.cat([torch.from_numpy(hits).reshape(-1), torch.from_numpy(num_pos), torch.tensor([len(mine)])])
    out["proposal"] = ev.evaluate()
    # confusion tables
    mc = gold["miou"]["basic"]
    gt_n = Ow.gt_num_classes(mc)
    mimgs = Ow.miou_images(mc)[rank::world]
    me = mIOU_Evaluator(mc["thing_classes"], gt_n, distributed=True, num_object_classes=16)
    me._conf = torch.from_numpy(Ow.confusion(mimgs, gt_n, 16))
    out["miou"] = me.evaluate()
    mm = mIOU_Matcher(mc["thing_classes"], gt_n, num_classes=mc["pred_n"], distributed=True, num_object_classes=16)
    mm._conf = torch.from_numpy(Ow.confusion(mimgs, max(gt_n, mc["pred_n"]), 16))
    out["match"] = {k: v.tolist() for k, v in mm.evaluate().items()}
    torch.save(out, os.path.join(tmp, f"merge{rank}.pt"))
    dist.destroy_process_group()


def test_count_tables_merge_over_two_gloo_ranks(gold, tmp_path):
    from partdistillation_amd.evaluation.metrics import proposal_metrics
    world = 2
    mp.spawn(_merge_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"merge{k}.pt", weights_only=False) for k in range(world)]
    imgs = O.proposal_images(gold["proposal"]["ellipses"]) + O.proposal_images(gold["proposal"]["ties"])
    hits, num_pos = O.recall_counts(imgs)
    O.assert_same_dict(r[0]["proposal"], {"box_proposals": proposal_metrics(hits, num_pos, len(imgs))})
    assert r[1]["proposal"] == {}                                        # only rank 0 reports, like the reference
    mc = gold["miou"]["basic"]
    O.assert_same_dict(r[0]["miou"], mc["eval"], rel=1e-12)
    O.assert_same_dict(r[1]["miou"], r[0]["miou"])
    assert r[0]["match"] == r[1]["match"] == mc["match"]
