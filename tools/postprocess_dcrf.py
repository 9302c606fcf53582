"""Dense-CRF clean-up of the files a proposal-generation run wrote, with the reference's command line
(continuously_postprocess_dcrf.py):

  python tools/postprocess_dcrf.py --dataset_name imagenet_1k_train --res res3_res4 --dist_metric dot --num_k 4 \
      [--parallel_job_id J --num_parallel_jobs N] [--once] [--debug]

reads   pseudo_labels/proposal_generation/<dataset>/detic_based/generated_proposals/<res>/<dist_metric>_<num_k>/<class code>/<file>
writes  pseudo_labels/proposal_generation/<dataset>/detic_based/generated_proposals_processed/<res>/<dist_metric>_<num_k>/<class code>/<file>
Job J of N (1-based) takes the J-th block of len(classes) // N class directories, the last job also the remainder.  Files that already
exist in the target are skipped.  Like the reference it keeps polling the source for new files; --once ends after one sweep."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from partdistillation_amd.postprocess_dcrf import refine_proposals  # noqa: E402

PATH_ROOT = "pseudo_labels/proposal_generation/"


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="Postprocess pseudo-labels")
    ap.add_argument("--parallel_job_id", type=int, default=-1)
    ap.add_argument("--num_parallel_jobs", type=int, default=-1)
    ap.add_argument("--dataset_name", type=str, default="imagenet_1k_train")
    ap.add_argument("--dist_metric", type=str, default="dot")
    ap.add_argument("--res", type=str, default="res3_res4")
    ap.add_argument("--num_k", type=int, default=4)
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--once", action="store_true", help="end after one sweep over the source instead of polling forever")
    ap.add_argument("--path_root", type=str, default=PATH_ROOT)
    return ap.parse_args(argv)


def job_classes(code_list, job_id, num_jobs):
    """the reference's split: equal blocks of len // num_jobs classes, the last job takes what is left"""
    if num_jobs <= 0:
        return code_list
    per_job = len(code_list) // num_jobs
    end = len(code_list) if job_id == num_jobs else per_job * job_id
    return code_list[per_job * (job_id - 1):end]


def read_image(data):
    from PIL import Image
    path = data.get("file_path") or data["file_name"]
    return np.asarray(Image.open(path).convert("RGB"))


def main(argv=None):
    args = get_args(argv)
    tail = os.path.join(args.dataset_name, "detic_based", "{}", args.res, "{}_{}".format(args.dist_metric, args.num_k))
    source_root = os.path.join(args.path_root, tail.format("generated_proposals"))
    target_root = os.path.join(args.path_root, tail.format("generated_proposals_processed"))
    code_list = job_classes(os.listdir(source_root), args.parallel_job_id, args.num_parallel_jobs)
    for code in code_list:
        os.makedirs(os.path.join(target_root, code), exist_ok=True)
    num_total = sum(len(os.listdir(os.path.join(source_root, code))) for code in code_list)
    t0, done = time.time(), 0
    while True:
        for code in code_list:
            for fname in os.listdir(os.path.join(source_root, code)):
                target = os.path.join(target_root, code, fname)
                if os.path.exists(target):
                    continue
                data = torch.load(os.path.join(source_root, code, fname), "cpu", weights_only=False)
                masks = data.get("part_masks", data.get("part_mask"))
                if masks is not None and len(masks):
                    data = refine_proposals(data, read_image(data))
                if args.debug:
                    raise SystemExit("debug. ")
                torch.save(data, target)
                done += 1
                if done % 1000 == 1:
                    print("{} ({:.2f} %) images processed on process {} ({:.2f} s / image)".format(
                        done, done / max(num_total, 1) * 100, args.parallel_job_id, (time.time() - t0) / done), flush=True)
        if args.once:
            break
        time.sleep(10)
    print("{} images processed".format(done), flush=True)


if __name__ == "__main__":
    main()
