"""Test helper (not collected): the reference's ProposalGenerationMapper and ImagenetPartRankingDatasetMapper restated with numpy on the
oracle's pieces — the image through input_chain_oracle.base_image_ref (Pillow-pinned), the masks through
oracle.input_pipeline_ref.rle_decode, the pad and the union in numpy, the boxes from the dense mask."""
import numpy as np

import input_chain_oracle as B
from oracle import input_pipeline_ref as R


def decode(seg):
    counts = seg["counts"]
    counts = R.rle_string_to_counts(counts) if isinstance(counts, (str, bytes)) else np.asarray(counts, dtype=np.int64)
    return R.rle_decode(counts, int(seg["size"][0]), int(seg["size"][1]))


def dense_box(mask):
    """BitMasks.get_bounding_boxes of one dense mask: [x0, y0, x1 + 1, y1 + 1] float32, zeros when it is empty"""
    xs, ys = np.flatnonzero(mask.any(axis=0)), np.flatnonzero(mask.any(axis=1))
    if len(xs) == 0:
        return np.zeros(4, dtype=np.float32)
    return np.asarray([xs[0], ys[0], xs[-1] + 1, ys[-1] + 1], dtype=np.float32)


def proposal_generation_ref(record, image, rng, S, with_given_mask):
    """-> None or {"image" [3, h, w], "size", and with masks "masks" bool [k, mh, mw], "classes", "boxes" float32 [k, 4]}; consumes
    ResizeScale's draw"""
    rng.uniform(1.0, 1.0)
    img = B.base_image_ref(image, S, False)
    want = {"image": img.transpose(2, 0, 1), "size": img.shape[:2]}
    if with_given_mask:
        annos = record.get("pseudo_annotations", [])
        masks = [decode(a["segmentation"]) for a in annos]
        keep = [i for i, m in enumerate(masks) if m.any()]                  # filter_empty_instances(by_box=False)
        if not keep:
            return None
        want["masks"] = np.stack([masks[i] for i in keep])
        want["classes"] = [int(annos[i].get("category_id", -1)) for i in keep]
        want["boxes"] = np.stack([dense_box(masks[i]) for i in keep])
    return want


def part_ranking_ref(record, image, rng, S, class_index):
    """-> {"image" [3, S, S], "mask" bool [1, S, S], "classes"}; consumes ResizeScale's and then FixedSizeCrop's draw"""
    rng.uniform(1.0, 1.0)
    rng.uniform(0.0, 1.0)
    img = B.base_image_ref(image, S, True)
    bh, bw = B.base_shape(image.shape[0], image.shape[1], S)
    masks = np.stack([decode(a["segmentation"]) for a in record["pseudo_annotations"]])
    assert masks.shape[1:] == (bh, bw)
    padded = np.zeros((len(masks), S, S), dtype=bool)                       # FixedSizeCrop pads masks with 0
    padded[:, :bh, :bw] = masks
    return {"image": img.transpose(2, 0, 1), "mask": padded.any(0)[None], "classes": [class_index[record["class_code"]]]}


def canvas_ref(masks, sx, sy, groups, canvas):
    """pd_rle_sample_groups_canvas_u8 as a numpy loop: masks bool [n, H, W] -> (planes uint8 [G, out_h, out_w], member_area, group_area)"""
    n, (out_h, out_w) = len(masks), canvas
    vh, vw = len(sy), len(sx)
    sampled = np.zeros((n, out_h, out_w), dtype=np.uint8)
    for m in range(n):
        for y in range(vh):
            for x in range(vw):
                sampled[m, y, x] = masks[m][sy[y], sx[x]]
    planes = np.zeros((len(groups), out_h, out_w), dtype=np.uint8)
    for g, members in enumerate(groups):
        for m in members:
            planes[g] |= sampled[m]
    return planes, sampled.reshape(n, -1).sum(axis=1).astype(np.int32), planes.reshape(len(groups), -1).sum(axis=1).astype(np.int32)
