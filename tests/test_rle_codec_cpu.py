"""Host half of the device COCO-RLE codec (partdistillation_amd/functions/rle.py, utils/rle.py): run tables assembled into strings, the
vectorised string parser against a character-loop restatement, and the wrappers' refusals.  The yardstick is the host codec utils/rle.py
(masks_to_coco_json / decode); equality is exact."""
import numpy as np
import pytest
import torch

from partdistillation_amd.utils import rle


def _loop_string_to_counts(s):
    """rleFrString, one character at a time (the parser utils/rle.py had before it was vectorised)"""
    if isinstance(s, str):
        s = s.encode("ascii")
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.asarray(cnts, dtype=np.int64)


def _loop_run_table(mask):
    """(starts, values) of the column-major flattening of a 2-d array, by a plain loop"""
    h, w = mask.shape
    starts, values, prev = [], [], None
    for x in range(w):
        for y in range(h):
            v = int(mask[y, x])
            if prev is None or v != prev:
                starts.append(x * h + y)
                values.append(v)
            prev = v
    return np.asarray(starts, dtype=np.int32), np.asarray(values, dtype=np.uint8)


def _masks():
    rng = np.random.RandomState(11)
    out = [np.zeros((1, 1), bool), np.ones((1, 1), bool), np.zeros((4, 6), bool), np.ones((5, 3), bool), np.zeros((0, 4), bool)]
    first = np.zeros((5, 3), bool)
    first[0, 0] = True                                                  # leading zero count
    seam = np.zeros((5, 3), bool)
    seam[3:, 0], seam[:2, 1] = True, True                               # a run across the bottom of column 0 into column 1
    out += [first, seam, (np.indices((7, 9)).sum(0) % 2).astype(bool)]
    for _ in range(12):
        h, w = rng.randint(1, 30, size=2)
        out.append(rng.rand(h, w) < rng.rand())
    return out


def test_run_tables_assemble_into_the_host_codecs_strings():
    masks = _masks()
    for m in masks:
        starts, values = _loop_run_table(m)
        got = rle.run_table_to_coco_json([0, len(starts)], starts, values, m.shape)
        assert got == rle.masks_to_coco_json(m[None]), m.shape
    same = [m for m in masks if m.shape == (5, 3)]                       # several masks in one table
    tables = [_loop_run_table(m) for m in same]
    offsets = np.concatenate(([0], np.cumsum([len(s) for s, _ in tables])))
    got = rle.run_table_to_coco_json(offsets, np.concatenate([s for s, _ in tables]), np.concatenate([v for _, v in tables]), (5, 3))
    assert len(same) == 4 and got == rle.masks_to_coco_json(np.stack(same))


def test_label_map_runs_assemble_into_labels_to_coco_json():
    rng = np.random.RandomState(3)
    labels = rng.randint(0, 4, size=(9, 7)).astype(np.uint8) * 85        # 0, 85, 170, 255
    labels[2:5, 3] = 1
    labels[5:8, 3] = 2
    starts, values = _loop_run_table(labels)
    lengths = np.diff(starts.astype(np.int64), append=labels.size)
    present = [1, 2, 7, 85, 255]                                         # 7 is absent: an all-zero mask
    assert rle.runs_to_coco_json(values, lengths, labels.shape, present) == rle.labels_to_coco_json(labels, present)


@pytest.mark.parametrize("counts", [[], [0, 4], [0, 70000, 5, 69990], [2 ** 15 - 1, 2 ** 15, 2 ** 15 + 1, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 1],
                                    [2 ** 20, 3, 2 ** 24, 2 ** 15, 1, 2 ** 30]])
def test_vectorised_string_to_counts_equals_the_character_loop(counts):
    s = rle.counts_to_string(counts)
    if counts == [0, 4]:
        assert s == b"04"
    got = rle.string_to_counts(s)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_string_to_counts(s)) and got.tolist() == counts
    assert np.array_equal(rle.string_to_counts(s.decode("ascii")), got)


def test_vectorised_string_to_counts_on_random_masks():
    for m in _masks():
        s = rle.encode(m)["counts"]
        assert np.array_equal(rle.string_to_counts(s), _loop_string_to_counts(s))
        assert np.array_equal(rle.decode(rle.encode(m)), m)


def test_segmentations_to_starts_is_the_sampler_format():
    m = np.zeros((5, 3), bool)
    m[0, 0], m[3:, 1] = True, True                                       # counts 0 1 7 2 5
    segs = [rle.encode(m), rle.encode(np.zeros((5, 3), bool)), {"size": [5, 3], "counts": [3, 12]}, {"size": [5, 3], "counts": b""}]
    starts, offsets = rle.segmentations_to_starts(segs, (5, 3))
    assert starts.dtype == np.int32 and offsets.dtype == np.int32
    assert offsets.tolist() == [0, 5, 6, 8, 9] and starts.tolist() == [0, 0, 1, 8, 10, 0, 0, 3, 0]
    starts, offsets = rle.segmentations_to_starts([], (5, 3))
    assert starts.shape == (0,) and offsets.tolist() == [0]


def test_wrappers_refuse_cpu_tensors():
    from partdistillation_amd.functions import rle as R
    assert R.SEG_ROWS >= 1
    for call in (lambda: R.plane_runs(torch.zeros(1, 4, 4, dtype=torch.uint8), True),
                 lambda: R.encode_masks(torch.zeros(1, 4, 4, dtype=torch.bool)),
                 lambda: R.encode_label_map(torch.zeros(4, 4, dtype=torch.uint8)),
                 lambda: R.decode_label_map([rle.encode(np.zeros((4, 4), bool))], (4, 4), "cpu"),
                 lambda: R.decode_masks([rle.encode(np.zeros((4, 4), bool))], (4, 4), "cpu")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_decode_raises_on_a_size_mismatch():
    from partdistillation_amd.functions import rle as R
    segs = [{"segmentation": rle.encode(np.zeros((4, 4), bool))}, {"segmentation": rle.encode(np.zeros((4, 5), bool))}]
    for fn in (R.decode_label_map, R.decode_masks):
        with pytest.raises(ValueError, match="do not match"):
            fn(segs, (4, 4), "cpu")
