"""Device COCO-RLE codec (include/pd_rle.h, partdistillation_amd/functions/rle.py) against the host codec utils/rle.py: the same bytes and the
same integers, no tolerance anywhere.  The shapes are tiny; the edge shapes come from functions.rle.SEG_ROWS (rows a lane walks per key)
and the 64 columns of a wavefront."""
import types

import numpy as np
import pytest
import torch

from partdistillation_amd.functions import rle as R
from partdistillation_amd.utils import rle

pytestmark = pytest.mark.gpu

S = R.SEG_ROWS


def _np_runs(planes, binary):
    """(offsets, starts, values) of uint8 planes [n, H, W] by numpy: run-length of planes[i].T.reshape(-1)"""
    offsets, starts, values = [0], [], []
    for p in planes:
        f = p.T.reshape(-1)
        f = (f != 0).astype(np.uint8) if binary else f
        st = np.concatenate(([0], np.flatnonzero(f[1:] != f[:-1]) + 1)) if f.size else np.zeros(0, dtype=np.int64)
        starts.append(st.astype(np.int32))
        values.append(f[st])
        offsets.append(offsets[-1] + len(st))
    return np.asarray(offsets, dtype=np.int32), np.concatenate(starts), np.concatenate(values)


def _check_masks(masks):
    """masks: bool numpy [n, H, W] -> plane_runs and encode_masks of the device copy equal numpy and the host codec"""
    dev = torch.from_numpy(masks).cuda()
    offsets, starts, values, nonzero = R.plane_runs(dev, binary=True)
    want = _np_runs(masks.astype(np.uint8), True)
    assert offsets.dtype == np.int32 and starts.dtype == np.int32 and values.dtype == np.uint8 and nonzero.dtype == np.int64
    for got, ref in zip((offsets, starts, values), want):
        assert np.array_equal(got, ref)
    assert np.array_equal(nonzero, masks.sum((1, 2)))
    segs, areas = R.encode_masks(dev)
    assert segs == rle.masks_to_coco_json(masks) and areas.dtype == np.int64 and np.array_equal(areas, masks.sum((1, 2)))
    return segs


def _blobs(n, H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), dtype=bool)
    for i in range(n):
        for _ in range(6):
            cy, cx, r = rng.randint(0, H), rng.randint(0, W), rng.randint(3, max(4, min(H, W) // 3))
            out[i] ^= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return out


def test_single_pixels_and_constant_masks():
    assert [s["segmentation"]["counts"] for s in _check_masks(np.zeros((1, 1, 1), bool))] == ["1"]
    assert [s["segmentation"]["counts"] for s in _check_masks(np.ones((1, 1, 1), bool))] == ["01"]
    _check_masks(np.zeros((2, 6, 5), bool))
    _check_masks(np.ones((2, 6, 5), bool))


def test_first_pixel_set_gives_a_leading_zero_count():
    m = np.zeros((1, 5, 3), bool)
    m[0, 0, 0] = True
    segs = _check_masks(m)
    assert rle.string_to_counts(segs[0]["segmentation"]["counts"]).tolist() == [0, 1, 14]


def test_column_seam_5x3():
    m = np.zeros((2, 5, 3), bool)
    m[0, 3:, 0], m[0, :2, 1] = True, True          # one run from the bottom of column 0 into the top of column 1
    m[1, 3:, 0] = True                             # the value changes exactly at that seam
    segs = _check_masks(m)
    assert [rle.string_to_counts(s["segmentation"]["counts"]).tolist() for s in segs] == [[3, 4, 8], [3, 2, 10]]


@pytest.mark.parametrize("W", [63, 65, 67])
@pytest.mark.parametrize("H", [S - 1, S, S + 1, 2 * S + 1])
def test_segment_edges(H, W):
    if H < 1:
        pytest.skip("SEG_ROWS = 1 has no shorter plane")
    rng = np.random.RandomState(H * 100 + W)
    m = rng.rand(3, H, W) < 0.5
    m[1] = False
    m[1, min(S, H - 1):, ::2] = True               # changes exactly on the first segment edge, in every other column
    m[2] = False
    m[2, :, 1::3] = True                           # whole columns: runs that span every segment of the column
    m[2, :, 64:] = True                            # ... and cross from one 64-column block into the next (W > 64)
    _check_masks(m)


def test_checkerboard_capacity_and_growth(monkeypatch):
    """33 x 70 checkerboard: H is odd, so the value also flips across every column seam and each of the H * W pixels is a run"""
    from partdistillation_amd import lib as L
    H, W, cap = 33, 70, 7
    m = (np.indices((H, W)).sum(0) % 2).astype(np.uint8)[None]
    want = _np_runs(m, True)
    total = int(want[0][1])
    assert total == H * W and np.array_equal(want[1], np.arange(H * W))
    lib, dev = L.load(), torch.from_numpy(m).cuda()
    work = torch.empty(lib.pd_rle_runs_workspace_bytes(1, H, W), dtype=torch.uint8, device="cuda")
    starts = torch.full((total + 8,), -77, dtype=torch.int32, device="cuda")
    values = torch.full((total + 8,), 99, dtype=torch.uint8, device="cuda")
    offsets = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    nonzero = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    rc = lib.pd_rle_plane_runs(dev.data_ptr(), H * W, 1, H, W, 1, cap, starts.data_ptr(), values.data_ptr(), offsets.data_ptr(),
                               nonzero.data_ptr(), work.data_ptr(), L.current_stream())
    assert rc == 0
    assert offsets.tolist() == [0, total] and nonzero.tolist() == [int(m.sum())]
    assert np.array_equal(starts[:cap].cpu().numpy(), want[1][:cap]) and np.array_equal(values[:cap].cpu().numpy(), want[2][:cap])
    assert bool((starts[cap:] == -77).all()) and bool((values[cap:] == 99).all())
    # the wrapper, starting from a buffer of 16 runs, must grow and return the whole table
    monkeypatch.setattr(R, "_MIN_CAPACITY", 16)
    monkeypatch.setattr(R, "_buffers", {})
    _check_masks(m.astype(bool))
    (buf,) = R._buffers.values()
    assert buf.capacity >= total
    _check_masks(np.concatenate([m, 1 - m]).astype(bool))          # twice the runs: grows again


def test_three_planes_with_an_empty_one_between_and_sliced_input():
    m = _blobs(3, 21, 45, 2)
    m[1] = False
    _check_masks(m)
    full = torch.from_numpy(_blobs(6, 21, 45, 4)).cuda()
    for view in (full[::2], full[1:4], full[:, 2:19, 3:40], full.permute(0, 2, 1), full[:1].expand(3, -1, -1)):
        assert not view.is_contiguous() or view.storage_offset()
        got = R.encode_masks(view)
        assert got[0] == rle.masks_to_coco_json(view.cpu()) and np.array_equal(got[1], view.sum((1, 2)).cpu().numpy())


def test_label_map_mode():
    rng = np.random.RandomState(8)
    lab = (rng.randint(0, 4, size=(2 * S + 3, 67)) * 85).astype(np.uint8)          # 0, 85, 170, 255
    lab[2:6, 5], lab[6:9, 5] = 1, 2                                                # 1 directly above 2: two runs
    lab[-1, 9], lab[0, 10] = 1, 2                                                  # ... and across a column seam
    offsets, starts, values, nonzero = R.plane_runs(torch.from_numpy(lab).cuda()[None], binary=False)
    want = _np_runs(lab[None], False)
    for got, ref in zip((offsets, starts, values), want):
        assert np.array_equal(got, ref)
    assert nonzero.tolist() == [int((lab != 0).sum())] and 255 in values and 1 in values and 2 in values
    flat = lab.T.reshape(-1)
    i = int(np.flatnonzero(starts == 5 * lab.shape[0] + 6)[0])
    assert values[i] == 2 and values[i - 1] == 1 and flat[starts[i]] == 2


def test_encode_label_map_with_an_absent_label():
    rng = np.random.RandomState(9)
    lab = rng.choice(np.array([0, 1, 3, 4], dtype=np.uint8), size=(37, 70))         # 2 is absent
    dev = torch.from_numpy(lab).cuda()
    segs, counts = R.encode_label_map(dev)
    assert segs == rle.labels_to_coco_json(lab, [1, 3, 4])
    assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(lab.reshape(-1), minlength=256))
    segs, _ = R.encode_label_map(dev, present=[1, 2, 3, 4])
    assert segs == rle.labels_to_coco_json(lab, [1, 2, 3, 4]) and len(segs) == 4


def test_random_blobs_twice_identical():
    m = _blobs(4, 257, 130, 6)
    dev = torch.from_numpy(m).cuda()
    a, b = R.plane_runs(dev, binary=True), R.plane_runs(dev, binary=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _check_masks(m)


def test_zero_sized_inputs_are_answered_on_the_host():
    for shape in ((0, 5, 3), (2, 0, 4), (2, 4, 0)):
        m = torch.zeros(shape, dtype=torch.bool, device="cuda")
        segs, areas = R.encode_masks(m)
        assert segs == rle.masks_to_coco_json(m.cpu()) and areas.tolist() == [0] * shape[0]


def _decode_cases(H, W):
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    a[3:20, 5:40], b[10:30, 30:60] = True, True                                    # overlap in rows 10-19, columns 30-39
    first = np.zeros((H, W), bool)
    first[:4, 0], first[H - 1, W - 1] = True, True                                 # starts with ones, ends with a one
    return np.stack([a, b, first, np.zeros((H, W), bool), _blobs(1, H, W, 12)[0]])


def test_decode_label_map_and_masks():
    H, W = 37, 70
    masks = _decode_cases(H, W)
    segs = rle.masks_to_coco_json(masks)
    host = np.stack([rle.decode(s["segmentation"]) for s in segs])
    assert np.array_equal(host, masks)
    labels = R.decode_label_map(segs, (H, W), "cuda")
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (H, W) and labels.is_cuda
    want = (host.astype(np.int64) * (np.arange(len(segs)) + 1)[:, None, None]).sum(0)
    assert np.array_equal(labels.cpu().numpy(), want)
    two = R.decode_label_map(segs[:2], (H, W), "cuda").cpu().numpy()
    assert (two[10:20, 30:40] == 3).all() and set(np.unique(two)) == {0, 1, 2, 3}
    got = R.decode_masks(segs, (H, W), "cuda")
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), host)
    assert R.encode_masks(got)[0] == segs                                          # round trip
    assert R.encode_masks(R.decode_masks([s["segmentation"] for s in segs], (H, W), "cuda"))[0] == segs
    zero = R.decode_label_map([], (H, W), "cuda")
    assert tuple(zero.shape) == (H, W) and not bool(zero.any())
    assert tuple(R.decode_masks([], (H, W), "cuda").shape) == (0, H, W)
    with pytest.raises(ValueError, match="do not match"):
        R.decode_label_map(segs, (H, W + 1), "cuda")


def test_decode_overwrites_every_output_pixel():
    from partdistillation_amd import lib as L
    H, W = 37, 70
    masks = _decode_cases(H, W)
    starts, offsets = rle.segmentations_to_starts([s["segmentation"] for s in rle.masks_to_coco_json(masks)], (H, W))
    n, lib = len(masks), L.load()
    st, off = torch.from_numpy(starts).cuda(), torch.from_numpy(offsets).cuda()
    labels = torch.full((H, W), -12345, dtype=torch.int32, device="cuda")
    out = torch.full((n, H, W), 0xAB, dtype=torch.uint8, device="cuda")
    want = (masks.astype(np.int64) * (np.arange(n) + 1)[:, None, None]).sum(0)
    assert lib.pd_rle_decode(st.data_ptr(), off.data_ptr(), n, H, W, labels.data_ptr(), out.data_ptr(), L.current_stream()) == 0
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(out.cpu().numpy(), masks.astype(np.uint8))
    labels.fill_(-12345)
    assert lib.pd_rle_decode(None, None, 0, H, W, labels.data_ptr(), None, L.current_stream()) == 0
    assert not bool(labels.any())
    assert lib.pd_rle_decode(st.data_ptr(), off.data_ptr(), n, H, W, None, None, L.current_stream()) != 0
    assert lib.pd_rle_decode(st.data_ptr(), off.data_ptr(), -1, H, W, labels.data_ptr(), None, L.current_stream()) != 0


def test_plane_runs_rejects_bad_arguments():
    from partdistillation_amd import lib as L
    lib = L.load()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    assert lib.pd_rle_runs_workspace_bytes(1, 46341, 46341) == -1 and lib.pd_rle_runs_workspace_bytes(-1, 4, 4) == -1
    assert lib.pd_rle_runs_workspace_bytes(1, 2, 2) > 0
    for args in ((None, 4, 1, 2, 2, 1, 4, p, p, p, p, p), (p, 4, 1, 2, 2, 1, 4, p, p, None, p, p), (p, 4, 1, 2, 2, 1, 4, p, p, p, p, None),
                 (p, 4, -1, 2, 2, 1, 4, p, p, p, p, p), (p, 4, 1, -2, 2, 1, 4, p, p, p, p, p), (p, 4, 1, 2, 2, 1, -4, p, p, p, p, p),
                 (p, 4, 1, 46341, 46341, 1, 4, p, p, p, p, p), (p, 4, 1, 2, 2, 1, 4, None, p, p, p, p)):
        assert lib.pd_rle_plane_runs(*args, L.current_stream()) == -1, args
        assert b"pd_rle_plane_runs" in lib.pd_last_error()


def _instances(masks, seed):
    from partdistillation_amd.compat import Instances
    g = torch.Generator().manual_seed(seed)
    inst = Instances(tuple(masks.shape[1:]))
    inst.pred_masks = masks
    inst.pred_classes = torch.randint(0, 5, (masks.shape[0],), generator=g).cuda()
    inst.scores = torch.rand(masks.shape[0], generator=g).cuda()
    return inst


def _same_dict(got, want):
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k]
        assert type(g) is type(w), k
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.device == w.device and torch.equal(g, w), k
        elif isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w), k
        else:
            assert g == w, k


@pytest.mark.parametrize("which", ["generated_part_labels", "part_segmentation"])
def test_save_functions_write_the_host_codecs_dict(tmp_path, which):
    import os
    from partdistillation_amd import inference as I
    masks_h = torch.from_numpy(_blobs(3, 2 * S + 5, 67, 21))
    masks_h[1] = False
    inst = _instances(masks_h.cuda(), 5)
    inp = {"file_name": "n01/x.JPEG", "image_id": "x_17", "class_code": "n01"}
    model = types.SimpleNamespace(root_save_path=str(tmp_path))
    H, W = masks_h.shape[1:]
    common = {"file_name": inp["file_name"], "image_id": inp["image_id"], "class_code": inp["class_code"], "height": H, "width": W,
              "part_masks": rle.masks_to_coco_json(masks_h), "part_labels": inst.pred_classes.cpu()}
    if which == "generated_part_labels":
        got = I.save_generated_part_labels(model, inp, torch.tensor(3).cuda(), inst)
        want = dict(common, object_ratio=masks_h.sum().long().item() / (H * W), part_ratios=masks_h.flatten(1).sum(-1) / (H * W),
                    object_class_label=3, part_scores=inst.scores.cpu().numpy())
    else:
        got = I.save_part_segmentation(model, inp, inst)
        area = masks_h.sum().long().item()
        want = dict(common, part_area_ratios=masks_h.flatten(1).sum(-1).long() / area, object_ratio=area / (H * W),
                    part_scores=inst.scores.cpu().numpy())
    _same_dict(got, want)
    _same_dict(torch.load(os.path.join(str(tmp_path), "n01", "x_17"), weights_only=False), want)


def test_refine_proposals_with_no_mean_field_step_re_encodes_its_input():
    import partdistillation_amd.postprocess_dcrf as P
    size = 64
    lab = np.zeros((size, size), dtype=np.int64)
    lab[4:44, 2:22], lab[6:30, 24:44], lab[10:46, 46:62] = 1, 2, 3
    masks = np.stack([lab == c for c in (1, 2, 3)])
    image = np.random.RandomState(1).randint(0, 256, size=(48, size, 3)).astype(np.uint8)
    for key in P.MASK_KEYS:
        data = {"file_name": "x.pth", key: rle.masks_to_coco_json(masks)}
        out = P.refine_proposals(data, image, size=size, t=0)
        assert out is data and out[key] == rle.masks_to_coco_json(masks) and list(out) == ["file_name", key]
    for empty in ({"file_name": "x"}, {"part_masks": None}, {"part_mask": []}):
        before = dict(empty)
        assert P.refine_proposals(empty, image, size=size) is empty and empty == before
    with pytest.raises(ValueError, match="do not match"):
        P.refine_proposals({"part_masks": rle.masks_to_coco_json(masks[:, :8])}, image, size=size)
