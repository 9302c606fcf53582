"""Cityscapes-Part ground truth without a GPU: the numpy oracle (cityscapes_part_oracle.py) against a hand-written uid table, the TIFF
round trip the part files rely on, the record builder's refusals, and the record builder with the oracle in place of the device
functions (it must not modify its input)."""
import copy

import numpy as np
import pytest
import torch
from PIL import Image

import cityscapes_part_oracle as O


def test_oracle_decode_against_the_hand_table():
    table = np.asarray(O.HAND_TABLE)
    assert table[:, 0].tolist() == [0, 1, 99, 100, 999, 1000, 24012, 99999, 100000, 2401203, 2600000, 9999999]
    sids, iids, pids = O.decode_uids(table[:, 0])
    assert sids.tolist() == table[:, 1].tolist() and iids.tolist() == table[:, 2].tolist() and pids.tolist() == table[:, 3].tolist()
    assert sids.dtype == iids.dtype == pids.dtype == np.int32
    assert O.part_label(table[:, 0]).tolist() == [0] * 9 + [3, 0, 99]
    for bad in (-1, 10000000):
        with pytest.raises(ValueError):
            O.decode_uids(np.asarray([5, bad]))


def test_int32_tiff_round_trip(tmp_path):
    from partdistillation_amd.data.cityscapes_part_record import read_part_map
    uids = O.scene(np.random.RandomState(0), 37, 53, False)[1]
    uids[0, :3] = [0, 9999999, 2401203]
    path = tmp_path / "x_gtFinePanopticParts.tif"
    Image.fromarray(uids).save(path)
    back = read_part_map(str(path), 37, 53)
    assert back.dtype == np.int32 and back.shape == (37, 53) and np.array_equal(back, uids)
    assert np.array_equal(read_part_map(path, 37, 53), uids)                  # a path object
    assert read_part_map(uids, 37, 53) is not None and read_part_map(torch.from_numpy(uids), 37, 53).dtype == torch.int32


def test_bad_part_files(tmp_path):
    from partdistillation_amd.data.cityscapes_part_record import load_object_and_parts, read_part_map
    record, uids = O.scene(np.random.RandomState(1), 37, 53, False)
    Image.fromarray((uids % 251).astype(np.uint8)).save(tmp_path / "u8.tif")
    Image.fromarray(uids[:, :52].copy()).save(tmp_path / "narrow.tif")
    for bad in (tmp_path / "u8.tif", tmp_path / "narrow.tif", uids.astype(np.int64), uids.astype(np.float32), uids.T.copy(), uids[None],
                torch.from_numpy(uids).long()):
        with pytest.raises(ValueError, match=r"int32 \[37, 53\] expected"):
            read_part_map(bad, 37, 53)
        with pytest.raises(ValueError, match=r"int32 \[37, 53\] expected"):   # before any device work: no GPU here
            load_object_and_parts(record, bad, "cuda")


def _oracle_in_place_of_the_device(monkeypatch):
    import partdistillation_amd.data.cityscapes_part_record as R
    monkeypatch.setattr(R, "_object_planes", lambda segs, h, w, device: np.stack([O.object_mask(s, h, w) for s in segs]).astype(np.uint8))
    monkeypatch.setattr(R, "_part_labels", lambda uids, device: (O.part_label(uids), lambda: None))
    monkeypatch.setattr(R._drle, "plane_runs", lambda planes, binary: O.runs_table(np.asarray(planes) != 0 if binary else planes))
    monkeypatch.setattr(R._drle, "encode_plane_labels", O.encode_plane_labels)
    return R


@pytest.mark.parametrize("polygons", [False, True])
def test_record_builder_on_the_oracle_does_not_modify_its_input(monkeypatch, polygons):
    R = _oracle_in_place_of_the_device(monkeypatch)
    record, uids = O.scene(np.random.RandomState(2), 37, 53, polygons)
    before, uids_before = copy.deepcopy(record), uids.copy()
    got = R.load_object_and_parts(record, uids, "cuda")
    want = O.load_object_and_parts(record, uids)
    assert got == want and [len(p) for p in got[1]] != [0] * 4 and len(got[0]) == 4 and got[1][1] == []
    assert all(isinstance(o["segmentation"]["counts"], bytes) for o in got[0])
    for for_segmentation in (True, False):
        mine = list(R.cityscapes_part_records(record, uids, for_segmentation, "cuda"))
        theirs = O.records(record, uids, for_segmentation)
        assert len(mine) == len(theirs) == (3 if for_segmentation else 1)
        for a, b in zip(mine, theirs):
            assert {k: v for k, v in a.items() if k != "image"} == {k: v for k, v in b.items() if k != "image"}
    assert np.array_equal(uids, uids_before) and sorted(record) == sorted(before) and "part_annotations" not in record
    assert record["annotations"] == before["annotations"] and np.array_equal(record["image"], before["image"])
    empty = dict(record, annotations=[])
    assert R.load_object_and_parts(empty, uids, "cuda") == (None, None) and list(R.cityscapes_part_records(empty, uids, True, "cuda")) == []


def test_part_id_beyond_the_table_is_an_index_error(monkeypatch):
    R = _oracle_in_place_of_the_device(monkeypatch)
    record, uids = O.scene(np.random.RandomState(3), 37, 53, False)
    uids[:] = 2801206                                                         # pid 6 under the bus: 18 + 6 - 1 = 23
    with pytest.raises(IndexError):
        R.load_object_and_parts(record, uids, "cuda")
    with pytest.raises(IndexError):
        O.load_object_and_parts(record, uids)
