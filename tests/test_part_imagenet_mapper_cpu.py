"""Host side of the PartImageNet mapper (partdistillation_amd/data/part_imagenet_mapper.py, functions/polygon.py): the rasteriser's
restatement (tests/poly_oracle.py) against what can be known without pycocotools — integer rectangles, an independent even-odd test away
from the outline, the original's run-merge ending and this project's RLE decoder — then the exact table sizes the host hands the kernel,
the argument checks of pd_poly_crossings_i32, the config surface and the host decisions of the mapper.  No GPU."""
import copy
import functools
import os

import numpy as np
import pytest

import poly_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "partdistillation_amd", "configs")


@functools.lru_cache(maxsize=None)
def _random_cases():
    """300 seeded polygons with 3-7 vertices, coordinates uniform in [-6, 54], canvases 8..47 -> [(poly, h, w, oracle table)]"""
    rng = np.random.RandomState(300)
    out = []
    for _ in range(300):
        k = rng.randint(3, 8)
        poly = rng.uniform(-6, 54, 2 * k)
        h, w = (int(v) for v in rng.randint(8, 48, 2))
        out.append((poly, h, w, P.table(poly, h, w)))
    return out


# ------------------------------------------------------------------------------------------------ the restatement
def test_integer_rectangle():
    """an integer rectangle [x0, x1) x [y0, y1) covers exactly the pixels whose centres it contains"""
    want = np.zeros((12, 15), dtype=bool)
    want[3:9, 2:11] = True
    assert np.array_equal(P.mask([2, 3, 2, 9, 11, 9, 11, 3], 12, 15), want)
    assert P.table([2, 3, 2, 9, 11, 9, 11, 3], 12, 15).tolist() == [0] + sorted([x * 12 + 3 for x in range(2, 11)] + [x * 12 + 9 for x in range(2, 11)])


def test_oracle_agrees_with_even_odd_away_from_the_outline():
    total = compared = wrong = 0
    for poly, h, w, tab in _random_cases():
        inside, dist = P.even_odd(poly, h, w)
        far = dist > 1.0
        total += h * w
        compared += int(far.sum())
        wrong += int((P.table_mask(tab, h, w)[far] != inside[far]).sum())
    print(f"compared {compared} of {total} pixels ({100.0 * compared / total:.1f} %), {wrong} mismatches")
    assert compared >= 0.8 * total
    assert wrong == 0


def test_parity_table_equals_the_run_merge_and_decodes_through_utils_rle():
    """`pixel set iff an odd number of boundary positions <= it` is what the original's difference-and-merge of zero-length runs produces"""
    from partdistillation_amd.utils import rle
    for poly, h, w, tab in _random_cases():
        counts = P.run_merge_counts(poly, h, w)
        want = P.table_mask(tab, h, w)
        assert sum(counts) == h * w and all(c > 0 for c in counts[1:])
        assert np.array_equal(P.counts_mask(counts, h, w), want)
        assert np.array_equal(rle.decode({"size": [h, w], "counts": rle.counts_to_string(np.asarray(counts, dtype=np.int64))}), want)
        # and as a run-starts table with repeated entries, through the host parser the sibling mappers use
        starts, offsets = rle.segmentations_to_starts([{"size": [h, w], "counts": counts}], (h, w))
        assert np.array_equal(P.table_mask(starts, h, w), want)


def test_fused_multiply_add_would_change_tables():
    """the four triangles (upsampled integer vertices / 5) on a 24 x 24 canvas for which fma(slope, t, start) rounds to another row"""
    for tri in P.CONTRACTION_TRIANGLES:
        poly = (np.asarray(tri, dtype=np.float64) / 5).reshape(-1)
        assert [list(t) for t in zip(*P.upsample(poly))][:3] == [list(t) for t in tri]
        assert not np.array_equal(P.table(poly, 24, 24), P.table(poly, 24, 24, fused=True))


# ------------------------------------------------------------------------------------------------ polygon_tables
def _special_polygons():
    return [("left of the canvas", [-9, 2, -3, 2, -3, 8, -9, 9], 10, 12), ("right of it", [14, 2, 19, 2, 19, 8], 10, 12),
            ("above", [1, -9, 8, -9, 8, -2], 10, 12), ("below", [1, 12, 8, 12, 8, 19, 2, 17], 10, 12),
            ("covering", [-5, -5, 60, -5, 60, 60, -5, 60], 20, 30), ("h = 1", [0.3, -2, 7.6, -1, 5, 3], 1, 9),
            ("w = 1", [-2, 0.2, 3, 4.4, -1, 8], 9, 1), ("h = w = 1", [-1, -1, 3, -1, 3, 3, -1, 3], 1, 1),
            ("first vertex repeated", [1, 1, 8, 1, 8, 8, 1, 1], 10, 10), ("all vertices equal", [3, 3, 3, 3, 3, 3], 10, 10),
            ("repeats inside", [1, 1, 1, 1, 8, 2, 8, 2, 4, 9], 10, 10)]


def test_polygon_tables_counts_are_exact():
    from partdistillation_amd.functions.polygon import polygon_tables, upsample
    cases = [(poly, h, w) for poly, h, w, _ in _random_cases()] + [(np.asarray(p, dtype=np.float64), h, w) for _, p, h, w in _special_polygons()]
    for poly, h, w in cases:
        xy, vo, to = polygon_tables([poly], h, w)
        assert xy.dtype == np.float64 and vo.dtype == np.int32 and to.dtype == np.int32 and xy.shape == (len(poly) // 2, 2)
        assert vo.tolist() == [0, len(poly) // 2] and to.tolist() == [0, 1 + len(P.crossings(poly, h, w))], (poly, h, w)
        X, Y = P.upsample(poly)
        assert upsample(xy).tolist() == [list(t) for t in zip(X[:-1], Y[:-1])]
    for name, poly, h, w in _special_polygons()[:2]:
        assert polygon_tables([poly], h, w)[2].tolist() == [0, 1], name       # wholly left / right: no column is crossed, the table is [0]
    for name, poly, h, w in _special_polygons()[2:4]:                         # wholly above / below: the columns ARE crossed, with the row
        tab = P.table(poly, h, w)                                             # clamped to 0 / to h: every position twice, nothing set
        assert len(tab) > 1 and (np.unique(tab[1:], return_counts=True)[1] % 2 == 0).all() and not P.table_mask(tab, h, w).any(), name
    # several polygons on one canvas: CSR offsets, the vertices side by side
    polys = [c[0] for c in cases[:7]]
    xy, vo, to = polygon_tables(polys, 33, 21)
    assert np.diff(vo).tolist() == [len(p) // 2 for p in polys] and np.array_equal(xy.reshape(-1), np.concatenate(polys))
    assert np.diff(to).tolist() == [1 + len(P.crossings(p, 33, 21)) for p in polys]
    xy, vo, to = polygon_tables([], 5, 5)
    assert xy.shape == (0, 2) and vo.tolist() == [0] and to.tolist() == [0]
    assert polygon_tables([np.asarray(polys[0]).reshape(-1, 2)], 33, 21)[2].tolist() == to.tolist()[:1] + [1 + len(P.crossings(polys[0], 33, 21))]


def test_polygon_tables_refusals():
    from partdistillation_amd.functions.polygon import polygon_tables
    with pytest.raises(ValueError, match="from 7 coordinates"):
        polygon_tables([[1, 1, 5, 1, 5, 5, 2]], 8, 8)
    with pytest.raises(ValueError, match="from 4 coordinates"):
        polygon_tables([[1, 1, 5, 1, 5, 5], [1, 1, 5, 5]], 8, 8)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            polygon_tables([[1, 1, 5, bad, 5, 5]], 8, 8)
    limit = (2.0 ** 30 - .5) / 5
    for bad in (limit, -limit - 1, 1e300):
        with pytest.raises(ValueError, match="out of range"):
            polygon_tables([[1, 1, bad, 1, 5, 5]], 8, 8)
    assert polygon_tables([[1, 1, np.nextafter(limit, 0), 1, 5, 5]], 8, 8)[2].tolist() == [0, 1 + 2 * 7]    # 14 crossings inside the 8 columns


# ------------------------------------------------------------------------------------------------ C-ABI
def test_poly_crossings_rejects_bad_arguments_before_any_launch():
    """the argument checks of pd_poly_crossings_i32 come before the launch, so they answer without a device"""
    import ctypes
    from partdistillation_amd import lib
    L = lib.load()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p).value
    good = dict(n=2, h=33, w=70)
    bad = {"negative n": dict(n=-1), "h 0": dict(h=0), "w 0": dict(w=0), "h negative": dict(h=-3), "h too large": dict(h=65536),
           "w too large": dict(w=65536), "h * w over int32": dict(h=65535, w=65535)}
    for what, change in bad.items():
        a = dict(good, **change)
        rc = L.pd_poly_crossings_i32(ptr, ptr, a["n"], a["h"], a["w"], ptr, ptr, None)
        assert rc == -1 and "pd_poly_crossings_i32: bad sizes" in L.pd_last_error().decode(), what
        with pytest.raises(lib.PdHipError, match="bad sizes"):
            lib.check(rc)
    names = ["xy", "vert_offsets", "table_offsets", "starts"]
    for missing in names:                                                  # never dereferenced: the call returns before any launch
        v = {k: (None if k == missing else ptr) for k in names}
        rc = L.pd_poly_crossings_i32(v["xy"], v["vert_offsets"], 2, 33, 70, v["table_offsets"], v["starts"], None)
        assert rc == -1 and "null pointer" in L.pd_last_error().decode(), missing
    assert L.pd_poly_crossings_i32(None, None, 0, 33, 70, None, None, None) == 0                 # nothing to do
    assert L.pd_poly_crossings_i32(None, None, 0, 0, 70, None, None, None) == -1                 # the sizes are checked first
    res, args = lib.SIGNATURES["pd_poly_crossings_i32"]
    assert res is ctypes.c_int and len(args) == 8 and args[2:5] == [ctypes.c_int] * 3
    fn = L.pd_cmd_fn_index(b"pd_poly_crossings_i32")
    assert fn >= 0 and L.pd_cmd_fn_nargs(fn) == 8


# ------------------------------------------------------------------------------------------------ config surface, host decisions
def _cfg(extra):
    from partdistillation_amd.config import setup_cfg
    return setup_cfg(os.path.join(CONFIGS, "proposal_learning/r50_mask2former.yaml"), ["MODEL.DEVICE", "cpu"] + list(extra))


def _record(**extra):
    rec = {"file_name": "data/val/n0123_456.JPEG", "image_id": 9, "height": 24, "width": 30, "image": np.zeros((24, 30, 3), np.uint8),
           "annotations": [{"category_id": 2, "bbox": [0, 0, 1, 1], "bbox_mode": 1, "segmentation": [[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]},
                           {"category_id": 1, "iscrowd": 0, "segmentation": [[12.0, 3.0, 20.0, 3.0, 20.0, 15.0, 12.0, 15.0],
                                                                               [22.0, 3.0, 28.0, 3.0, 28.0, 20.0]]}]}
    rec.update(extra)
    return rec


def test_from_config_and_refusals():
    from partdistillation_amd.data import DevicePartImageNetMapper as M
    from partdistillation_amd.data.part_imagenet_mapper import MAPPING_22K
    cfg = _cfg(["INPUT.MIN_SIZE_TRAIN", "(480, 512)", "INPUT.MAX_SIZE_TRAIN", "900", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range",
                "INPUT.MIN_SIZE_TEST", "640", "CUSTOM_DATASETS.USE_MERGED_GT", "False"])
    table = {"n0123": 7}
    for is_train in (True, False):                                         # the TRAIN sizes in both modes
        m = M.from_config(cfg, is_train, class_code_to_class_id=table)
        assert (m.is_train, m.min_size, m.max_size, m.sample_style, m.crop_type) == (is_train, (480, 512), 900, "range", None)
        assert (m.use_merged_gt, m.device.type, m.class_code_to_class_id, m.num_repeats) == (False, "cpu", table, 20)
    assert M.from_config(_cfg([])).use_merged_gt and M.from_config(_cfg([])).class_code_to_class_id == {}
    with pytest.raises(NotImplementedError, match="shapely"):
        M.from_config(_cfg(["INPUT.CROP.ENABLED", "True"]), is_train=True)
    assert M.from_config(_cfg(["INPUT.CROP.ENABLED", "True"]), is_train=False).crop_type is None     # the crop is a train augmentation
    with pytest.raises(NotImplementedError, match="COLOR_AUG_SSD"):
        M.from_config(_cfg(["INPUT.COLOR_AUG_SSD", "True"]), is_train=True)
    assert not os.path.exists(MAPPING_22K)
    with pytest.raises(FileNotFoundError, match="imagenet1k_to_22k_mapping.pkl"):
        M.from_config(_cfg(["DATASETS.TRAIN", "('imagenet_22k_train',)"]), is_train=False, class_code_to_class_id=table)
    assert M.from_config(_cfg(["DATASETS.TRAIN", "('imagenet_1k_train',)"]), class_code_to_class_id=table).class_code_to_class_id == table


def test_path_correction_and_the_input_is_not_modified():
    from partdistillation_amd.data import DevicePartImageNetMapper as M
    from partdistillation_amd.data.part_imagenet_mapper import correct_part_imagenet_path
    assert correct_part_imagenet_path("data/val/n0123_456.JPEG") == ("data/val/n0123/n0123_456.JPEG", "n0123")
    assert correct_part_imagenet_path("data/val/n0123_456.JPEG") == P.correct_path("data/val/n0123_456.JPEG")
    rec = _record()
    before = copy.deepcopy(rec)
    with pytest.raises(RuntimeError, match="GPU only"):                    # no CPU fallback; everything before the upload is host work
        M(False, (32,), 100, device="cpu", class_code_to_class_id={"n0123": 7})(rec)
    assert rec["file_name"] == before["file_name"] and "class_code" not in rec and rec["annotations"] == before["annotations"]
    with pytest.raises(KeyError, match="n0123"):
        M(False, (32,), 100, device="cpu")(rec)


def test_records_without_parts_and_bad_polygons():
    from partdistillation_amd.data import DevicePartImageNetMapper as M
    table = {"n0123": 7}
    crowd = _record()
    for a in crowd["annotations"]:
        a["iscrowd"] = 1
    for rec in (_record(annotations=[]), crowd):
        assert M(False, (32,), 100, device="cpu", class_code_to_class_id=table)(rec) is None            # as the reference does
        with pytest.raises(ValueError, match="n0123/n0123_456.JPEG"):                                     # the reference crashes here
            M(True, (32,), 100, device="cpu", class_code_to_class_id=table)(rec)
    for seg, what in (([[1.0, 1.0, 9.0, 1.0, 9.0]], "from 5 coordinates"), ([[1.0, 1.0, 9.0, 1.0]], "from 4 coordinates")):
        rec = _record()
        rec["annotations"][0]["segmentation"] = seg
        with pytest.raises(ValueError, match=what):
            M(False, (32,), 100, device="cpu", class_code_to_class_id=table)(rec)
    rec = _record()
    rec["annotations"][0]["segmentation"] = {"size": [24, 30], "counts": [720]}
    with pytest.raises(ValueError, match="lists of polygons"):
        M(False, (32,), 100, device="cpu", class_code_to_class_id=table)(rec)


def test_plan_boxes_filter_and_group_table():
    """the host half of an attempt against the oracle chain: vertices, float32 boxes, survivors; then the group table"""
    from partdistillation_amd.data import DevicePartImageNetMapper as M
    rec = _record()
    rec["annotations"].append({"category_id": 2, "segmentation": [[4.0, 5.0, 4.0, 11.0, 4.0, 20.0]]})       # collinear: an empty box
    m = M(True, (32,), 100, device="cpu", class_code_to_class_id={"n0123": 7})
    parsed = m.parse(rec)
    assert parsed["part_cls"].tolist() == [2, 1, 2] and [len(p) for p in parsed["part_polys"]] == [1, 2, 1]
    for flip in (False, True):
        p = {"in_h": 24, "in_w": 30, "resize": (32, 40), "flip": flip, "crop": (0, 0, 40, 32)}
        parts, boxes, ok = m.plan(parsed, p)
        assert ok.tolist() == [True, True, False] and boxes.dtype == np.float32
        for a, mine in zip(rec["annotations"], parts):
            for q, got in zip(a["segmentation"], mine):
                assert got.dtype == np.float64 and np.array_equal(got, P.transform_polygon(q, p))
        want = P.forward(rec, rec["image"], p, False, {"n0123": 7})
        assert np.array_equal(boxes[ok], want["part_boxes"]) and want["part_classes"] == [2, 1]
    off, mem, cls = M.group_table(np.asarray([2, 1, 2]), [0, 1, 1, 2, 2, 2], merged=True)
    assert off.dtype == np.int32 and mem.dtype == np.int32 and cls.dtype == np.int64
    assert [mem[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [[0, 1, 2, 3, 4, 5], [1, 2], [0, 3, 4, 5]] and cls.tolist() == [1, 2]
    off, mem, cls = M.group_table(np.asarray([2, 1, 2]), [0, 1, 1, 2, 2, 2], merged=False)
    assert [mem[a:b].tolist() for a, b in zip(off[:-1], off[1:])] == [[0, 1, 2, 3, 4, 5], [0], [1, 2], [3, 4, 5]] and cls.tolist() == [2, 1, 2]
    for merged in (True, False):
        off, mem, cls = M.group_table(np.zeros(0, dtype=np.int64), [], merged)
        assert off.tolist() == [0, 0] and len(mem) == 0 and len(cls) == 0                                 # the object plane alone, empty


def test_draws_are_the_resize_and_the_flip_only():
    from partdistillation_amd.data import DevicePartImageNetMapper as M
    for is_train in (True, False):
        mine, theirs = np.random.RandomState(3), np.random.RandomState(3)
        m = M(is_train, (32, 40, 48), 60, "choice", device="cpu", rng=mine)
        for _ in range(8):
            assert m.draw(40, 56) == P.draw(theirs, 40, 56, (32, 40, 48), 60, "choice", is_train)
        assert mine.get_state()[2] == theirs.get_state()[2] and np.array_equal(mine.get_state()[1], theirs.get_state()[1])
    assert M.identity(40, 56) == P.identity_params(40, 56)
