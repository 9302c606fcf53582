"""Dense-CRF refinement without a GPU: the fp64 oracle (dcrf_oracle.py) against properties it must have, the cap on near-tie pixels the
GPU tests rely on, the wrapper's argument checks and refine_proposals with the oracle in place of the device mean field."""
import numpy as np
import pytest
import torch

import dcrf_oracle as O


def test_oracle_columns_sum_to_one_and_t0_returns_the_ranks():
    c = O.case("c")
    for q in c["q"].values():
        assert q.shape == (16, 28, 40) and np.abs(q.sum(0) - 1.0).max() < 1e-12 and (q >= 0).all()
    out, q0, _ = O.mean_field(c["image"], c["labels"], 16, t=0)
    values, ranks = O.rank_map(c["labels"])
    assert out.dtype == np.uint8 and np.array_equal(out, ranks)
    assert 5 not in values and c["labels"].max() > ranks.max()                  # the absent value shifts the larger ones down
    assert np.allclose(q0[ranks, np.arange(28)[:, None], np.arange(40)[None, :]], 0.7, atol=1e-12)


def test_oracle_without_pairwise_terms_stays_at_q0():
    image, labels = O.make_inputs(12, 14, 4, 3)
    _, q0, _ = O.mean_field(image, labels, 4, t=0)
    out, q, _ = O.mean_field(image, labels, 4, t=3, compat1=0, compat2=0)
    assert np.abs(q - q0).max() < 1e-15 and np.array_equal(out, O.rank_map(labels)[1])


def test_oracle_normalisers_on_a_constant_image_are_the_box_sums():
    H, W, sd1, sd2 = 11, 15, 1.5, 3.0
    image = np.full((H, W, 3), 77, dtype=np.uint8)
    k1, k2 = O.kernels(image, sd1, sd2, 13)
    for k, sd in ((k1, sd1), (k2, sd2)):
        R = O.radius(sd)
        e = np.exp(-np.arange(-R, R + 1) ** 2 / (2.0 * sd * sd))
        def row_sum(pos, size):
            d = np.arange(-R, R + 1)
            return e[(pos + d >= 0) & (pos + d < size)].sum()
        want = np.array([[1.0 / np.sqrt(row_sum(x, W) * row_sum(y, H) + 1e-20) for x in range(W)] for y in range(H)])
        assert np.abs(O.normalisers(k).reshape(H, W) - want).max() < 1e-12
    out, q, _ = O.mean_field(image, np.full((H, W), 9), 2, t=2, sd1=sd1, sd2=sd2)    # one label: rank 0 everywhere
    assert (out == 0).all() and (q[0] > 0.7).all()


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_oracle_near_ties_stay_under_the_cap(name):
    """the GPU tests compare labels only where the oracle's top-two margin is at least MARGIN: those are at least 99 % of the pixels"""
    c = O.case(name)
    for step, q in c["q"].items():
        share = float((O.margins(q) < O.MARGIN).mean())
        print(f"case {name} t={step}: {share:.4%} of the pixels have a margin below {O.MARGIN}")
        assert share <= O.MARGIN_SHARE, (name, step, share)
    assert np.array_equal(c["labels10"], c["q"][10].argmax(0))
    assert len(np.unique(c["labels"])) <= c["L"]


def test_dense_crf_checks_its_arguments():
    from partdistillation_amd.functions.dense_crf import dense_crf
    image, labels = (torch.from_numpy(a) for a in O.make_inputs(8, 8, 3, 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        dense_crf(image, labels, 3)
    with pytest.raises(ValueError, match="n_labels"):
        dense_crf(image, labels, 1)
    with pytest.raises(ValueError, match="n_labels"):
        dense_crf(image, labels, 17)
    many = torch.arange(64).reshape(8, 8) % 5
    with pytest.raises(ValueError, match="5 distinct"):
        dense_crf(image, many, 4)


def _data(masks, key):
    from partdistillation_amd.utils import rle
    return {"file_name": "n01440764_1.pth", "class_code": "n01440764", key: rle.masks_to_coco_json(masks), "height": 16, "width": 16}


def test_refine_proposals_with_the_oracle_in_place_of_the_device(monkeypatch):
    import partdistillation_amd.postprocess_dcrf as P
    from partdistillation_amd.utils import rle
    S = 16
    calls = []

    def oracle_crf(image, labels, n_labels, **kw):
        calls.append((tuple(image.shape), int(n_labels), dict(kw)))
        out, _, _ = O.mean_field(image.numpy(), labels.numpy(), n_labels, **dict(O.DEFAULTS, **kw))
        return torch.from_numpy(out)

    monkeypatch.setattr(P._dcrf, "dense_crf", oracle_crf)
    monkeypatch.setattr(P, "resize_image", lambda image, size, device: torch.as_tensor(image))     # the image path itself needs the GPU
    # background (columns 0-3, no mask), two parts, and a third part of ONE pixel inside the first that the mean field removes
    masks = np.zeros((3, S, S), dtype=bool)
    masks[0, :, 4:10], masks[1, :, 10:] = True, True
    masks[0, 5, 6], masks[2, 5, 6] = False, True
    image = np.zeros((S, S, 3), dtype=np.uint8)
    image[:, :4], image[:, 4:10], image[:, 10:] = (30, 200, 30), (200, 30, 30), (30, 30, 200)
    want_labels, _, _ = O.mean_field(image, (masks * np.arange(1, 4)[:, None, None]).sum(0), 4, **dict(O.DEFAULTS, sd2=4))
    assert set(np.unique(want_labels)) == {0, 1, 2}                             # the third part is dropped
    for key in ("part_masks", "part_mask"):
        data = _data(masks, key)
        out = P.refine_proposals(data, image, size=S, device="cpu", sd2=4)
        assert out is data and set(out) == set(_data(masks, key))               # written back under the key found, nothing else touched
        got = np.stack([rle.decode(m["segmentation"]) for m in out[key]])
        assert got.shape == (2, S, S) and all(isinstance(m["segmentation"]["counts"], str) for m in out[key])
        assert np.array_equal(got[0], want_labels == 1) and np.array_equal(got[1], want_labels == 2)
        assert got[0, 5, 6] and got[0].sum() == 6 * S
    assert calls == [((S, S, 3), 4, {"sd2": 4})] * 2
    # pass-through: None, empty, no mask key at all
    for data in ({"part_masks": None, "file_name": "x"}, {"part_mask": [], "file_name": "x"}, {"file_name": "x"}):
        before = dict(data)
        assert P.refine_proposals(data, image, size=S, device="cpu") is data and data == before
    assert len(calls) == 2
    with pytest.raises(ValueError, match="do not match"):
        P.refine_proposals(_data(masks[:, :8], "part_masks"), image, size=S, device="cpu")
