"""The launchers of include/pd_input.h (partdistillation_amd/functions/input_pipeline.py) on their own, at shapes a hand can check:
`resample_u8` — a window of a resize on a padded canvas, both layouts, the source-side crop and flip, the flip by reversed tables, an
identity axis, an empty window — and `rle_sample`, against the Pillow restatement oracle/input_pipeline_ref.py.  Exact equality."""
import functools

import numpy as np
import pytest
import torch

from oracle import input_pipeline_ref as R

pytestmark = pytest.mark.gpu

H, W, RH, RW = 11, 17, 7, 23                     # rows 11 -> 7: downscale, ksize 5; columns 17 -> 23: upscale, ksize 3
Y0, Y1, X0, X1 = 2, 6, 5, 14                     # the window of the resize that survives
CANVAS, PAD = (8, 12), 128


@functools.lru_cache(maxsize=None)
def _scene():
    """(big uint8 [13, 21, 3], src = its mirrored crop [11, 17, 3], the oracle's full resize of src [7, 23, 3]); read-only"""
    big = np.random.RandomState(7).randint(0, 256, (H + 2, W + 3 + 1, 3)).astype(np.uint8)
    src = np.ascontiguousarray(big[:, ::-1][2:2 + H, 3:3 + W])
    full = R.resize_bilinear_u8(src, RH, RW)
    for a in (big, src, full):
        a.setflags(write=False)
    return big, src, full


def _tables(flip_tables=False):
    from partdistillation_amd.functions.input_pipeline import resample_coeffs
    xtab = resample_coeffs(W, RW, RW - X1 if flip_tables else X0, X1 - X0)
    if flip_tables:
        xtab = tuple(t[::-1] for t in xtab)
    ytab = resample_coeffs(H, RH, Y0, Y1 - Y0)
    assert xtab[2].shape == (X1 - X0, 3) and ytab[2].shape == (Y1 - Y0, 5)
    return xtab, ytab


def _on_canvas(window, planar):
    want = np.full(CANVAS + (3,), PAD, np.uint8)
    want[:window.shape[0], :window.shape[1]] = window
    return want.transpose(2, 0, 1) if planar else want


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("planar", [True, False])
def test_window_of_a_resize_on_a_padded_canvas(planar):
    from partdistillation_amd.functions.input_pipeline import resample_u8
    _, src, full = _scene()
    got = resample_u8(_dev(src), *_tables(), CANVAS, pad_value=PAD, planar=planar)
    assert got.dtype == torch.uint8 and tuple(got.shape) == ((3,) + CANVAS if planar else CANVAS + (3,))
    assert np.array_equal(got.cpu().numpy(), _on_canvas(full[Y0:Y1, X0:X1], planar))


@pytest.mark.parametrize("planar", [True, False])
def test_source_side_crop_and_flip_through_the_kernels_flag(planar):
    from partdistillation_amd.functions.input_pipeline import resample_u8
    big, _, full = _scene()                                                # src IS big[:, ::-1][2:13, 3:20]
    got = resample_u8(_dev(big), *_tables(), CANVAS, row0=2, x0=3, flip=True, pad_value=PAD, planar=planar)
    assert np.array_equal(got.cpu().numpy(), _on_canvas(full[Y0:Y1, X0:X1], planar))


@pytest.mark.parametrize("planar", [True, False])
def test_flip_by_reversed_column_tables(planar):
    from partdistillation_amd.functions.input_pipeline import resample_u8
    _, src, full = _scene()
    got = resample_u8(_dev(src), *_tables(flip_tables=True), CANVAS, pad_value=PAD, planar=planar)
    assert np.array_equal(got.cpu().numpy(), _on_canvas(full[:, ::-1][Y0:Y1, X0:X1], planar))


@pytest.mark.parametrize("oh,ow", [(H, 9), (RH, W)])
def test_identity_axis(oh, ow):
    """resample_coeffs' identity branch (ksize 1) in one axis, a real resize in the other; the canvas defaults to the window"""
    from partdistillation_amd.functions.input_pipeline import resample_coeffs, resample_u8
    _, src, _ = _scene()
    xtab, ytab = resample_coeffs(W, ow, 0, ow), resample_coeffs(H, oh, 0, oh)
    assert (xtab[2].shape[1] == 1) != (ytab[2].shape[1] == 1)
    got = resample_u8(_dev(src), xtab, ytab)
    assert tuple(got.shape) == (3, oh, ow)
    assert np.array_equal(got.cpu().numpy(), R.resize_bilinear_u8(src, oh, ow).transpose(2, 0, 1))


@pytest.mark.parametrize("planar", [True, False])
def test_empty_window_is_a_canvas_of_pad_value(planar):
    from partdistillation_amd.functions.input_pipeline import resample_coeffs, resample_u8
    _, src, _ = _scene()
    got = resample_u8(_dev(src), _tables()[0], resample_coeffs(H, RH, Y0, 0), CANVAS, pad_value=PAD, planar=planar)
    assert tuple(got.shape) == ((3,) + CANVAS if planar else CANVAS + (3,)) and bool((got == PAD).all())


def test_rle_sample_without_masks_launches_nothing():
    from partdistillation_amd.functions.input_pipeline import rle_sample
    masks, area = rle_sample(None, torch.zeros(1, dtype=torch.int32, device="cuda"), 9, 7, False, None, None, 8)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (0, 8, 8) and area.dtype == torch.int32 and tuple(area.shape) == (0,)
    assert masks.is_cuda and area.is_cuda


@pytest.mark.parametrize("flip", [False, True])
def test_rle_sample_against_the_nearest_resize_of_the_decoded_masks(flip):
    from partdistillation_amd.functions.input_pipeline import nearest_index, rle_sample, upload_tables
    from partdistillation_amd.utils import rle
    h, w, S = 9, 7, 8
    rng = np.random.RandomState(4)
    masks = np.stack([rng.rand(h, w) < 0.5, rng.rand(h, w) < 0.2, np.ones((h, w), bool)])
    masks[0, 0, 0] = True                                                  # starts with ones: COCO's leading zero-length run
    starts, offsets = rle.segmentations_to_starts([rle.encode(m) for m in masks], (h, w))
    d = upload_tables((starts, offsets, nearest_index(w, S), nearest_index(h, S)), "cuda")
    got, area = rle_sample(d[0], d[1], h, w, flip, d[2], d[3], S)
    want = np.stack([R.resize_nearest(m[:, ::-1] if flip else m, S, S) for m in masks])
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    assert area.dtype == torch.int32 and area.cpu().tolist() == want.reshape(3, -1).sum(1).tolist()
