"""Dense-CRF refinement on the device (include/pd_dcrf.h) against the fp64 brute-force oracle of dcrf_oracle.py.

  case  H x W     L   sd1 / sd2 / sc   what it reaches
  a     20 x 24   5   3 / 20 / 13      the defaults: a window larger than the image, every border
  b     37 x 70   3   1 / 4 / 13       several tiles both ways, ragged edge tiles, interior pixels with a full window (R2 = 12)
  c     28 x 40   16  1 / 2 / 30       the widest L class; an absent label value, which gives the rank shift
  d     33 x 17   2   2 / 6 / 5        the narrowest L class; an image narrower than one tile
  e     9 x 130   8   1 / 3 / 13       the middle L class; fewer rows than a strip

Q_TOL is 4 x the largest |Q - oracle| measured on an MI355X over the ten runs below (each case at t = 1 and t = 10): 8.793e-07, in case c
at t = 10 (per case, t = 1 / t = 10: a 2.04e-07 / 2.30e-07, b 3.15e-07 / 1.50e-07, c 7.52e-07 / 8.79e-07, d 1.97e-07 / 5.95e-08,
e 3.73e-07 / 4.11e-07; also in DESIGN.md section 7e).  The margin covers fp32 summation order and the hardware exp; the tolerance may never
exceed 1e-3."""
import numpy as np
import pytest
import torch

import dcrf_oracle as O

pytestmark = pytest.mark.gpu

Q_TOL = 3.5e-6
assert Q_TOL <= 1e-3
PD_ERR_INVALID_ARG = -1


def _dev(c):
    return torch.from_numpy(c["image"]).cuda(), torch.from_numpy(c["labels"]).cuda()


def _run(name, t, **kw):
    from partdistillation_amd.functions.dense_crf import dense_crf
    c = O.case(name)
    image, labels = _dev(c)
    return dense_crf(image, labels, c["L"], **dict(c["params"], t=t, **kw))


@pytest.mark.parametrize("t", [1, 10])
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_q_and_labels_match_the_oracle(name, t):
    c = O.case(name)
    out, q = _run(name, t, return_q=True)
    want = c["q"][t]
    assert q.dtype == torch.float32 and tuple(q.shape) == want.shape and out.dtype == torch.uint8 and tuple(out.shape) == want.shape[1:]
    q, out = q.cpu().numpy().astype(np.float64), out.cpu().numpy()
    err = float(np.abs(q - want).max())
    sure = O.margins(want) >= O.MARGIN
    print(f"case {name} t={t}: max |Q - oracle| = {err:.3e}, {int((~sure).sum())} of {sure.size} pixels below the margin")
    assert err <= Q_TOL, (name, t, err)
    assert np.array_equal(out, q.argmax(0))                                     # the first maximum of the device's own Q
    assert sure.mean() >= 1.0 - O.MARGIN_SHARE
    assert np.array_equal(out[sure], want.argmax(0)[sure])
    assert np.array_equal(_run(name, t).cpu().numpy(), out)                     # without return_q: the same map


def test_t0_and_no_pairwise_terms_return_the_rank_map():
    for name in ("a", "c"):
        c = O.case(name)
        out = _run(name, 0)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), c["ranks"])
        out0, q0 = _run(name, 0, return_q=True)
        assert np.array_equal(out0.cpu().numpy(), c["ranks"])
        own = q0.cpu().numpy()[c["ranks"], np.arange(q0.shape[1])[:, None], np.arange(q0.shape[2])[None, :]]
        assert np.abs(own - 0.7).max() < 1e-6 and np.abs(q0.sum(0).cpu().numpy() - 1).max() < 1e-6
        flat = _run(name, 10, compat1=0, compat2=0)
        assert np.array_equal(flat.cpu().numpy(), c["ranks"])
    assert O.case("c")["labels"].max() > O.case("c")["ranks"].max()             # case c's ranks are not its label values


def test_runs_are_bit_identical_also_on_another_stream():
    for name in ("b", "c"):
        out, q = _run(name, 10, return_q=True)
        out2, q2 = _run(name, 10, return_q=True)
        assert torch.equal(out, out2) and torch.equal(q.view(torch.int32), q2.view(torch.int32))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out3, q3 = _run(name, 10, return_q=True)
        side.synchronize()
        assert torch.equal(out, out3) and torch.equal(q.view(torch.int32), q3.view(torch.int32))


def test_capi_rejects_bad_arguments_and_launches_nothing():
    from partdistillation_amd import lib
    so = lib.load()
    H, W, L = 6, 7, 3
    image = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    lab = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    rgb = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    n1, n2 = (torch.full((H, W), 7.0, device="cuda") for _ in range(2))
    q, q2, tmp, msg = (torch.full((16, H, W), 7.0, device="cuda") for _ in range(4))
    out = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
    st = lib.current_stream()
    P = lambda t: t.data_ptr()  # noqa: E731

    def prepare(image=P(image), H=H, W=W, L=L, n2=P(n2)):
        return so.pd_dcrf_prepare(image, P(lab), H, W, L, 0.7, 3.0, 20.0, 13.0, P(rgb), P(n1), n2, P(q), st)

    def spatial(q_=P(q), H=H, L=L):
        return so.pd_dcrf_spatial_message(q_, P(n1), H, W, L, 3.0, 3.0, P(tmp), P(msg), st)

    def update(msg_=P(msg), H=H, L=L, q_next=P(q2)):
        return so.pd_dcrf_bilateral_update(P(rgb), P(lab), P(n2), P(q), msg_, H, W, L, 0.7, 20.0, 13.0, 10.0, q_next, st)

    def argmax(out_=P(out), H=H, L=L):
        return so.pd_dcrf_argmax(P(q), H, W, L, out_, st)

    bad = [("null", lambda: prepare(image=None)), ("null", lambda: prepare(n2=None)), ("L=1", lambda: prepare(L=1)),
           ("L=17", lambda: prepare(L=17)), ("H=0", lambda: prepare(H=0)),
           ("null", lambda: spatial(q_=None)), ("L=1", lambda: spatial(L=1)), ("L=17", lambda: spatial(L=17)), ("H=0", lambda: spatial(H=0)),
           ("null", lambda: update(msg_=None)), ("L=1", lambda: update(L=1)), ("L=17", lambda: update(L=17)), ("H=0", lambda: update(H=0)),
           ("aliases", lambda: update(q_next=P(q))),
           ("null", lambda: argmax(out_=None)), ("L=1", lambda: argmax(L=1)), ("L=17", lambda: argmax(L=17)), ("H=0", lambda: argmax(H=0))]
    for word, call in bad:
        assert call() == PD_ERR_INVALID_ARG, word
        message = so.pd_last_error().decode()
        assert message.startswith("pd_dcrf_") and word in message, (word, message)
    torch.cuda.synchronize()
    for t in (rgb, n1, n2, q, q2, tmp, msg, out):                               # nothing was launched: every output still holds its fill
        assert bool((t == 7).all())
    assert prepare() == 0 and spatial() == 0 and update() == 0 and argmax() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and float((q2[:L].sum(0) - 1).abs().max()) < 1e-5


def test_refine_proposals_end_to_end():
    """48 x 64 image, three masks that do not overlap, at size 64 with sd2 = 4 (the product runs at 640 with the defaults)"""
    import partdistillation_amd.postprocess_dcrf as P
    from partdistillation_amd.utils import rle
    S, rng = 64, np.random.RandomState(5)
    lab = np.zeros((S, S), dtype=np.int64)
    lab[4:44, 2:22], lab[6:30, 24:44], lab[10:46, 46:62] = 1, 2, 3
    lab[30:48, 24:44] = 0
    lab[48:] = 0                                                                 # the rows the padding fills
    flip = (rng.rand(S, S) < 0.05) & (np.arange(S)[:, None] < 48)
    noisy = np.where(flip, rng.randint(0, 4, size=(S, S)), lab)
    base = np.array([(60, 60, 60), (210, 50, 50), (50, 200, 60), (40, 70, 220)])
    image = np.clip(base[lab[:48]] + rng.randint(-25, 26, size=(48, S, 3)), 0, 255).astype(np.uint8)
    masks = np.stack([noisy == c for c in (1, 2, 3)])
    data = {"file_name": "x.pth", "part_mask": rle.masks_to_coco_json(masks)}
    out = P.refine_proposals(data, image, size=S, sd2=4)
    resized = P.resize_image(image, S).cpu().numpy()
    assert resized.shape == (S, S, 3) and np.array_equal(resized[:48], image) and (resized[48:] == 128).all()
    want, q, _ = O.mean_field(resized, noisy, 4, **dict(O.DEFAULTS, sd2=4))
    present = [c for c in np.unique(want) if c != 0]
    assert present == [1, 2, 3] and len(out["part_mask"]) == 3 and "part_masks" not in out
    got = sum(rle.decode(m["segmentation"]).astype(np.int64) * c for m, c in zip(out["part_mask"], present))
    sure = O.margins(q) >= O.MARGIN
    print(f"refine_proposals: {int((~sure).sum())} of {sure.size} pixels below the margin, {int((got != want).sum())} labels differ")
    assert sure.mean() >= 1.0 - O.MARGIN_SHARE and np.array_equal(got[sure], want[sure])
    assert (got != noisy).sum() > 0                                              # the mean field changed something
