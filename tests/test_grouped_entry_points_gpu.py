"""The host path that the eight grouped evaluation entry points share (include/pd_eval.h, pd_grouping.h, pd_assign.h), called through
the C ABI with one tiny descriptor each: an empty list, null tables, one field out of range and (where legal) an empty set are answered
on the host and launch nothing; the valid descriptor runs one workgroup.  Every output starts at FILL; the counters accumulate on it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PD_ERR_INVALID_ARG = -1
FILL = 7
MAX_K_GROUPING, MAX_K_ASSIGN, MAX_KEYS, MAX_GT, MAX_ROWS = 32, 256, 1024, 64, 200        # include/*.h


def _full(shape, dtype):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype, device="cuda")


def _pack():
    from partdistillation_amd.functions import eval_metrics as E
    masks = torch.ones((2, 16), dtype=torch.uint8, device="cuda")
    bits, area = _full((2, 1), torch.int64), _full((2,), torch.int64)
    fields = dict(masks=masks.data_ptr(), bits=bits.data_ptr(), area=area.data_ptr(), n=2, hw=16)
    return (E.PdEvalMaskSet, fields, (), [(bits, [[0xFFFF], [0xFFFF]]), (area, [FILL + 16] * 2)], dict(hw=0),
            dict(n=0, masks=None, bits=None, area=None), [masks])


def _intersect():
    from partdistillation_amd.functions import eval_metrics as E
    a, b = _dev([[0xFFFF], [0x00FF]], torch.int64), _dev([[0x000F], [0xFF00]], torch.int64)
    inter = _full((2, 2), torch.int64)
    fields = dict(a=a.data_ptr(), rows=None, b=b.data_ptr(), inter=inter.data_ptr(), p=2, g=2, words=1)
    return E.PdEvalPairs, fields, (), [(inter, [[FILL + 4, FILL + 8], [FILL + 4, FILL]])], dict(g=MAX_GT + 1), None, [a, b]


def _confusion():
    from partdistillation_amd.functions import eval_metrics as E
    planes, cls, slot = _dev([[0x00FF], [0xFF00]], torch.int64), _dev([0, 1], torch.int64), _dev([0], torch.int64)
    conf = _full((1, 3, 3), torch.int64)
    fields = dict(pred_bits=planes.data_ptr(), pred_cls=cls.data_ptr(), gt_bits=planes.data_ptr(), gt_cls=cls.data_ptr(),
                  slot=slot.data_ptr(), pred_n=2, gt_n=2, hw=16)
    want = [[[FILL + 8, FILL, FILL], [FILL, FILL + 8, FILL], [FILL, FILL, FILL]]]
    return E.PdEvalConfusion, fields, (2, conf.data_ptr(), 1), [(conf, want)], dict(hw=0), None, [planes, cls, slot]


def _recall():
    from partdistillation_amd.functions import eval_metrics as E
    inter, area = _dev([[4, 0], [0, 4]], torch.int64), _dev([4, 4], torch.int64)
    thr = E.thresholds("cuda")
    hits, num_pos = _full((5, 10), torch.int64), _full((5,), torch.int64)
    fields = dict(inter=inter.data_ptr(), rows=None, area_p=area.data_ptr(), area_g=area.data_ptr(), p=2, g=2)
    want = [[FILL + 1] * 10] + [[FILL + 2] * 10] * 4                           # both IoUs are 1: AR@1 takes one, the other limits both
    return (E.PdEvalRecall, fields, (thr.data_ptr(), hits.data_ptr(), num_pos.data_ptr()), [(hits, want), (num_pos, [FILL + 2] * 5)],
            dict(p=MAX_ROWS + 1), None, [inter, area, thr])


def _labels():
    from partdistillation_amd.functions import pixel_grouping as G
    scores = torch.stack((torch.zeros((4, 4)), torch.ones((4, 4)))).cuda()
    mask = torch.ones((8, 8), dtype=torch.uint8, device="cuda")
    labels, counts = _full((8, 8), torch.uint8), _full((3,), torch.int32)
    fields = dict(scores=scores.data_ptr(), mask=mask.data_ptr(), labels=labels.data_ptr(), counts=counts.data_ptr(), K=2, h=4, w=4,
                  Hp=8, Wp=8, Hi=6, Wi=6, H=8, W=8)
    return (G.PdGroupLabels, fields, (), [(labels, [[2] * 8] * 8), (counts, [FILL, FILL, FILL + 64])], dict(K=MAX_K_GROUPING + 1), None,
            [scores, mask])


def _resize():
    from partdistillation_amd.functions import pixel_grouping as G
    src = torch.ones((2, 4, 4), dtype=torch.uint8, device="cuda")
    dst, area = _full((2, 8, 8), torch.uint8), _full((2,), torch.int64)
    fields = dict(src=src.data_ptr(), dst=dst.data_ptr(), area=area.data_ptr(), n=2, Hp=4, Wp=4, Hi=4, Wi=4, H=8, W=8)
    return (G.PdMaskResize, fields, (), [(dst, [[[1] * 8] * 8] * 2), (area, [FILL + 64] * 2)], dict(Hi=5),
            dict(n=0, src=None, dst=None, area=None), [src])


def _assign():
    from partdistillation_amd.functions import mask_assign as A
    logits = torch.stack((-torch.ones((4, 4)), torch.ones((4, 4)))).cuda()
    scores = torch.ones(2, device="cuda")
    arg, obj, positive = _full((8, 8), torch.int16), _full((8, 8), torch.uint8), _full((2,), torch.int32)
    fields = dict(logits=logits.data_ptr(), scores=scores.data_ptr(), object=None, cls_of_query=None, arg=arg.data_ptr(), obj=obj.data_ptr(),
                  positive=positive.data_ptr(), cls=None, K=2, h=4, w=4, Hp=8, Wp=8, Hi=6, Wi=6, H=8, W=8)
    return (A.PdAssignResized, fields, (), [(arg, [[1] * 8] * 8), (obj, [[1] * 8] * 8), (positive, [FILL, FILL + 64])],
            dict(K=MAX_K_ASSIGN + 1), None, [logits, scores])


def _histogram():
    from partdistillation_amd.functions import mask_assign as A
    key = _dev([0] * 32 + [1] * 32, torch.int16)
    obj = torch.ones(64, dtype=torch.uint8, device="cuda")
    gt = torch.stack((torch.ones(64), torch.zeros(64))).to(torch.uint8).cuda()
    won, area, inter, gt_area = _full((2,), torch.int64), _full((2,), torch.int64), _full((2, 2), torch.int64), _full((2,), torch.int64)
    fields = dict(key=key.data_ptr(), obj=obj.data_ptr(), gt=gt.data_ptr(), won=won.data_ptr(), area=area.data_ptr(), inter=inter.data_ptr(),
                  gt_area=gt_area.data_ptr(), n=2, G=2, hw=64)
    want = [(won, [FILL + 32] * 2), (area, [FILL + 32] * 2), (inter, [[FILL + 32, FILL]] * 2), (gt_area, [FILL + 64, FILL])]
    return A.PdAssignHistogram, fields, (), want, dict(n=MAX_KEYS + 1), None, [key, obj, gt]


ENTRY_POINTS = {
    "pd_eval_pack_grouped": _pack, "pd_eval_intersect_grouped": _intersect, "pd_eval_confusion_grouped": _confusion,
    "pd_eval_recall_grouped": _recall, "pd_scores_argmax_resized_u8": _labels, "pd_masks_resize_u8": _resize,
    "pd_mask_assign_resized": _assign, "pd_assign_histogram": _histogram,
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_point_answers_on_the_host_and_launches_only_valid_work(name):
    from partdistillation_amd import lib
    so = lib.load()
    struct, fields, extra, outputs, bad, empty, keep = ENTRY_POINTS[name]()
    pinned = torch.empty(4096, dtype=torch.uint8).pin_memory()
    table = _full((4096,), torch.uint8)
    st = lib.current_stream()

    def call(count=1, pinned_=pinned.data_ptr(), table_=table.data_ptr(), no_list=False, **over):
        arr = (struct * 1)()
        for k, v in {**fields, **over}.items():
            setattr(arr[0], k, v)
        return getattr(so, name)(None if no_list else arr, count, *extra, pinned_, table_, st)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in [table] + [t for t, _ in outputs])

    assert call(count=0) == 0 and untouched()
    for what, kw in (("list", dict(no_list=True)), ("pinned table", dict(pinned_=None)), ("device table", dict(table_=None)),
                     (f"{bad}", bad)):
        assert call(**kw) == PD_ERR_INVALID_ARG, what
        message = so.pd_last_error().decode()
        assert message.startswith(name + ":"), (what, message)
        assert untouched(), what
    if empty is not None:                                                      # an empty set without data pointers is legal and launches nothing
        assert call(**empty) == 0 and untouched()
    assert call() == 0
    torch.cuda.synchronize()
    for t, want in outputs:
        assert torch.equal(t.cpu(), torch.tensor(want, dtype=t.dtype).reshape(t.shape)), (name, t)
