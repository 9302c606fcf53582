"""pd_pair_assign_resized (include/pd_assign.h): K (query, class) pairs over Q shared logit maps.  Its contract is bit-equality with
pd_mask_assign_resized on the gathered stack logits[pair_query] - arg, obj, positive and cls - which the tests of that kernel
(test_supervised_gpu.py) tie to chained F.interpolate; and the host behaviour of the grouped entry points."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PD_ERR_INVALID_ARG = -1
FILL = 7

# name: (Q, K, h, w, (Hp, Wp), (Hi, Wi), (H, W), object mask, classes)
CASES = {
    "a_identity": (5, 12, 6, 7, (24, 28), (21, 26), (21, 26), "band", True),          # identity size; an empty row band; classes
    "b_two_tiles": (3, 7, 5, 9, (20, 36), (17, 33), (37, 300), "blocks", True),        # two column tiles; 37 rows: not a multiple of 4
    "c_from_memory": (4, 9, 3, 600, (12, 2400), (11, 2390), (6, 256), None, False),    # strong down-scale: the row mix does not fit in LDS
    "d_lds_chunks": (40, 256, 8, 40, (32, 160), (30, 150), (50, 200), "blocks", True),  # ~40 columns: chunks of ~25 of the 40 queries
    "e_smallest": (1, 1, 4, 4, (16, 16), (15, 13), (9, 11), None, False),
}


def _inputs(name, seed):
    Q, K, h, w, pad, crop, out, objkind, with_cls = CASES[name]
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn((Q, h, w), generator=g) * 2).to(DEV)
    pq = torch.randint(0, Q, (K,), generator=g, dtype=torch.int32)
    if K >= 2 and Q >= 2:
        pq[-1] = pq[0]                                                    # at least one query under two pairs, far apart in pair order
    scores = (torch.rand((K,), generator=g) * 0.9 + 0.05).to(DEV)
    H, W = out
    obj = None
    if objkind == "blocks":                                               # whole 256-pixel segments lie outside
        obj = (F.interpolate(torch.rand((1, 1, 3, 4), generator=g), size=(H, W), mode="nearest")[0, 0] > 0.35).to(DEV)
    elif objkind == "band":
        obj = (torch.rand((H, W), generator=g) > 0.2)
        obj[8:13] = False                                                 # rows 8..11 are one workgroup's four segments: none sees the logits
        obj = obj.to(DEV)
    cop = torch.randint(0, 6, (K,), generator=g, dtype=torch.int32).to(DEV) if with_cls else None
    return logits, pq.to(DEV), scores, obj, cop, pad, crop, out


def _assert_equal(got, want, what):
    for name, a, b in zip(("arg", "obj", "positive", "cls"), got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert torch.equal(a, b), (what, name, int((a != b).sum()))


def _gathered(item):
    logits, pq, scores, obj, cop, pad, crop, out = item
    return (logits[pq.long()].contiguous(), scores, obj, cop, pad, crop, out)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bit_equal_to_mask_assign_resized_on_the_gathered_stack(name):
    from partdistillation_amd.functions import mask_assign as A
    item = _inputs(name, 11)
    got, = A.pair_assign_resized([item])
    want, = A.mask_assign_resized([_gathered(item)])
    _assert_equal(got, want, name)
    if CASES[name][7] == "band":                                          # the band took the no-object path: first largest score, no object
        assert bool((got[0][8:12] == int(item[2].argmax())).all()) and not bool(got[1][8:12].any())
    if name == "d_lds_chunks":                                            # every query is referenced: the chunk loop runs twice
        assert int(torch.bincount(item[1].long(), minlength=40).min()) >= 1


def test_equal_scores_take_the_first_pair_in_pair_order():
    """pairs listed in DESCENDING query order, two pairs of one query, all scores equal: the products of the two pairs of a query tie on every
    pixel, and the kernel visits pairs grouped by ascending query - only the explicit rule gives the first maximum in pair order"""
    from partdistillation_amd.functions import mask_assign as A
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn((3, 5, 6), generator=g) * 2).to(DEV)
    pq = torch.tensor([2, 2, 1, 0, 0, 1], dtype=torch.int32, device=DEV)
    scores = torch.full((6,), 0.5, device=DEV)
    cop = torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int32, device=DEV)
    for crop, out in (((18, 22), (29, 41)), ((18, 22), (18, 22))):
        item = (logits, pq, scores, None, cop, (20, 24), crop, out)
        got, = A.pair_assign_resized([item])
        want, = A.mask_assign_resized([_gathered(item)])
        _assert_equal(got, want, out)
        assert set(got[0].unique().tolist()) <= {0, 2, 3}                 # never the second pair of a query
        assert torch.equal(got[2][0], got[2][1]) and torch.equal(got[2][3], got[2][4]) and torch.equal(got[2][2], got[2][5])


def test_one_launch_for_a_batch():
    from partdistillation_amd.functions import mask_assign as A
    items = [_inputs(n, 40 + i) for i, n in enumerate(("a_identity", "b_two_tiles", "e_smallest"))]
    got = A.pair_assign_resized(items)
    want = A.mask_assign_resized([_gathered(it) for it in items])
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_equal(a, b, i)


def test_wrapper_refuses_bad_inputs():
    from partdistillation_amd.functions import mask_assign as A
    lg, pq, sc, obj, cop, pad, crop, out = _inputs("a_identity", 1)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        A.pair_assign_resized([(lg.cpu(), pq, sc, None, None, pad, crop, out)])
    with pytest.raises(ValueError, match="pair_query must be int32"):
        A.pair_assign_resized([(lg, pq.long(), sc, None, None, pad, crop, out)])
    with pytest.raises(ValueError, match="cls_of_pair must be int32"):
        A.pair_assign_resized([(lg, pq, sc, None, cop[:-1], pad, crop, out)])
    with pytest.raises(ValueError, match="not at the output size"):
        A.pair_assign_resized([(lg, pq, sc, obj[:-1], None, pad, crop, out)])
    assert A.pair_assign_resized([]) == []


def test_entry_point_answers_on_the_host_and_launches_only_valid_work():
    """what test_grouped_entry_points_gpu.py checks for its eight entry points"""
    from partdistillation_amd import lib
    from partdistillation_amd.functions import mask_assign as A
    so = lib.load()
    name = "pd_pair_assign_resized"

    def full(shape, dtype):
        return torch.full(shape, FILL, dtype=dtype, device=DEV)

    logits = torch.stack((-torch.ones((4, 4)), torch.ones((4, 4)))).to(DEV)
    scores = torch.ones(3, device=DEV)
    pq = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)
    arg, obj, positive = full((8, 8), torch.int16), full((8, 8), torch.uint8), full((3,), torch.int32)
    fields = dict(logits=logits.data_ptr(), pair_query=pq.data_ptr(), scores=scores.data_ptr(), cls_of_pair=None, object=None,
                  arg=arg.data_ptr(), obj=obj.data_ptr(), positive=positive.data_ptr(), cls=None, K=3, Q=2, h=4, w=4, Hp=8, Wp=8, Hi=6, Wi=6,
                  H=8, W=8)
    outputs = [(arg, [[1] * 8] * 8), (obj, [[1] * 8] * 8), (positive, [FILL, FILL + 64, FILL + 64])]
    pinned = torch.empty(4096, dtype=torch.uint8).pin_memory()
    table = full((4096,), torch.uint8)
    st = lib.current_stream()

    def call(count=1, pinned_=pinned.data_ptr(), table_=table.data_ptr(), no_list=False, **over):
        arr = (A.PdAssignPairs * 1)()
        for k, v in {**fields, **over}.items():
            setattr(arr[0], k, v)
        return so.pd_pair_assign_resized(None if no_list else arr, count, pinned_, table_, st)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in [table] + [t for t, _ in outputs])

    assert call(count=0) == 0 and untouched()
    for what, kw in (("list", dict(no_list=True)), ("pinned table", dict(pinned_=None)), ("device table", dict(table_=None)),
                     ("K", dict(K=A.MAX_K + 1)), ("Q", dict(Q=A.MAX_Q + 1)), ("K = 0", dict(K=0)), ("Q = 0", dict(Q=0)),
                     ("pair_query", dict(pair_query=None))):
        assert call(**kw) == PD_ERR_INVALID_ARG, what
        message = so.pd_last_error().decode()
        assert message.startswith(name + ":"), (what, message)
        assert untouched(), what
    assert (A.MAX_K, A.MAX_Q) == (256, 1024)
    assert call(K=257) == PD_ERR_INVALID_ARG and "K=257" in so.pd_last_error().decode()
    assert call(Q=1025) == PD_ERR_INVALID_ARG and "Q=1025" in so.pd_last_error().decode()
    assert untouched()
    assert call() == 0
    torch.cuda.synchronize()
    for t, want in outputs:
        assert torch.equal(t.cpu(), torch.tensor(want, dtype=t.dtype).reshape(t.shape)), t
