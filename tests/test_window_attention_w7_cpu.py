"""Host side of the 7 x 7 window attention (include/pd_window_attention.h, *_w7): the header's table-index formula against the
reference-style relative_position_index, the region labels against the reference's shifted-window mask, and the shipped Swin-T
config.  None of it needs a GPU."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "partdistillation_amd", "configs")


def _relative_position_index(ws):
    ch, cw = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    coords = torch.stack([ch.reshape(-1), cw.reshape(-1)])
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def _reference_mask(H, W, shift, ws):
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    img = torch.zeros((1, Hp, Wp, 1))
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = img.view(1, Hp // ws, ws, Wp // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)


def test_header_index_formula_is_the_relative_position_index():
    """index(q, key) = A(q) - A(key) + 84, A(t) = t + 6 * (t / 7), over all 49^2 pairs; the range is exactly the 169-row table"""
    t = torch.arange(49)
    A = t + 6 * (t // 7)
    idx = A[:, None] - A[None, :] + 84
    assert torch.equal(idx, _relative_position_index(7))
    assert idx.min().item() == 0 and idx.max().item() == 168
    assert sorted(idx.unique().tolist()) == list(range(169))
    # the kernel's division-free t / 7 for the 64 on-chip rows
    assert all((x * 37) >> 8 == x // 7 for x in range(64))


@pytest.mark.parametrize("H,W", [(14, 14), (10, 17), (7, 7)])
def test_regions_reproduce_the_reference_mask_w7(H, W):
    from partdistillation_amd.functions import window_attention as wa
    assert wa.WINDOWS == (12, 7)
    reg, flags = wa.shifted_window_regions(H, W, 3, "cpu", window=7)
    nW = (-(-H // 7)) * (-(-W // 7))
    assert reg.shape == (nW, 49) and reg.dtype == torch.uint8 and flags.shape == (nW,) and flags.dtype == torch.uint8
    mask = _reference_mask(H, W, 3, 7)
    ours = (reg[:, :, None] != reg[:, None, :])
    assert torch.equal(ours, mask == -100.0) and torch.equal(~ours, mask == 0.0)
    more_than_one = torch.tensor([len(r.unique()) > 1 for r in reg])
    assert torch.equal(flags.bool(), more_than_one)
    # window 12: the same call with and without `window=` is the same thing, and still the reference's mask
    r12, f12 = wa.shifted_window_regions(H, W, 3, "cpu", window=12)
    d12, g12 = wa.shifted_window_regions(H, W, 3, "cpu")
    assert r12.shape[1] == 144 and torch.equal(r12, d12) and torch.equal(f12, g12)
    assert torch.equal(r12[:, :, None] != r12[:, None, :], _reference_mask(H, W, 3, 12) == -100.0)


@pytest.mark.parametrize("H,W", [(7, 9), (14, 14), (7, 7)])
def test_library_path_mask_for_one_row_of_windows(H, W):
    """the additive mask of the module-by-module path: a 7 x 9 grid (Swin-T's second stage on a 56 x 72 image) is one row of two windows"""
    from partdistillation_amd.modeling.backbone.swin import shifted_window_mask
    assert torch.equal(shifted_window_mask(H, W, 7, 3, "cpu"), _reference_mask(H, W, 3, 7))


def test_supported_needs_a_gpu_tensor():
    from partdistillation_amd.functions import window_attention as wa
    qkv = torch.zeros(4, 49, 3 * 96, dtype=torch.bfloat16)
    assert not wa.supported(qkv, (7, 7), 3, 0.0)                # CPU tensor
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.window_attention(qkv, torch.zeros(169, 3), None, 1.0, 1)


def test_swint_config_loads_and_backbone_builds():
    import partdistillation_amd.modeling  # noqa: F401  (registers)
    from partdistillation_amd.compat import BACKBONE_REGISTRY
    from partdistillation_amd.config import setup_cfg
    cfg = setup_cfg(os.path.join(CONFIGS, "proposal_learning", "swint_mask2former.yaml"), ["MODEL.DEVICE", "cpu"])
    s = cfg.MODEL.SWIN
    assert cfg.MODEL.BACKBONE.NAME == "D2SwinTransformer" and cfg.MODEL.META_ARCHITECTURE == "ProposalModel"
    assert s.WINDOW_SIZE == 7 and s.EMBED_DIM == 96 and list(s.DEPTHS) == [2, 2, 6, 2] and list(s.NUM_HEADS) == [3, 6, 12, 24]
    assert s.DROP_PATH_RATE == 0.3 and s.APE is False and s.PATCH_NORM is True
    base = setup_cfg(os.path.join(CONFIGS, "proposal_learning", "swinl_mask2former.yaml"))
    assert cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES == base.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES
    assert cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES == base.MODEL.SEM_SEG_HEAD.NUM_CLASSES
    net = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, None)
    sd = net.state_dict()
    for i, heads in enumerate([3, 6, 12, 24]):
        for blk in net.layers[i].blocks:
            assert blk.attn.window_size == (7, 7) and blk.attn.num_heads == heads and blk.attn.dim == 32 * heads
            assert blk.attn.relative_position_bias_table.shape == (169, heads) and blk.attn.relative_position_index.shape == (49, 49)
        assert [blk.shift_size for blk in net.layers[i].blocks] == [0, 3] * (len(net.layers[i].blocks) // 2)
    # the key names of the other Swin configs: Swin-B's with the third stage cut to 6 blocks
    swinb = setup_cfg(os.path.join(CONFIGS, "part_distillation", "swinb_mask2former.yaml"), ["MODEL.DEVICE", "cpu", "MODEL.SWIN.DEPTHS", "[2, 2, 6, 2]"])
    other = BACKBONE_REGISTRY.get(swinb.MODEL.BACKBONE.NAME)(swinb, None).state_dict()
    assert set(sd) == set(other)
    assert "layers.2.blocks.5.attn.relative_position_bias_table" in sd and "layers.2.blocks.6.attn.qkv.weight" not in sd
    assert "patch_embed.norm.weight" in sd and "absolute_pos_embed" not in sd
