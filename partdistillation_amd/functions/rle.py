"""COCO run-length codec on the device (include/pd_rle.h, csrc/rle.hip): masks and label maps that live on the GPU become the reference's
pseudo-label dicts (utils/utils.py:15-32 proposals_to_coco_json) without a dense copy to the host, and such dicts become a label map
(continuously_postprocess_dcrf.py's `cmask`) or masks on the device.  Only run tables cross the bus; the ASCII step stays on the host
(utils/rle.py).  GPU only; there is no fallback."""
import numpy as np
import torch

from .. import lib as _lib
from ..utils import rle as _rle

SEG_ROWS = 8                     # PD_RLE_SEG_ROWS: rows a lane walks per (plane, column, segment) key of the count / write passes
_MIN_CAPACITY = 1 << 16          # runs


class _Buffers:
    """grow-only per-device buffers of plane_runs: the run table (int32 starts, then uint8 values), the head (int64 non-zero counts, then
    int32 offsets), the workspace, and pinned host twins of the first two — steady state allocates nothing"""

    def __init__(self, device):
        self.device = device
        self.capacity = 0
        self.runs = self.head = self.work = self.host_runs = self.host_head = None

    @staticmethod
    def _grown(buf, nbytes, **kw):
        if buf is not None and buf.numel() >= nbytes:
            return buf
        return torch.empty(max(nbytes, 2 * (buf.numel() if buf is not None else 0)), dtype=torch.uint8, **kw)

    def reserve(self, capacity, n, work_bytes):
        if capacity > self.capacity:
            self.capacity = max(capacity, 2 * self.capacity)
            self.runs = torch.empty(5 * self.capacity, dtype=torch.uint8, device=self.device)
            self.host_runs = torch.empty(5 * self.capacity, dtype=torch.uint8, pin_memory=True)
        self.head = self._grown(self.head, 12 * n + 4, device=self.device)
        self.host_head = self._grown(self.host_head, 12 * n + 4, pin_memory=True)
        self.work = self._grown(self.work, work_bytes, device=self.device)


_buffers = {}


def _require_gpu(t, who):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{who} runs on the GPU only (no CPU fallback in partdistillation_amd)")


def _planes_u8(planes, who):
    if planes.dim() != 3 or planes.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{who}: uint8 or bool [n, H, W] expected, got {planes.dtype} {tuple(planes.shape)}")
    n, H, W = planes.shape
    if n and H and W and (planes.stride(2) != 1 or planes.stride(1) != W or planes.stride(0) < 0):
        planes = planes.contiguous()                       # planes may be any distance apart, each must be row-major and dense
    return planes.view(torch.uint8) if planes.dtype == torch.bool else planes


def _labels_u8(labels, planes, who):
    if labels.dim() != 2 or labels.dtype != torch.uint8 or tuple(labels.shape) != tuple(planes.shape[1:]):
        raise ValueError(f"{who}: labels uint8 {tuple(planes.shape[1:])} expected, got {labels.dtype} {tuple(labels.shape)}")
    if labels.device != planes.device:
        raise ValueError(f"{who}: planes on {planes.device}, labels on {labels.device}")
    return labels.contiguous()


def plane_runs(planes, binary):
    """planes uint8 / bool [n, H, W] on the GPU -> host arrays (offsets int32 [n + 1], starts int32, values uint8, nonzero int64 [n]): the
    runs of every plane's COLUMN-major flattening (plane i: entries [offsets[i], offsets[i + 1])), of (byte != 0) when `binary`, of the
    byte values otherwise, and the planes' exact non-zero pixel counts.  Two blocking reads: offsets + counts, then the run table."""
    _require_gpu(planes, "pd_rle_plane_runs")
    return _runs(_planes_u8(planes, "plane_runs"), "plane_runs", "pd_rle_plane_runs", (int(bool(binary)),))


def plane_label_runs(planes, labels):
    """planes uint8 / bool [n, H, W] and labels uint8 [H, W] on the GPU -> `plane_runs(v, binary=False)` of the virtual planes
    v[i] = where(planes[i], labels, 0), which are never written (pd_rle_masked_label_runs): the same host tuple, the same grow-and-relaunch
    path, the same two blocking reads"""
    _require_gpu(planes, "pd_rle_masked_label_runs")
    _require_gpu(labels, "pd_rle_masked_label_runs")
    planes = _planes_u8(planes, "plane_label_runs")
    labels = _labels_u8(labels, planes, "plane_label_runs")
    return _runs(planes, "plane_label_runs", "pd_rle_masked_label_runs", (labels.data_ptr(),))


def _runs(planes, who, entry, extra):
    """the launch / read / grow / read sequence of `plane_runs` for the entry point `entry`, whose arguments between W and capacity are
    `extra`"""
    n, H, W = (int(s) for s in planes.shape)
    if n == 0 or H == 0 or W == 0:
        return np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(n, dtype=np.int64)
    lib, dev = _lib.load(), planes.device
    assert lib.pd_rle_seg_rows() == SEG_ROWS
    work_bytes = lib.pd_rle_runs_workspace_bytes(n, H, W)
    if work_bytes < 0:
        raise ValueError(f"{who}: {n} planes of {H} x {W} are beyond the limits of {entry} (include/pd_rle.h)")
    buf = _buffers.get(dev)
    if buf is None:
        buf = _buffers[dev] = _Buffers(dev)
    buf.reserve(max(buf.capacity, _MIN_CAPACITY), n, work_bytes)
    stride = planes.stride(0) if n > 1 else H * W
    with torch.cuda.device(dev):
        st = _lib.current_stream()

        def launch():
            cap = buf.capacity
            _lib.check(getattr(lib, entry)(planes.data_ptr(), stride, n, H, W, *extra, cap, buf.runs.data_ptr(),
                                           buf.runs.data_ptr() + 4 * cap, buf.head.data_ptr() + 8 * n, buf.head.data_ptr(),
                                           buf.work.data_ptr(), st))

        launch()
        buf.host_head[:12 * n + 4].copy_(buf.head[:12 * n + 4], non_blocking=True)
        torch.cuda.current_stream().synchronize()                                           # blocking read 1
        head = buf.host_head[:12 * n + 4].numpy()
        nonzero, offsets = head[:8 * n].view(np.int64).copy(), head[8 * n:].view(np.int32).copy()
        total = int(offsets[n])
        if total > buf.capacity:                                                            # grow and run again; the head does not change
            buf.reserve(total, n, work_bytes)
            launch()
        cap = buf.capacity
        buf.host_runs[:4 * total].copy_(buf.runs[:4 * total], non_blocking=True)
        buf.host_runs[4 * total:5 * total].copy_(buf.runs[4 * cap:4 * cap + total], non_blocking=True)
        torch.cuda.current_stream().synchronize()                                           # blocking read 2
    runs = buf.host_runs[:5 * total].numpy()
    return offsets, runs[:4 * total].view(np.int32).copy(), runs[4 * total:].copy(), nonzero


def encode_masks(masks):
    """masks bool / uint8 [n, H, W] on the GPU -> (utils.rle.masks_to_coco_json(masks.cpu()), byte for byte; areas int64 numpy [n])"""
    _require_gpu(masks, "pd_rle_plane_runs")
    masks = _planes_u8(masks, "encode_masks")
    n, H, W = (int(s) for s in masks.shape)
    if n == 0 or H == 0 or W == 0:
        return _rle.masks_to_coco_json(np.zeros((n, H, W), dtype=bool)), np.zeros(n, dtype=np.int64)
    offsets, starts, values, nonzero = plane_runs(masks, binary=True)
    return _rle.run_table_to_coco_json(offsets, starts, values, (H, W)), nonzero


def encode_label_map(labels, present=None):
    """labels uint8 [H, W] on the GPU (0 = background) -> (utils.rle.labels_to_coco_json(labels.cpu(), present), pixel counts int64 numpy
    [256] by label value).  present: ascending labels to write, by default the non-zero values that occur."""
    _require_gpu(labels, "pd_rle_plane_runs")
    if labels.dim() != 2 or labels.dtype != torch.uint8:
        raise ValueError(f"encode_label_map: uint8 [H, W] expected, got {labels.dtype} {tuple(labels.shape)}")
    H, W = (int(s) for s in labels.shape)
    _, starts, values, _ = plane_runs(labels[None], binary=False)
    lengths = np.diff(starts.astype(np.int64), append=H * W)
    counts = label_counts(values, lengths)
    if present is None:
        present = [int(l) for l in np.flatnonzero(counts[1:]) + 1]
    return _rle.runs_to_coco_json(values, lengths, (H, W), present), counts


def encode_plane_labels(planes, labels):
    """planes uint8 / bool [n, H, W] and labels uint8 [H, W] on the GPU (0 = background) -> (per plane the list [(label, entry), ...] in
    ascending label order over the non-zero labels that occur under the plane, entry = utils.rle.labels_to_coco_json(where(plane,
    labels, 0), [label])[0]; pixel counts int64 numpy [n, 256] by plane and label value).  Only run tables cross the bus."""
    offsets, starts, values, _ = plane_label_runs(planes, labels)
    n, H, W = (int(s) for s in planes.shape)
    out, counts = [], np.zeros((n, 256), dtype=np.int64)
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        lengths = np.diff(starts[a:b].astype(np.int64), append=H * W)
        counts[i] = label_counts(values[a:b], lengths)
        present = [int(l) for l in np.flatnonzero(counts[i, 1:]) + 1]
        out.append(list(zip(present, _rle.runs_to_coco_json(values[a:b], lengths, (H, W), present))))
    return out, counts


def label_counts(values, lengths, minlength=256):
    """pixels per label value from a label map's runs, int64 [max(minlength, largest value + 1)]"""
    counts = np.zeros(max(int(minlength), int(values.max()) + 1 if values.size else 0), dtype=np.int64)
    np.add.at(counts, values, lengths)
    return counts


def _decode(segmentations, size, device, want_labels):
    H, W = int(size[0]), int(size[1])
    starts, offsets = _rle.segmentations_to_starts(segmentations, (H, W))      # ValueError on a size mismatch, before any device work
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("pd_rle_decode runs on the GPU only (no CPU fallback in partdistillation_amd)")
    n = len(offsets) - 1
    out = torch.empty((H, W), dtype=torch.int32, device=device) if want_labels else torch.empty((n, H, W), dtype=torch.uint8, device=device)
    if out.numel():
        table = torch.from_numpy(np.concatenate([offsets, starts])).to(device)  # one upload
        with torch.cuda.device(device):
            _lib.check(_lib.load().pd_rle_decode(table.data_ptr() + 4 * (n + 1), table.data_ptr(), n, H, W, out.data_ptr() if want_labels else None,
                                                 None if want_labels else out.data_ptr(), _lib.current_stream()))
    return out if want_labels else out.view(torch.bool)


def decode_label_map(segmentations, size, device="cuda"):
    """list of COCO RLE dicts (or of {"segmentation": rle}), each of `size` -> int32 [H, W] on the device:
    labels[y][x] = sum over the masks i that cover the pixel of (i + 1) — the reference's cmask, overlaps included"""
    return _decode([s.get("segmentation", s) for s in segmentations], size, device, True)


def decode_masks(segmentations, size, device="cuda"):
    """the same input -> bool [n, H, W] on the device"""
    return _decode([s.get("segmentation", s) for s in segmentations], size, device, False)
