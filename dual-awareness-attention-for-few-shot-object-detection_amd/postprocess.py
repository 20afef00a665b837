"""Inference post-processing on device: what inference.py:106-140 does between the
model call and `all_boxes[j][i] = cls_dets` -- de-normalise the regression deltas, decode them on the rois,
clip, rescale to the original image, threshold the fg score, sort, NMS (utils.py:312-317) -- as ONE C call
(decode + device sort + on-device NMS) and one small D2H read for the variable-length result.
`detections_batched` does the same for B images in one C call and one D2H read of the per-image counts."""
import ctypes

import torch

from . import ops
from ._lib import lib
from .config import cfg


def detections(rois, cls_prob, bbox_pred, im_info, thresh=0.05, nms_inclusive=False):
    """rois [1,R,5], cls_prob [R,2], bbox_pred [R,4], im_info [1,3] (device tensors of one image, as returned
    by the eval forward) -> cls_dets [K,5] = (x1,y1,x2,y2,score), descending score (what utils.NMS returns)."""
    rois = ops._chk(rois.reshape(-1, 5).contiguous(), "rois")
    cls_prob = ops._chk(cls_prob.reshape(-1, 2).contiguous(), "cls_prob")
    bbox_pred = ops._chk(bbox_pred.reshape(-1, 4).contiguous(), "bbox_pred")
    im_info = ops._chk(im_info.reshape(-1)[:3].float().contiguous(), "im_info")
    R = rois.size(0)
    dev = rois.device
    dets = torch.empty((R, 5), dtype=torch.float32, device=dev)
    ibuf = torch.empty((R + 2,), dtype=torch.int32, device=dev)  # keep positions | meta[2]
    ws = ops._ws(lib().query("dana_detect_postprocess_workspace_bytes", R), dev)
    f4 = ctypes.c_float * 4
    lib().call("dana_detect_postprocess", ops._p(rois), ops._p(cls_prob), ops._p(bbox_pred), ops._p(im_info), R,
               ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_STDS), ctypes.c_void_p),
               ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_MEANS), ctypes.c_void_p),
               int(bool(cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)), float(thresh), float(cfg.TEST.NMS),
               int(bool(nms_inclusive)), ops._p(dets), ibuf.data_ptr(), ibuf.data_ptr() + 4 * R, ops._p(ws),
               ws.numel(), ops._stream())
    host = ibuf.cpu()
    n_valid, n_keep = int(host[R]), int(host[R + 1])
    keep = host[:n_keep]
    keep = keep[keep < n_valid].long().to(dev)
    return dets[keep]


def _detections_packed(rois, cls_prob, bbox_pred, im_info, thresh, nms_inclusive):
    """the batched call itself -> (dets [max(B*R,1),5] packed device buffer, host int32 counts [B], offsets [B+1])"""
    if rois.dim() != 3 or rois.size(2) != 5:
        raise ValueError("detections_batched: rois must be [B, R, 5], got %s" % (tuple(rois.shape),))
    B, R = rois.size(0), rois.size(1)
    rois = ops._chk(rois.contiguous(), "rois")
    cls_prob = ops._chk(cls_prob.reshape(-1, 2).contiguous(), "cls_prob")
    bbox_pred = ops._chk(bbox_pred.reshape(-1, 4).contiguous(), "bbox_pred")
    im_info = ops._chk(im_info.reshape(-1, im_info.size(-1))[:, :3].float().contiguous(), "im_info")
    if cls_prob.size(0) != B * R or bbox_pred.size(0) != B * R or im_info.size(0) != B:
        raise ValueError("detections_batched: cls_prob / bbox_pred need B*R = %d rows and im_info B = %d rows" % (B * R, B))
    dev = rois.device
    dets = torch.empty((max(B * R, 1), 5), dtype=torch.float32, device=dev)
    layout = torch.empty((2 * B + 1,), dtype=torch.int32, device=dev)  # counts [B] | offsets [B+1]
    ws = ops._ws(lib().query("dana_detect_postprocess_batched_workspace_bytes", B, R), dev)
    f4 = ctypes.c_float * 4
    lib().call("dana_detect_postprocess_batched", ops._p(rois), ops._p(cls_prob), ops._p(bbox_pred), ops._p(im_info), B,
               R, ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_STDS), ctypes.c_void_p),
               ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_MEANS), ctypes.c_void_p),
               int(bool(cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)), float(thresh), float(cfg.TEST.NMS),
               int(bool(nms_inclusive)), ops._p(dets), layout.data_ptr(), layout.data_ptr() + 4 * B, ops._p(ws),
               ws.numel(), ops._stream())
    host = layout.cpu()
    return dets, host[:B], host[B:]


def detections_batched(rois, cls_prob, bbox_pred, im_info, thresh=0.05, nms_inclusive=False, with_layout=False):
    """rois [B,R,5], cls_prob [B*R,2], bbox_pred [B*R,4], im_info [B,3] (the eval forward's outputs for B images) ->
    list of B cls_dets [K_b,5], each equal to `detections()` on its image. One C call (decode over B*R rows, B-row sort,
    B NMS problems, packed compaction) and ONE D2H read of the per-image counts / offsets. with_layout=True also returns
    the host int32 tensors counts [B] and offsets [B+1] (image b's rows: dets[offsets[b]:offsets[b+1]])."""
    dets, counts, offsets = _detections_packed(rois, cls_prob, bbox_pred, im_info, thresh, nms_inclusive)
    out = [dets[int(offsets[b]):int(offsets[b]) + int(counts[b])] for b in range(counts.numel())]
    return (out, counts, offsets) if with_layout else out


class ClassDetections(list):
    """`detections_by_class(with_layout=True)`: the nested list dets[b][c] itself, plus the one device buffer its entries
    are views of -- `packed` [rows,5], host int32 `counts` [B*C] and `offsets` [B*C+1] of problem p = b*C + c -- which is
    what `evaluate.DetectionEvaluator.add_by_class` appends in one launch instead of slicing B*C tensors apart."""
    packed = counts = offsets = None
    num_classes = 0


def detections_by_class(rois, cls_prob, bbox_pred, im_info, num_classes, thresh=0.05, nms_inclusive=False,
                        with_layout=False):
    """A class sweep's outputs (model(..., cache.sweep(classes)): rois [B*C,R,5], cls_prob [B*C*R,2], bbox_pred [B*C*R,4])
    with im_info [B,3] per IMAGE -> dets[b][c], a [K,5] tensor equal to `detections()` on problem b*C + c with image b's
    im_info: the all_boxes[j][i] layout of inference.py:70-140 (j the class, i the image). One batched post-processing
    call over the B*C problems, one D2H read; the im_info row of problem p (image p // C) is repeated on the device.
    with_layout=True returns the same nested list as a `ClassDetections`, which also carries the packed buffer."""
    if rois.dim() != 3 or rois.size(2) != 5:
        raise ValueError("detections_by_class: rois must be [B*C, R, 5], got %s" % (tuple(rois.shape),))
    C = int(num_classes)
    im_info = ops._chk(im_info.reshape(-1, im_info.size(-1)).float().contiguous(), "im_info")
    B = im_info.size(0)
    if C < 1 or rois.size(0) != B * C:
        raise ValueError("detections_by_class: %d problems for %d images x %d classes" % (rois.size(0), B, C))
    info_p = ops.repeat_rows_grouped(im_info, 1, 3, C, B * C, ld_src=im_info.size(1))
    packed, counts, offsets = _detections_packed(rois, cls_prob, bbox_pred, info_p, thresh, nms_inclusive)
    flat = [packed[int(offsets[p]):int(offsets[p]) + int(counts[p])] for p in range(B * C)]
    nested = [flat[b * C:(b + 1) * C] for b in range(B)]
    if not with_layout:
        return nested
    out = ClassDetections(nested)
    out.packed, out.counts, out.offsets, out.num_classes = packed, counts, offsets, C
    return out
