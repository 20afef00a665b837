"""Inference post-processing on device: what inference.py:106-140 does between the
model call and `all_boxes[j][i] = cls_dets` -- de-normalise the regression deltas, decode them on the rois,
clip, rescale to the original image, threshold the fg score, sort, NMS (utils.py:312-317) -- as ONE C call
(decode + device sort + on-device NMS) and one small D2H read for the variable-length result.
`detections_batched` does the same for B images in one C call and one D2H read of the per-image counts.

`merge_detections` combines such lists on the device (csrc/merge.hip): what utils.py:182-204 (generate_pseudo_label) does
with the per-shot lists of an image -- cat, sort by score, one more NMS over the union -- and the `max_per_image` cut over
an image's class lists (inference.py:70), as one C call over all lists and one D2H read of the output layout;
`ensemble_shots` and `cap_per_image` are the two uses spelled out. `as_gt_boxes` turns merged lists into the
gt_boxes / num_boxes tensors of a train-mode forward (pseudo-labels are trained on, utils.py:130-179) without leaving the
device. `merge_numpy` is the merge restated in numpy float64 (host): the tests' yardstick, pinned to the reference's own
chain by tests/golden/merge_dets.npz. `merge_detections(method="linear" | "gaussian", vote_thresh=...)` runs Soft-NMS and box
voting in the same call (dana_detect_merge_soft; restated from their papers, not from the reference), and
`merge_soft_numpy` is their host restatement, operation for operation.

`fold_views` / `ensemble_views` are the same merge for the other source of redundant lists, test-time augmentation: the
lists of a sweep over the B * V views `pipeline.plan_views` planned (mirrored, several scales) are mapped back into the frame
of their image and laid out list-major on the device (csrc/views.hip, one C call, nothing read back), then merged with
groups = V. `fold_views_numpy` restates the fold in numpy float32. Neither is in the reference tree.

`fold_tiles` is that fold for tiled inference: the views of `pipeline.plan_tiles` are overlapping windows of the frame (beside
an optional full-frame view), so a list is first tested against its tile, put through the seam rule, clipped to the tile and
translated (dana_detect_fold_tiles, the same kernel body). `ensemble_views` takes a `TileSet` and folds with it;
`fold_tiles_numpy` is the restatement."""
import ctypes
import math

import numpy as np
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


def _decode_nms_thresh(nms_thresh):
    """the `nms_thresh` keyword of the batched decoders -> the float handed to the C call: "cfg" is cfg.TEST.NMS; None is
    2.0, above every IoU (with +1 widths iou <= 1), so nothing is suppressed and the lists come back thresholded and sorted"""
    if nms_thresh is None:
        return 2.0
    return float(cfg.TEST.NMS if isinstance(nms_thresh, str) and nms_thresh == "cfg" else nms_thresh)


def _detections_packed(rois, cls_prob, bbox_pred, im_info, thresh, nms_inclusive, nms_thresh="cfg"):
    """the batched call itself -> (dets [max(B*R,1),5] packed device buffer, host int32 counts [B], offsets [B+1], and the
    device int32 tensor counts | offsets [2B+1] the host pair was read from)"""
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
               int(bool(cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)), float(thresh), _decode_nms_thresh(nms_thresh),
               int(bool(nms_inclusive)), ops._p(dets), layout.data_ptr(), layout.data_ptr() + 4 * B, ops._p(ws),
               ws.numel(), ops._stream())
    host = layout.cpu()
    return dets, host[:B], host[B:], layout


def detections_batched(rois, cls_prob, bbox_pred, im_info, thresh=0.05, nms_inclusive=False, with_layout=False, *,
                       nms_thresh="cfg"):
    """rois [B,R,5], cls_prob [B*R,2], bbox_pred [B*R,4], im_info [B,3] (the eval forward's outputs for B images) ->
    list of B cls_dets [K_b,5], each equal to `detections()` on its image. One C call (decode over B*R rows, B-row sort,
    B NMS problems, packed compaction) and ONE D2H read of the per-image counts / offsets. with_layout=True also returns
    the host int32 tensors counts [B] and offsets [B+1] (image b's rows: dets[offsets[b]:offsets[b+1]]). `nms_thresh`
    replaces cfg.TEST.NMS in the call; None leaves the lists unsuppressed (thresholded and sorted), which is what a
    soft-NMS `merge_detections(..., 1, method="linear")` over them starts from."""
    dets, counts, offsets, _ = _detections_packed(rois, cls_prob, bbox_pred, im_info, thresh, nms_inclusive, nms_thresh)
    out = [dets[int(offsets[b]):int(offsets[b]) + int(counts[b])] for b in range(counts.numel())]
    return (out, counts, offsets) if with_layout else out


class ClassDetections(list):
    """`detections_by_class(with_layout=True)`: the nested list dets[b][c] itself, plus the one device buffer its entries
    are views of -- `packed` [rows,5], host int32 `counts` [B*C] and `offsets` [B*C+1] of problem p = b*C + c -- which is
    what `evaluate.DetectionEvaluator.add_by_class` appends in one launch instead of slicing B*C tensors apart. `layout_dev`
    is the same layout where the device wrote it (int32 [2*B*C+1]: counts | offsets), which `merge_detections` reads in place."""
    packed = counts = offsets = layout_dev = None
    num_classes = 0


def detections_by_class(rois, cls_prob, bbox_pred, im_info, num_classes, thresh=0.05, nms_inclusive=False,
                        with_layout=False, *, nms_thresh="cfg"):
    """A class sweep's outputs (model(..., cache.sweep(classes)): rois [B*C,R,5], cls_prob [B*C*R,2], bbox_pred [B*C*R,4])
    with im_info [B,3] per IMAGE -> dets[b][c], a [K,5] tensor equal to `detections()` on problem b*C + c with image b's
    im_info: the all_boxes[j][i] layout of inference.py:70-140 (j the class, i the image). One batched post-processing
    call over the B*C problems, one D2H read; the im_info row of problem p (image p // C) is repeated on the device.
    with_layout=True returns the same nested list as a `ClassDetections`, which also carries the packed buffer.
    `nms_thresh` as in `detections_batched` (None: no per-class NMS, for soft-NMS in its place)."""
    if rois.dim() != 3 or rois.size(2) != 5:
        raise ValueError("detections_by_class: rois must be [B*C, R, 5], got %s" % (tuple(rois.shape),))
    C = int(num_classes)
    im_info = ops._chk(im_info.reshape(-1, im_info.size(-1)).float().contiguous(), "im_info")
    B = im_info.size(0)
    if C < 1 or rois.size(0) != B * C:
        raise ValueError("detections_by_class: %d problems for %d images x %d classes" % (rois.size(0), B, C))
    info_p = ops.repeat_rows_grouped(im_info, 1, 3, C, B * C, ld_src=im_info.size(1))
    packed, counts, offsets, layout = _detections_packed(rois, cls_prob, bbox_pred, info_p, thresh, nms_inclusive, nms_thresh)
    flat = [packed[int(offsets[p]):int(offsets[p]) + int(counts[p])] for p in range(B * C)]
    nested = [flat[b * C:(b + 1) * C] for b in range(B)]
    if not with_layout:
        return nested
    out = ClassDetections(nested)
    out.packed, out.counts, out.offsets, out.num_classes, out.layout_dev = packed, counts, offsets, C, layout
    return out


# ---- merging detection lists ---------------------------------------------------------------------------------------------

class MergedDetections(ClassDetections):
    """`merge_detections(with_layout=True)`: the list of merged lists (views of `packed`), the host `counts` [n] / `offsets`
    [n+1] and device `layout_dev` of a `ClassDetections`, plus per packed row the device int32 `group` (which of the list's
    `groups` inputs the row came from) and `row` (its row inside that input). `total` = rows in all lists."""
    group = row = None
    total = 0
    votes = None  # device int32 [total]: the voters of every packed row, when the merge ran with box voting

    def _take_layout(self, m):
        self.packed, self.counts, self.offsets, self.layout_dev = m.packed, m.counts, m.offsets, m.layout_dev
        self.total, self.group, self.row, self.votes = m.total, m.group, m.row, m.votes

    def list_index(self):
        """host int32 [total]: the output list of every packed row (what `add_packed` takes as image ids, mapped through
        the caller's image indices)"""
        c = self.counts.numpy().astype(np.int64)
        return np.repeat(np.arange(c.size, dtype=np.int32), c)


def _nms_pair(nms_thresh):
    """the `nms_thresh` argument -> (do_nms, threshold): "cfg" is cfg.TEST.NMS, None turns NMS off"""
    if nms_thresh is None:
        return 0, 0.0
    return 1, float(cfg.TEST.NMS if isinstance(nms_thresh, str) and nms_thresh == "cfg" else nms_thresh)


def _packed_layout(dets, who):
    """a ClassDetections-like object or a tuple (packed, counts, offsets) -> (packed [rows,5] device, P, host counts and
    offsets as numpy int64 or None when the layout lives on the device only, device pointers of counts [P] and
    offsets [>=P], and the tensors that keep those pointers alive)"""
    if isinstance(dets, (tuple, list)) and not hasattr(dets, "packed"):
        if len(dets) != 3:
            raise ValueError("%s: pass a ClassDetections or a tuple (packed, counts, offsets)" % who)
        packed, counts, offsets, layout = dets[0], dets[1], dets[2], None
    else:
        packed, counts, offsets = dets.packed, dets.counts, dets.offsets
        layout = getattr(dets, "layout_dev", None)
    if packed is None or counts is None or offsets is None:
        raise ValueError("%s: the detections carry no packed layout (detections_by_class(..., with_layout=True))" % who)
    packed = ops._chk(packed.reshape(-1, 5), "packed")
    on_dev = [isinstance(x, torch.Tensor) and x.is_cuda for x in (counts, offsets)]
    if all(on_dev) and layout is None:
        counts, offsets = ops._chk(counts.reshape(-1), "counts", torch.int32), ops._chk(offsets.reshape(-1), "offsets", torch.int32)
        P = counts.numel()
        if offsets.numel() < P:
            raise ValueError("%s: %d counts but %d offsets" % (who, P, offsets.numel()))
        return packed, P, None, None, counts.data_ptr(), offsets.data_ptr(), (counts, offsets)
    if any(on_dev):
        raise ValueError("%s: counts and offsets must both be host or both be device int32 tensors" % who)
    hc = np.asarray(counts).reshape(-1).astype(np.int64)
    ho = np.asarray(offsets).reshape(-1).astype(np.int64)
    P = hc.size
    if ho.size < P or (hc < 0).any() or (ho[:P] < 0).any() or (P and int((ho[:P] + hc).max()) > packed.size(0)):
        raise ValueError("%s: counts / offsets do not describe rows of the packed buffer" % who)
    if layout is None or layout.numel() < 2 * P:
        layout = ops._h2d_int32(np.concatenate((hc, ho[:P])).astype(np.int32), packed.device)
    layout = ops._chk(layout, "layout_dev", torch.int32)
    return packed, P, hc, ho, layout.data_ptr(), layout.data_ptr() + 4 * P, (layout,)


SOFT_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}
VOTE_SCORES = {"id": 0, "avg": 1}


def _soft_args(who, nms_thresh, method, sigma, min_score, vote_thresh, vote_score):
    """the soft-NMS / voting keywords, checked before any C call -> (method id, sigma, min_score, vote_thresh or -1.0 when
    voting is off, vote_score id)"""
    if method not in SOFT_METHODS:
        raise ValueError("%s: method must be one of %s, got %r" % (who, sorted(SOFT_METHODS), method))
    if vote_score not in VOTE_SCORES:
        raise ValueError("%s: vote_score must be one of %s, got %r" % (who, sorted(VOTE_SCORES), vote_score))
    if method == "linear" and nms_thresh is None:
        raise ValueError("%s: method=\"linear\" decays the rows above nms_thresh and needs one, got None" % who)
    if not float(sigma) > 0.0:
        raise ValueError("%s: sigma must be positive, got %r" % (who, sigma))
    if vote_thresh is not None and not 0.0 < float(vote_thresh) <= 1.0:
        raise ValueError("%s: vote_thresh must lie in (0, 1], got %r" % (who, vote_thresh))
    return (SOFT_METHODS[method], float(sigma), float(min_score), -1.0 if vote_thresh is None else float(vote_thresh),
            VOTE_SCORES[vote_score])


def merge_detections(dets, groups, nms_thresh="cfg", nms_inclusive=False, max_dets=0, with_layout=False, capacity=None, *,
                     method="hard", sigma=0.5, min_score=0.001, vote_thresh=None, vote_score="id"):
    """Merge every `groups` consecutive detection lists into one, on the device: concatenate in group order, sort by score
    (descending, stable: equal scores keep concatenation order -- lower group first, then lower row), greedy NMS at
    `nms_thresh` ("cfg": cfg.TEST.NMS; None: no NMS, a pure merge), keep the first `max_dets` (0: all). The chain of
    utils.py:192-199 for every list at once; every output row is a bit-for-bit copy of an input row.

    `dets`: a `ClassDetections` (problem p goes to list p // groups) or a tuple (packed [rows,5], counts [P], offsets [P+])
    with host or device int32 layout. -> list of P // groups tensors [K_l,5]; with_layout=True a `MergedDetections`,
    which also carries `packed`, `counts`, `offsets`, `layout_dev`, `group`, `row`. One C call, one D2H read (the output
    layout). The frame a list is sorted in (`capacity` rows) is sized from the host counts; with a device-only layout
    pass `capacity` (>= the longest concatenation), because nothing is read back to find it.

    `method` "linear" / "gaussian" put Soft-NMS (Bodla et al. 2017) in the place of the hard NMS: the best live row is
    emitted with its working score, the live rows it overlaps are decayed -- by 1 - IoU above `nms_thresh`, or by
    exp(-IoU^2 / sigma) -- and rows falling below `min_score` are dropped; the output rows then carry the decayed scores, in
    descending order. `vote_thresh` in (0, 1] turns box voting on (Gidaris & Komodakis 2015) under any method: every emitted
    box becomes the score-weighted mean of ALL the list's input boxes with IoU >= vote_thresh to it, and `votes` (device
    int32 per packed row) counts them; `vote_score="avg"` also replaces the score by the voters' mean score. The definitions
    are in include/dana_hip.h (dana_detect_merge_soft) and restated by `merge_soft_numpy`. With the defaults (method "hard",
    no voting) the call and the result are dana_detect_merge's; otherwise a `MergedDetections` comes back, lists up to 3072
    rows long under the soft methods."""
    soft = _soft_args("merge_detections", nms_thresh, method, sigma, min_score, vote_thresh, vote_score)
    use_soft = soft[0] != 0 or vote_thresh is not None
    groups = int(groups)
    if groups < 1:
        raise ValueError("merge_detections: groups must be >= 1, got %d" % groups)
    packed, P, hc, _, p_counts, p_offsets, alive = _packed_layout(dets, "merge_detections")
    if P % groups:
        raise ValueError("merge_detections: %d lists are not a multiple of groups = %d" % (P, groups))
    n_lists = P // groups
    dev = packed.device
    if hc is not None:
        need = int(hc.reshape(n_lists, groups).sum(1).max()) if n_lists else 0
        if capacity is None:
            capacity = need
        elif int(capacity) < need:
            raise ValueError("merge_detections: capacity %d is below the longest concatenation (%d rows)" % (int(capacity), need))
        rows_cap = min(int(hc.sum()), n_lists * int(capacity))
    elif capacity is None:
        raise ValueError("merge_detections: a device-only layout needs capacity (nothing is read back to size the frame)")
    else:
        rows_cap = n_lists * int(capacity)
    capacity = int(capacity)
    do_nms, thr = _nms_pair(nms_thresh)
    out = torch.empty((max(rows_cap, 1), 5), dtype=torch.float32, device=dev)
    slot = max(rows_cap, 1)
    votes = None
    if not use_soft:
        ibuf = torch.empty((2 * slot + 2 * n_lists + 1,), dtype=torch.int32, device=dev)  # group | row | counts | offsets
        group, row, layout = ibuf[:slot], ibuf[slot:2 * slot], ibuf[2 * slot:]
        ws = ops._ws(lib().query("dana_detect_merge_workspace_bytes", n_lists, groups, capacity), dev)
        lib().call("dana_detect_merge", ops._p(packed), p_counts, p_offsets, n_lists, groups, capacity, do_nms, thr,
                   int(bool(nms_inclusive)), int(max_dets), ops._p(out), group.data_ptr(), row.data_ptr(), layout.data_ptr(),
                   layout.data_ptr() + 4 * n_lists, ops._p(ws), ws.numel(), ops._stream())
    else:
        ibuf = torch.empty((3 * slot + 2 * n_lists + 1,), dtype=torch.int32, device=dev)  # group | row | votes | counts | offsets
        group, row, votes, layout = ibuf[:slot], ibuf[slot:2 * slot], ibuf[2 * slot:3 * slot], ibuf[3 * slot:]
        ws = ops._ws(lib().query("dana_detect_merge_soft_workspace_bytes", n_lists, groups, capacity), dev)
        lib().call("dana_detect_merge_soft", ops._p(packed), p_counts, p_offsets, n_lists, groups, capacity, do_nms, thr,
                   int(bool(nms_inclusive)), int(max_dets), soft[0], soft[1], soft[2], soft[3], soft[4], ops._p(out),
                   group.data_ptr(), row.data_ptr(), votes.data_ptr(), layout.data_ptr(), layout.data_ptr() + 4 * n_lists,
                   ops._p(ws), ws.numel(), ops._stream())
    del alive
    host = layout.cpu()
    counts, offsets = host[:n_lists], host[n_lists:]
    lists = [out[int(offsets[i]):int(offsets[i]) + int(counts[i])] for i in range(n_lists)]
    if not with_layout and not use_soft:
        return lists
    m = MergedDetections(lists)
    m.packed, m.counts, m.offsets, m.layout_dev, m.num_classes = out, counts, offsets, layout, 1
    m.total = int(offsets[n_lists])
    m.group, m.row = group[:m.total], row[:m.total]
    m.votes = votes[:m.total] if vote_thresh is not None else None
    return m


def ensemble_shots(cd, shots, nms_thresh="cfg", nms_inclusive=False, max_dets=0, *, method="hard", sigma=0.5, min_score=0.001,
                   vote_thresh=None, vote_score="id"):
    """The shot ensemble of utils.py:182-204: `cd` = detections_by_class(..., with_layout=True) of a sweep whose cached
    problems are laid out as c*shots + s (class c seen through its shot s alone: `cache.sweep(classes, shots="each")`
    on a k-shot cache, or a num_shot=1 model's cache of C*S one-shot sets). -> `merge_detections(cd, shots)` as dets[b][c], a
    `MergedDetections` that `DetectionEvaluator.add_by_class` / `CocoEvaluator.add_by_class` take unchanged. The soft-NMS and
    voting keywords are `merge_detections`'; K shots vote K times for an object, which is what box voting averages."""
    _soft_args("ensemble_shots", nms_thresh, method, sigma, min_score, vote_thresh, vote_score)
    shots = int(shots)
    if shots < 1 or cd.num_classes % shots:
        raise ValueError("ensemble_shots: %d sets per image are not a multiple of shots = %d" % (cd.num_classes, shots))
    C, B = cd.num_classes // shots, len(cd)
    m = merge_detections(cd, shots, nms_thresh, nms_inclusive, max_dets, with_layout=True, method=method, sigma=sigma,
                         min_score=min_score, vote_thresh=vote_thresh, vote_score=vote_score)
    out = MergedDetections([list(m[b * C:(b + 1) * C]) for b in range(B)])
    out._take_layout(m)
    out.num_classes = C
    return out


# ---- view ensembles: flip and multi-scale testing -------------------------------------------------------------------------
# Out of scope here: views times shots in one fold (fold the views, then merge the shots); views of an im_data tensor that
# did not come from an ImagePool (a resize of a resized image is not the loader's image); vertical flips and rotations;
# QueryBank views (training-time augmentation is `pipeline.plan_episode`'s, not a view's). The sibling detectors need nothing of their own: the fold sees only lists.

class FoldedViews:
    """`fold_views`' result, which `merge_detections(folded, folded.views, capacity=folded.capacity)` accepts: `packed`
    [rows,5] and device int32 `counts` / `offsets` of the problems q = (i * C + c) * V + v, nothing of it on the host.
    Rows of `packed` that no list's count covers are unwritten. `src_row` (device int32 per packed row) is a kept row's
    index inside its input list; `capacity` the longest concatenation of an (image, class)'s V input lists, an upper bound
    of the folded one because the fold only removes rows."""
    layout_dev = None

    def __init__(self, packed, counts, offsets, src_row, capacity, n_images, views, num_classes):
        self.packed, self.counts, self.offsets, self.src_row = packed, counts, offsets, src_row
        self.capacity, self.n_images, self.views, self.num_classes = capacity, n_images, views, num_classes


def _fold(who, entry, cd, views):
    V, B = int(views.views), int(views.n_images)
    if len(cd) != B * V:
        raise ValueError("%s: %d images in the detections, but %d images x %d views were planned" % (who, len(cd), B, V))
    packed, P, hc, ho, p_counts, p_offsets, alive = _packed_layout(cd, who)
    C = int(cd.num_classes)
    if hc is None or C < 1 or P != B * V * C:
        raise ValueError("%s: needs detections_by_class(..., with_layout=True) of %d x %d view images" % (who, B, V))
    dev = packed.device
    table = views.table_dev(dev)
    out = torch.empty_like(packed)
    ibuf = torch.empty((2 * P + packed.size(0),), dtype=torch.int32, device=dev)  # counts | offsets | src_row
    counts, offsets, src_row = ibuf[:P], ibuf[P:2 * P], ibuf[2 * P:]
    lib().call(entry, ops._p(packed), p_counts, p_offsets, B, V, C, ops._p(table), table.size(1), ops._p(out),
               counts.data_ptr(), offsets.data_ptr(), src_row.data_ptr(), ops._stream())
    del alive
    capacity = int(hc.reshape(B, V, C).sum(1).max()) if P else 0
    return FoldedViews(out, counts, offsets, src_row, capacity, B, V, C)


def _is_tiled(views):
    return getattr(views, "columns", 5) >= 13


def fold_views(cd, views):
    """`cd` = detections_by_class(..., with_layout=True) of a class sweep over the n_images * V view images of
    `pipeline.plan_views` (problem (i * V + v) * C + c), `views` its `ViewSet`. Every list is mapped into the frame of its
    original image -- un-mirrored, rows outside the frame dropped, clipped to the frame (not to the padded holder), cut to
    the view's area window -- and the layout transposed so that the V lists of one (image, class) are consecutive: the
    rule of include/dana_hip.h (dana_detect_fold_views), restated by `fold_views_numpy`. One C call, nothing read back.
    -> `FoldedViews`."""
    if _is_tiled(views):
        raise ValueError("fold_views: a TileSet's views are windows of the frame; fold them with fold_tiles")
    return _fold("fold_views", "dana_detect_fold_views", cd, views)


def fold_tiles(cd, tiles):
    """`fold_views` for tiled inference: `cd` = detections_by_class(..., with_layout=True) of a class sweep over the
    n_images * V view images of `pipeline.plan_tiles`, `tiles` its `TileSet`. A row is kept only if it touches its tile and
    keeps the margin from every interior side of it (the seam rule, on the unclipped box: an object cut by a tile's side
    comes back as a truncated box that NMS would not match with the whole box of the neighbouring tile); it is clipped to the
    TILE (not the padded holder), translated into the frame and then folded as `fold_views` does -- un-mirrored, frame test,
    clip, area window. The rule is include/dana_hip.h's (dana_detect_fold_tiles), restated by `fold_tiles_numpy`. The same
    packing, capacity and one C call as `fold_views`, nothing read back -> `FoldedViews`.
    Two limits. `capacity` is computed from the INPUT counts without a device read, and under the soft methods the 3072-row
    limit of a concatenation applies to all V views of a class together: with many tiles, detect the views with a per-view
    NMS or a score threshold, or merge with method="hard". And the coverage guarantee (`pipeline.tile_windows`) is about
    boxes no larger than overlap - 2 * margin: larger objects are the full-frame view's."""
    if not _is_tiled(tiles):
        raise ValueError("fold_tiles: needs the TileSet of pipeline.plan_tiles (13 table columns), got %d columns"
                         % getattr(tiles, "columns", 5))
    return _fold("fold_tiles", "dana_detect_fold_tiles", cd, tiles)


def ensemble_views(cd, views, nms_thresh="cfg", nms_inclusive=False, max_dets=0, *, method="hard", sigma=0.5, min_score=0.001,
                   vote_thresh=None, vote_score="id"):
    """Flip / multi-scale testing merged on the device: `fold_views(cd, views)`, then `merge_detections` over the V views of
    every (image, class) -> dets[i][c], a `MergedDetections` as `ensemble_shots` returns (`add_by_class`, `cap_per_image`,
    `as_gt_boxes`, `render.prediction_sheet` take it unchanged). `group` is the view index v = s * F + f of a row and `row`
    its index in the FOLDED list; `folded.src_row` (the `folded` attribute of the result) maps that to the row of `cd`'s
    list. The keywords are `merge_detections`'. Under the soft methods the 3072-row limit of a concatenation applies to the
    V views of a class together: with R rois per view, V * R <= 3072 is safe for any thresholds. Detect the views with
    `detections_by_class(..., nms_thresh=None)` to let soft-NMS see unsuppressed lists.
    `views` may be the `TileSet` of `pipeline.plan_tiles` (tiled inference): the lists are then folded with `fold_tiles`, and
    `group` is the view index v = t * F + f (t = 0 the full frame when planned, then the tiles row-major). Its two limits: the
    3072 rows are those of ALL V views of a class, counted on the INPUT lists without a device read -- with many tiles,
    detect the views with a per-view NMS or a score threshold, or use method="hard"; and only boxes no larger than
    overlap - 2 * margin are guaranteed a tile that holds them clear of its seams -- larger objects are the full-frame
    view's."""
    _soft_args("ensemble_views", nms_thresh, method, sigma, min_score, vote_thresh, vote_score)
    folded = fold_tiles(cd, views) if _is_tiled(views) else fold_views(cd, views)
    B, C = folded.n_images, folded.num_classes
    m = merge_detections(folded, folded.views, nms_thresh, nms_inclusive, max_dets, with_layout=True, capacity=folded.capacity,
                         method=method, sigma=sigma, min_score=min_score, vote_thresh=vote_thresh, vote_score=vote_score)
    out = MergedDetections([list(m[b * C:(b + 1) * C]) for b in range(B)])
    out._take_layout(m)
    out.num_classes = C
    out.folded = folded
    return out


def fold_views_numpy(lists, table, V, C):
    """`fold_views` restated in numpy float32 (host), operation for operation as include/dana_hip.h defines
    dana_detect_fold_views. lists: P = B * V * C arrays [k,5] in problem order p = (i * V + v) * C + c; table [B * V][>=5]
    = (fw, fh, flip, area_lo, area_hi) -> dict(dets: the P folded lists in list-major order q = (i * C + c) * V + v,
    src_row: int32 [k'] per list, the kept rows' indices in the input list, counts int32 [P] in q order, source: int64 [P],
    the input problem p of every q)."""
    V, C = int(V), int(C)
    table = np.asarray(table, np.float32)
    table = table.reshape(-1, table.shape[-1] if table.ndim > 1 else 5)
    P = len(lists)
    if V < 1 or C < 1 or P % (V * C) or table.shape[0] * C != P or table.shape[1] < 5:
        raise ValueError("fold_views_numpy: %d lists and %d table rows do not make images x %d views x %d lists" % (P, table.shape[0], V, C))
    one, zero = np.float32(1.0), np.float32(0.0)
    dets, rows, source = [None] * P, [None] * P, np.zeros(P, np.int64)
    for p in range(P):
        iv, c = divmod(p, C)
        i, v = divmod(iv, V)
        q = (i * C + c) * V + v
        fw, fh, flip, lo, hi = table[iv, :5]
        wm1, hm1 = fw - one, fh - one
        d = np.array(lists[p], dtype=np.float32).reshape(-1, 5)
        x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        if flip != 0:
            x1, x2 = wm1 - x2, wm1 - x1
        with np.errstate(invalid="ignore"):
            keep = (x1 <= wm1) & (y1 <= hm1) & (x2 >= zero) & (y2 >= zero)
            clip = lambda a, m: (lambda b: np.where(b > m, m, b))(np.where(a < zero, zero, a))  # noqa: E731
            x1, x2, y1, y2 = clip(x1, wm1), clip(x2, wm1), clip(y1, hm1), clip(y2, hm1)
            area = (x2 - x1 + one) * (y2 - y1 + one)
            keep &= (lo <= area) & (area < hi)
        assert area.dtype == np.float32
        dets[q] = np.stack((x1, y1, x2, y2, d[:, 4]), 1).astype(np.float32)[keep]
        rows[q] = np.nonzero(keep)[0].astype(np.int32)
        source[q] = p
    return dict(dets=dets, src_row=rows, counts=np.asarray([len(d) for d in dets], np.int32), source=source)


def fold_tiles_numpy(lists, table, V, C):
    """`fold_tiles` restated in numpy float32 (host), operation for operation as include/dana_hip.h defines
    dana_detect_fold_tiles: lists and the result as `fold_views_numpy`'s, table [B * V][>=13] = (fw, fh, flip, area_lo, area_hi,
    x_off, y_off, tw, th, lim_x1, lim_y1, lim_x2, lim_y2). Steps (a) - (d) -- tile test, seam rule on the unclipped box, clip to
    the tile, translate -- then `fold_views_numpy` on the translated rows; a row stays if both keep it."""
    V, C = int(V), int(C)
    table = np.asarray(table, np.float32)
    table = table.reshape(-1, table.shape[-1] if table.ndim > 1 else 13)
    P = len(lists)
    if V < 1 or C < 1 or P % (V * C) or table.shape[0] * C != P or table.shape[1] < 13:
        raise ValueError("fold_tiles_numpy: %d lists and %d table rows of %d columns do not make images x %d views x %d lists"
                         % (P, table.shape[0], table.shape[1], V, C))
    one, zero = np.float32(1.0), np.float32(0.0)
    moved, in_tile = [], []
    for p in range(P):
        x_off, y_off, tw, th, lx1, ly1, lx2, ly2 = table[p // C, 5:13]
        twm1, thm1 = tw - one, th - one
        d = np.array(lists[p], dtype=np.float32).reshape(-1, 5)
        x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        with np.errstate(invalid="ignore"):
            keep = (x1 <= twm1) & (y1 <= thm1) & (x2 >= zero) & (y2 >= zero)
            keep &= (x1 >= lx1) & (y1 >= ly1) & (x2 <= lx2) & (y2 <= ly2)
            clip = lambda a, m: (lambda b: np.where(b > m, m, b))(np.where(a < zero, zero, a))  # noqa: E731
            x1, x2, y1, y2 = clip(x1, twm1), clip(x2, twm1), clip(y1, thm1), clip(y2, thm1)
            x1, x2, y1, y2 = x1 + x_off, x2 + x_off, y1 + y_off, y2 + y_off
        assert x1.dtype == np.float32
        moved.append(np.stack((x1, y1, x2, y2, d[:, 4]), 1).astype(np.float32))
        in_tile.append(keep)
    # steps (1) - (5) on every translated row; a row of the result is one that also passed (a) and (b)
    r = fold_views_numpy(moved, table, V, C)
    for q, p in enumerate(r["source"]):
        sel = in_tile[p][r["src_row"][q]]
        r["dets"][q], r["src_row"][q] = r["dets"][q][sel], r["src_row"][q][sel]
    r["counts"] = np.asarray([len(d) for d in r["dets"]], np.int32)
    return r


def cap_per_image(cd, max_per_image=100):
    """The `max_per_image` cut of a Faster R-CNN test loop (inference.py:70) on the device: image b's num_classes lists of
    `cd` = detections_by_class(..., with_layout=True) merged by score with NMS off and cut to its best `max_per_image`
    rows. -> `MergedDetections` of B tensors; `group` is each row's class index, so
    `ev.add_packed(m.packed[:m.total], image_indices[m.list_index()], m.group)` appends the capped detections."""
    return merge_detections(cd, cd.num_classes, nms_thresh=None, max_dets=int(max_per_image), with_layout=True)


def as_gt_boxes(merged, im_info, labels=1, score_thresh=0.5, max_boxes=None):
    """Pseudo-labels as a train-mode forward takes them (fs_loader.py:325): `merged` = n detection lists, one per image
    (a `MergedDetections` / `ClassDetections` or a tuple (packed, counts, offsets)), im_info [n,3]. Image b's first
    `max_boxes` (default cfg.MAX_NUM_GT_BOXES) rows with score > score_thresh (0.5: plot_box's threshold, utils.py:304)
    become (x1, y1, x2, y2) * im_info[b][2] -- back to network-input coordinates, the inverse of inference.py:125 -- with
    label labels[b] (a number, or [n] values); zero rows pad the rest.
    -> (gt_boxes [n, max_boxes, 5] float32, num_boxes [n] int64), both on the device; nothing is read back."""
    packed, P, _, _, p_counts, p_offsets, alive = _packed_layout(merged, "as_gt_boxes")
    max_boxes = int(cfg.MAX_NUM_GT_BOXES if max_boxes is None else max_boxes)
    dev = packed.device
    im_info = ops._chk(im_info.reshape(-1, im_info.size(-1)).float().contiguous(), "im_info")
    if im_info.size(0) != P or im_info.size(1) < 3:
        raise ValueError("as_gt_boxes: %d lists need im_info [%d, 3], got %s" % (P, P, tuple(im_info.shape)))
    if isinstance(labels, torch.Tensor):
        lab = labels.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    else:
        lab = torch.full((P,), float(labels), dtype=torch.float32, device=dev)
    if lab.numel() != P:
        raise ValueError("as_gt_boxes: %d lists but %d labels" % (P, lab.numel()))
    gt_boxes = torch.empty((P, max_boxes, 5), dtype=torch.float32, device=dev)
    num_boxes = torch.empty((P,), dtype=torch.int64, device=dev)
    lib().call("dana_dets_to_gt_boxes", ops._p(packed), p_counts, p_offsets, ops._p(im_info), im_info.size(1), ops._p(lab), P,
               float(score_thresh), max_boxes, ops._p(gt_boxes), num_boxes.data_ptr(), ops._stream())
    del alive
    return gt_boxes, num_boxes


def _iou_rows(box, rest):
    """IoU of one box against rows, float64, legacy +1 widths (nms_cpu.cpp:30-60)"""
    area = (box[2] - box[0] + 1.) * (box[3] - box[1] + 1.)
    areas = (rest[:, 2] - rest[:, 0] + 1.) * (rest[:, 3] - rest[:, 1] + 1.)
    w = np.maximum(np.minimum(box[2], rest[:, 2]) - np.maximum(box[0], rest[:, 0]) + 1., 0.)
    h = np.maximum(np.minimum(box[3], rest[:, 3]) - np.maximum(box[1], rest[:, 1]) + 1., 0.)
    inter = w * h
    return inter / (area + areas - inter)


def merge_numpy(lists_per_problem, groups, nms_thresh, nms_inclusive=False, max_dets=0):
    """`merge_detections` restated in numpy (host): lists_per_problem = P arrays [k,5] (float32 values), list l merges
    problems l*groups .. l*groups + groups - 1. Concatenation, `np.argsort(-score, kind="stable")`, greedy NMS with +1
    widths in float64 (`>`, or `>=` with nms_inclusive; nms_thresh None: none), the first max_dets (0: all).
    -> dict(dets: list of float32 [K_l,5], group / row: lists of int32 [K_l], counts int32 [n], offsets int32 [n+1],
    margin: the smallest |IoU - nms_thresh| over every suppression decision taken -- a kept box against each later box not
    yet suppressed --, inf when there was none)."""
    groups = int(groups)
    P = len(lists_per_problem)
    if groups < 1 or P % groups:
        raise ValueError("merge_numpy: %d lists are not a multiple of groups = %d" % (P, groups))
    out_d, out_g, out_r, margin = [], [], [], np.inf
    for l in range(P // groups):
        parts = [np.asarray(lists_per_problem[l * groups + g], np.float32).reshape(-1, 5) for g in range(groups)]
        cat = np.concatenate(parts, 0)
        grp = np.concatenate([np.full(len(q), g, np.int32) for g, q in enumerate(parts)])
        row = np.concatenate([np.arange(len(q), dtype=np.int32) for q in parts])
        order = np.argsort(-cat[:, 4].astype(np.float64), kind="stable")
        n = order.size
        if nms_thresh is None:
            kept = np.arange(n)
        else:
            box = cat[order, :4].astype(np.float64)
            dead = np.zeros(n, bool)
            kept = []
            for i in range(n):
                if dead[i]:
                    continue
                kept.append(i)
                if max_dets > 0 and len(kept) >= max_dets:
                    break
                live = np.nonzero(~dead[i + 1:])[0] + i + 1
                if live.size:
                    iou = _iou_rows(box[i], box[live])
                    margin = min(margin, float(np.abs(iou - float(nms_thresh)).min()))
                    dead[live[(iou >= nms_thresh) if nms_inclusive else (iou > nms_thresh)]] = True
            kept = np.asarray(kept, np.int64)
        if max_dets > 0:
            kept = kept[:max_dets]
        sel = order[kept]
        out_d.append(cat[sel])
        out_g.append(grp[sel])
        out_r.append(row[sel])
    counts = np.asarray([len(d) for d in out_d], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return dict(dets=out_d, group=out_g, row=out_r, counts=counts, offsets=offsets, margin=margin)


def _iou32_rows(box, rest):
    """iou(box, rest[j]) for every row j in float32, one IEEE operation per written operation (numpy's elementwise float32
    operators round each result to float32): area = (x2 - x1 + 1) * (y2 - y1 + 1), w = max(min(x2) - max(x1) + 1, 0),
    inter = w * h, iou = inter / ((area(a) + area(b)) - inter) -- the exact-division branch of csrc/nms.hip's iou_suppress"""
    one, zero = np.float32(1.0), np.float32(0.0)
    box = np.asarray(box, np.float32)
    rest = np.asarray(rest, np.float32).reshape(-1, 4)
    area = (box[2] - box[0] + one) * (box[3] - box[1] + one)
    areas = (rest[:, 2] - rest[:, 0] + one) * (rest[:, 3] - rest[:, 1] + one)
    w = np.maximum(np.minimum(box[2], rest[:, 2]) - np.maximum(box[0], rest[:, 0]) + one, zero)
    h = np.maximum(np.minimum(box[3], rest[:, 3]) - np.maximum(box[1], rest[:, 1]) + one, zero)
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        out = inter / ((area + areas) - inter)
    assert out.dtype == np.float32
    return out


def _rel_gap(a, b):
    """|a - b| relative to |b| (absolute where b is 0), in float64"""
    a, b = float(a), float(b)
    return abs(a - b) / abs(b) if b != 0.0 else abs(a - b)


def merge_soft_numpy(lists_per_problem, groups, nms_thresh, nms_inclusive=False, max_dets=0, method="hard", sigma=0.5,
                     min_score=0.001, vote_thresh=None, vote_score="id"):
    """`merge_detections` with its soft-NMS / voting keywords restated in numpy (host), operation for operation as
    include/dana_hip.h defines dana_detect_merge_soft: float32 for the IoU and the linear decay, Python floats (doubles) for
    the Gaussian decay and the voting sums, explicit loops where an order is part of the definition. The parameters are
    rounded to float32 first, as the C call receives them. `method="hard"` is `merge_numpy`'s chain with the float32 IoU the
    device decides by (equal to merge_numpy wherever that one's margin is positive).
    -> what `merge_numpy` returns, plus votes: list of int32 [K_l] (None with voting off), and margin: a dict of
    pick: the smallest relative gap between the best and the second-best live working score over all picks (inf with fewer
    than two live rows), drop: the smallest relative |t - min_score| over all removal decisions, vote: the smallest
    |iou - vote_thresh| over all voter decisions -- how far the discrete outputs are from changing."""
    _soft_args("merge_soft_numpy", nms_thresh, method, sigma, min_score, vote_thresh, vote_score)
    groups = int(groups)
    P = len(lists_per_problem)
    if groups < 1 or P % groups:
        raise ValueError("merge_soft_numpy: %d lists are not a multiple of groups = %d" % (P, groups))
    nt = None if nms_thresh is None else np.float32(nms_thresh)
    ms = np.float32(min_score)
    dsigma = float(np.float32(sigma))
    vt = None if vote_thresh is None else np.float32(vote_thresh)
    one = np.float32(1.0)
    margin = dict(pick=np.inf, drop=np.inf, vote=np.inf)
    out_d, out_g, out_r, out_v = [], [], [], []
    for l in range(P // groups):
        parts = [np.asarray(lists_per_problem[l * groups + g], np.float32).reshape(-1, 5) for g in range(groups)]
        cat = np.concatenate(parts, 0)
        grp = np.concatenate([np.full(len(q), g, np.int32) for g, q in enumerate(parts)])
        row = np.concatenate([np.arange(len(q), dtype=np.int32) for q in parts])
        n = len(cat)
        box, s = cat[:, :4], cat[:, 4]
        limit = min(max_dets, n) if max_dets > 0 else n
        sel, emit_t = [], []
        if method == "hard":
            order = np.argsort(-s.astype(np.float64), kind="stable")
            if nt is None:
                sel = list(order[:limit])
            else:
                dead = np.zeros(n, bool)
                for pos in range(n):
                    if len(sel) >= limit:
                        break
                    if dead[pos]:
                        continue
                    sel.append(order[pos])
                    later = np.nonzero(~dead[pos + 1:])[0] + pos + 1
                    if later.size:
                        o = _iou32_rows(box[order[pos]], box[order[later]])
                        dead[later[(o >= nt) if nms_inclusive else (o > nt)]] = True
            emit_t = [s[j] for j in sel]
        else:
            t = s.copy()
            live = np.ones(n, bool)
            while live.any() and len(sel) < limit:
                idx = np.nonzero(live)[0]
                num = idx[~np.isnan(t[idx])]  # a NaN ranks behind every number
                i = int(num[np.argmax(t[num])]) if num.size else int(idx[0])  # (argmax: the first, i.e. lowest, index of the maximum)
                if num.size >= 2:
                    top = np.sort(t[num].astype(np.float64))[-2:]
                    margin["pick"] = min(margin["pick"], _rel_gap(top[0], top[1]))
                sel.append(i)
                emit_t.append(t[i])
                live[i] = False
                idx = np.nonzero(live)[0]
                if not idx.size:
                    break
                o = _iou32_rows(box[i], box[idx])
                if method == "linear":
                    hit = (o >= nt) if nms_inclusive else (o > nt)
                    t[idx[hit]] = t[idx[hit]] * (one - o[hit])
                else:
                    for j, oj in zip(idx, o):
                        t[j] = np.float32(float(t[j]) * math.exp(-float(oj * oj) / dsigma))
                gap = np.abs(t[idx].astype(np.float64) - float(ms)) / (abs(float(ms)) if ms != 0 else 1.0)
                if not np.isnan(gap).all():
                    margin["drop"] = min(margin["drop"], float(np.nanmin(gap)))
                live[idx[t[idx] < ms]] = False
        sel = np.asarray(sel, np.int64)
        d = cat[sel].copy()
        d[:, 4] = np.asarray(emit_t, np.float32)
        votes = None
        if vt is not None:
            votes = np.zeros(len(sel), np.int32)
            for k in range(len(sel)):
                o = _iou32_rows(d[k, :4], box)
                if n:
                    margin["vote"] = min(margin["vote"], float(np.abs(o.astype(np.float64) - float(vt)).min()))
                acc, wsum = [0.0, 0.0, 0.0, 0.0], 0.0
                for j in np.nonzero(o >= vt)[0]:  # ascending concatenation index; the order is part of the definition
                    sj = float(s[j])
                    for c in range(4):
                        acc[c] += sj * float(box[j, c])
                    wsum += sj
                    votes[k] += 1
                if wsum > 0.0:
                    d[k, :4] = [np.float32(a / wsum) for a in acc]
                if vote_score == "avg":
                    with np.errstate(divide="ignore", invalid="ignore"):
                        d[k, 4] = np.float32(np.float64(wsum) / np.float64(votes[k]))
        out_d.append(d)
        out_g.append(grp[sel])
        out_r.append(row[sel])
        out_v.append(votes)
    counts = np.asarray([len(d) for d in out_d], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return dict(dets=out_d, group=out_g, row=out_r, counts=counts, offsets=offsets, margin=margin,
                votes=None if vt is None else out_v)


def gt_boxes_numpy(lists, im_scale, labels, score_thresh=0.5, max_boxes=50):
    """`as_gt_boxes` restated in numpy float32 (host): the multiply is the same single fp32 operation"""
    n = len(lists)
    gt = np.zeros((n, max_boxes, 5), np.float32)
    num = np.zeros(n, np.int64)
    lab = np.broadcast_to(np.asarray(labels, np.float32), (n,))
    for b, d in enumerate(lists):
        d = np.asarray(d, np.float32).reshape(-1, 5)
        d = d[d[:, 4] > np.float32(score_thresh)][:max_boxes]
        gt[b, :len(d), :4] = d[:, :4] * np.float32(im_scale[b])
        gt[b, :len(d), 4] = lab[b]
        num[b] = len(d)
    return gt, num
