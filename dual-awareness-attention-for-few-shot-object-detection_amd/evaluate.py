"""Detection evaluation on the device: what `imdb.evaluate_detections(all_boxes, output_dir)` (inference.py:181) ends
in -- lib/datasets/voc_eval.py -- without the text files, the parse and the per-detection Python loop.

`DetectionEvaluator` accumulates detections across forwards in device buffers (no method reads from the device: the
row counts come from the host layout that post-processing has already read) and `compute()` gives per-class AP at every
IoU threshold in one C call (csrc/evaluate.hip: two radix sorts, one wavefront per (class, image) for the TP/FP
marking, one workgroup per (class, threshold) for the curves). All arithmetic is float64.

This is the VOC protocol: the TP/FP marking of voc_eval.py:165-199, the curves of :202-207, both `voc_ap` metrics of
:35-66. Thresholds 0.50:0.05:0.95 are ten `voc_eval` calls in one pass. That is NOT COCOeval: crowd regions, area ranges
and maxDets are not modelled there. The COCO protocol is the second half of this module (`CocoEvaluator`, below).

Defined where the reference is not, or differs:
  * equal scores within a class are ranked in arrival order (the reference's `np.argsort(-confidence)` is not stable);
  * a class without non-difficult ground truth (npos == 0) has AP = NaN under BOTH metrics (the reference: 0 under the
    11-point metric, NaN under the area metric) and `mean_ap()` averages the classes with npos > 0;
  * boxes are taken as given: pascal_voc.py:288-291 adds 1 to the detection coordinates before voc_eval sees them, so a
    caller that wants the reference's numbers adds it (`evaluate_all_boxes(..., add_one=True)` does).

`voc_numpy` is the same semantics restated in plain numpy float64 (host): the tests' yardstick, pinned to the reference
by tests/golden/eval_voc.npz.

The COCO protocol (`CocoEvaluator`, `eval_coco`, `evaluate_coco_boxes`, `coco_numpy`): what the COCO splits end in --
coco_split.py:287-298, `COCOeval.evaluate()`, `accumulate()`, `summarize()`, and the per-category table of
`_print_detection_eval_metrics` (:254-285) -- for iouType = 'bbox': AP@[.50:.95], AP50, AP75, AP small / medium / large,
AR@1/10/100. One C call (csrc/evaluate.hip: the same sorts and segment tables, one wavefront per (class, image) whose
lanes own the (area range, threshold) pairs, one workgroup per (class, area range, maxDets, threshold)), float64.

Defined where the reference is not: pycocotools is not part of the reference tree and is not installed, so nothing here
was generated from it. The protocol is pinned three ways instead: `coco_numpy` restates the published algorithm
(COCOeval `evaluateImg` / `accumulate` / `summarize` and maskApi's `bbIou`); hand-worked cases with known answers
(tests/test_coco_eval_host.py); and, on inputs where the two protocols must agree (pairwise disjoint ground truth, no
flags, one area range, no maxDets cut), `coco_numpy` is checked against the reference-pinned `voc_numpy`. Two choices:
  * objects are matched by index, not by annotation id: pycocotools' `dtm == 0` confusion over an annotation whose id is
    0 is not reproduced;
  * the rank is (class, score descending, image index, arrival): COCOeval's stable mergesort over the per-image lists.

Proposal recall (`ProposalRecallEvaluator`, `eval_proposal_recall`, `proposal_recall_numpy`): the stage in front of both
protocols -- py-faster-rcnn's `evaluate_recall`, which the reference still carries commented out (lib/datasets/
imdb.py:137-225) -- on the `rois` an eval-mode forward returns: proposals and ground truth matched one to one, greedily
(:193-210), the matched IoUs held against 0.50:0.05:0.95 (:214-221), averaged into AR (:223) per proposal budget
(`limit`, :187-188) and object-size range (`area`, :150-174). One C call (csrc/recall.hip: one workgroup per (unit, limit,
area range) for the matching, one thread per (limit, area range, pair) for the counts), float64 IoUs, integer counts.
A proposal list is made for one image under one class, so it is measured twice: on the image's objects of that class
(role 0) and, with others=True, on the image's other objects (role 1). ar[0] beside ar[1] is the selectivity the
attention in front of the RPN is there to buy.

Defined where the reference is not, or differs:
  * when a list has fewer candidates than the image has objects in range, the objects left over count as missed
    (IoU 0, no match): the reference's `assert (gt_ovr >= 0)` fires there;
  * the area is (x2 - x1 + 1) * (y2 - y1 + 1) unless the caller gives one (the reference reads the roidb's `seg_areas`);
  * crowd annotations are the caller's to leave out (:166-170 drops them through the roidb's overlaps).
`proposal_recall_numpy` restates the matrix procedure in numpy float64 (host): the tests' yardstick, itself checked
against hand-worked cases and an independent sorted sweep (tests/recall_cases.py).
"""
import numpy as np
import torch

from . import ops
from ._lib import lib

COCO_THRESHOLDS = tuple(float(x) for x in np.arange(0.5, 0.96, 0.05))  # voc_eval at ten `ovthresh` values


# ---- host restatement ----------------------------------------------------------------------------------------------------

def _iou_matrix(bb, gt):
    """voc_eval.py:174-187 for nd detections x ng boxes, float64, the reference's operation order"""
    bb = bb[:, None, :]
    gt = gt[None, :, :]
    ixmin = np.maximum(gt[..., 0], bb[..., 0])
    iymin = np.maximum(gt[..., 1], bb[..., 1])
    ixmax = np.minimum(gt[..., 2], bb[..., 2])
    iymax = np.minimum(gt[..., 3], bb[..., 3])
    iw = np.maximum(ixmax - ixmin + 1., 0.)
    ih = np.maximum(iymax - iymin + 1., 0.)
    inters = iw * ih
    uni = ((bb[..., 2] - bb[..., 0] + 1.) * (bb[..., 3] - bb[..., 1] + 1.) +
           (gt[..., 2] - gt[..., 0] + 1.) * (gt[..., 3] - gt[..., 1] + 1.) - inters)
    return inters / uni


def _ap_numpy(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            sel = rec >= t
            p = prec[sel].max() if sel.any() else 0.
            ap = ap + p / 11.
        return float(ap)
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]  # the precision envelope
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def voc_numpy(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls, iou_thr, use_07_metric=False):
    """The evaluator's semantics in numpy float64: per (class, image) greedy marking in rank order, scattered to the
    global rank, cumulative sums, AP. -> dict(order [n], cls_offsets [C+1], tpfp uint8 [T,n] (1 TP, 2 FP, 0 ignored),
    rec / prec float64 [T,n] by rank, ap [C,T], npos [C]). Rows with ids out of range take no part (ranked last)."""
    det = np.asarray(det, np.float32).reshape(-1, 5)
    det_img = np.asarray(det_img, np.int64).reshape(-1)
    det_cls = np.asarray(det_cls, np.int64).reshape(-1)
    gt_box = np.asarray(gt_box, np.float32).reshape(-1, 4)
    gt_img = np.asarray(gt_img, np.int64).reshape(-1)
    gt_cls = np.asarray(gt_cls, np.int64).reshape(-1)
    gt_difficult = np.asarray(gt_difficult).reshape(-1).astype(bool)
    thr = np.asarray(iou_thr, np.float64).reshape(-1)
    n, T = det.shape[0], thr.size
    ok = (det_cls >= 0) & (det_cls < n_cls) & (det_img >= 0) & (det_img < n_img)
    cls_key = np.where(ok, det_cls, n_cls)
    order = np.lexsort((np.arange(n), -det[:, 4].astype(np.float64), cls_key)).astype(np.int64)  # stable in arrival
    cls_offsets = np.searchsorted(cls_key[order], np.arange(n_cls + 1), side="left").astype(np.int64)
    gok = (gt_cls >= 0) & (gt_cls < n_cls) & (gt_img >= 0) & (gt_img < n_img)
    tpfp = np.zeros((T, n), np.uint8)
    rec = np.full((T, n), np.nan)
    prec = np.full((T, n), np.nan)
    ap = np.zeros((n_cls, T))
    npos = np.zeros(n_cls, np.int64)
    gt64 = gt_box.astype(np.float64)
    det64 = det[:, :4].astype(np.float64)
    for c in range(n_cls):
        gsel = np.nonzero(gok & (gt_cls == c))[0]
        npos[c] = int((~gt_difficult[gsel]).sum())
        r0, r1 = int(cls_offsets[c]), int(cls_offsets[c + 1])
        ranks = np.arange(r0, r1)
        imgs = det_img[order[r0:r1]]
        by_img = np.argsort(imgs, kind="stable")  # each image's ranks stay ascending
        bounds = np.nonzero(np.diff(imgs[by_img]))[0] + 1
        g_img = gt_img[gsel]
        for seg in np.split(by_img, bounds) if r1 > r0 else []:
            im = imgs[seg[0]]
            gi = gsel[g_img == im]  # arrival order: the order of the image's objects
            seg_ranks = ranks[seg]
            if gi.size == 0:
                tpfp[:, seg_ranks] = 2  # ovmax = -inf
                continue
            ov = _iou_matrix(det64[order[seg_ranks]], gt64[gi])
            ovmax = ov.max(axis=1)
            jmax = ov.argmax(axis=1)  # the lowest index among equal maxima
            diff = gt_difficult[gi]
            for t in range(T):
                taken = np.zeros(gi.size, bool)
                for d in range(seg_ranks.size):
                    code = 2
                    if ovmax[d] > thr[t]:
                        j = jmax[d]
                        if diff[j]:
                            code = 0
                        elif not taken[j]:
                            taken[j] = True
                            code = 1
                    tpfp[t, seg_ranks[d]] = code
        for t in range(T):
            tp = np.cumsum(tpfp[t, r0:r1] == 1).astype(np.float64)
            fp = np.cumsum(tpfp[t, r0:r1] == 2).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rc = tp / float(npos[c])
            pr = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            rec[t, r0:r1], prec[t, r0:r1] = rc, pr
            ap[c, t] = _ap_numpy(rc, pr, use_07_metric) if npos[c] > 0 else np.nan
    return dict(order=order, cls_offsets=cls_offsets, tpfp=tpfp, rec=rec, prec=prec, ap=ap, npos=npos)


def min_iou_margin(det, det_img, det_cls, gt_box, gt_img, gt_cls, n_img, iou_thr):
    """min |IoU - thr| over every (detection, same class-and-image box, threshold): fixtures assert it stays above 1e-9,
    so that a last-bit difference in one double division cannot flip a decision"""
    det = np.asarray(det, np.float32).reshape(-1, 5)
    gt_box = np.asarray(gt_box, np.float32).reshape(-1, 4)
    thr = np.asarray(iou_thr, np.float64).reshape(-1)
    dseg = np.asarray(det_cls, np.int64) * n_img + np.asarray(det_img, np.int64)
    gseg = np.asarray(gt_cls, np.int64) * n_img + np.asarray(gt_img, np.int64)
    gorder = np.argsort(gseg, kind="stable")
    gs = gseg[gorder]
    dorder = np.argsort(dseg, kind="stable")
    ds = dseg[dorder]
    margin = np.inf
    starts = np.nonzero(np.diff(ds, prepend=ds[:1] - 1))[0] if ds.size else np.zeros(0, np.int64)
    ends = np.append(starts[1:], ds.size)
    for a, b in zip(starts, ends):
        lo, hi = np.searchsorted(gs, ds[a], "left"), np.searchsorted(gs, ds[a], "right")
        if hi == lo:
            continue
        ov = _iou_matrix(det[dorder[a:b], :4].astype(np.float64), gt_box[gorder[lo:hi]].astype(np.float64))
        margin = min(margin, float(np.abs(ov[:, :, None] - thr[None, None, :]).min()))
    return margin


# ---- device ----------------------------------------------------------------------------------------------------------------

def radix_sort_pairs(keys, vals, key_bits=64):
    """The evaluator's stable LSD radix sort on its own (debug entry point): int64 keys (read as unsigned) and int32
    values -> (sorted keys, values), ascending in the low `key_bits` bits, equal keys in input order."""
    keys = ops._chk(keys.contiguous(), "keys", torch.int64)
    vals = ops._chk(vals.contiguous(), "vals", torch.int32)
    n = keys.numel()
    if vals.numel() != n:
        raise ValueError("radix_sort_pairs: %d keys, %d values" % (n, vals.numel()))
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    ws = ops._ws(lib().query("dana_debug_radix_sort_workspace_bytes", n), keys.device)
    lib().call("dana_debug_radix_sort_pairs", ops._p(keys), ops._p(vals), ops._p(ko), ops._p(vo), n, int(key_bits),
               ops._p(ws), ws.numel(), ops._stream())
    return ko, vo


def eval_ap(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls, iou_thr, use_07_metric=False,
            curves=False):
    """One `dana_eval_ap` call on device tensors (det [n,5] float32, ids int32, gt_difficult uint8, iou_thr float64 [T])
    -> EvalResult. No synchronisation, no device-to-host copy."""
    det = ops._chk(det, "det")
    dev = det.device
    n, g, T = det.size(0), gt_box.size(0), iou_thr.numel()
    ops._chk(det_img, "det_img", torch.int32), ops._chk(det_cls, "det_cls", torch.int32)
    ops._chk(gt_box, "gt_box"), ops._chk(gt_img, "gt_img", torch.int32), ops._chk(gt_cls, "gt_cls", torch.int32)
    ops._chk(gt_difficult, "gt_difficult", torch.uint8), ops._chk(iou_thr, "iou_thr", torch.float64)
    if det_img.numel() != n or det_cls.numel() != n or gt_img.numel() != g or gt_cls.numel() != g or gt_difficult.numel() != g:
        raise ValueError("eval_ap: id tensors do not match %d detections / %d ground-truth boxes" % (n, g))
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    cls_offsets = torch.empty((n_cls + 1,), dtype=torch.int32, device=dev)
    tpfp = torch.empty((T, n), dtype=torch.uint8, device=dev)
    rec = torch.empty((T, n), dtype=torch.float64, device=dev) if curves else None
    prec = torch.empty((T, n), dtype=torch.float64, device=dev) if curves else None
    ap = torch.empty((n_cls, T), dtype=torch.float64, device=dev)
    npos = torch.empty((n_cls,), dtype=torch.int32, device=dev)
    ws = ops._ws(lib().query("dana_eval_ap_workspace_bytes", n, g, int(n_img), int(n_cls), T), dev)
    lib().call("dana_eval_ap", ops._p(det), ops._p(det_img), ops._p(det_cls), n, ops._p(gt_box), ops._p(gt_img),
               ops._p(gt_cls), ops._p(gt_difficult), g, int(n_img), int(n_cls), ops._p(iou_thr), T,
               int(bool(use_07_metric)), ops._p(order), ops._p(cls_offsets), ops._p(tpfp), ops._p(rec), ops._p(prec),
               ops._p(ap), ops._p(npos), ops._p(ws), ws.numel(), ops._stream())
    return EvalResult(ap, npos, order, cls_offsets, tpfp if curves else None, rec, prec, iou_thr)


class EvalResult:
    """Device tensors of one `compute()`: ap [C,T] float64 (NaN where npos == 0), npos [C] int32, order [n] (detection
    row by rank) and cls_offsets [C+1] (class c = ranks cls_offsets[c]:cls_offsets[c+1]); with curves also tpfp uint8
    [T,n] (1 TP, 2 FP, 0 matched a difficult box) and rec / prec float64 [T,n], all by rank."""

    def __init__(self, ap, npos, order, cls_offsets, tpfp, rec, prec, iou_thresholds):
        self.ap, self.npos, self.order, self.cls_offsets = ap, npos, order, cls_offsets
        self.tpfp, self.rec, self.prec, self.iou_thresholds = tpfp, rec, prec, iou_thresholds
        self._host_offsets = None

    def mean_ap(self):
        """-> [T] float64 device tensor: the mean over the classes that have non-difficult ground truth"""
        has = (self.npos > 0).to(torch.float64).unsqueeze(1)
        return torch.where(has > 0, self.ap, torch.zeros_like(self.ap)).sum(0) / has.sum(0)

    def class_curves(self, c, t=0):
        """-> (rec, prec) views of class c at threshold index t (reads cls_offsets from the device once)"""
        if self.rec is None:
            raise ValueError("class_curves needs compute(curves=True)")
        if self._host_offsets is None:
            self._host_offsets = self.cls_offsets.cpu()
        a, b = int(self._host_offsets[c]), int(self._host_offsets[c + 1])
        return self.rec[t, a:b], self.prec[t, a:b]


def _host_ints(x):
    """host integers (list / numpy / CPU tensor) -> numpy int32, or None for a device tensor"""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            return None
        x = x.numpy()
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)


class _DetectionStore:
    """What both evaluators share: the detections accumulated across forwards in device buffers (doubling growth), fed
    by `add_packed`, `add_batched` and `add_by_class`. No method reads from the device. A subclass sets `device` and
    `num_classes`, calls `_reset_detections()` from its `reset()` and keeps its own ground truth."""

    def _reset_detections(self):
        self.num_rows = 0
        self.num_images = 0
        self._cap = 0
        self._det = self._img = self._cls = None

    # -- growth: doubling, so that appends cost amortised O(rows)
    def _reserve(self, rows):
        need = self.num_rows + rows
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 1024)
        det = torch.empty((cap, 5), dtype=torch.float32, device=self.device)
        img = torch.empty((cap,), dtype=torch.int32, device=self.device)
        cls = torch.empty((cap,), dtype=torch.int32, device=self.device)
        if self.num_rows:
            det[:self.num_rows].copy_(self._det[:self.num_rows])
            img[:self.num_rows].copy_(self._img[:self.num_rows])
            cls[:self.num_rows].copy_(self._cls[:self.num_rows])
        self._det, self._img, self._cls, self._cap = det, img, cls, cap

    def _dev(self, x, dtype):
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return x.to(device=self.device, dtype=dtype).contiguous()

    def add_packed(self, dets, img_ids, cls_ids, num_images=None):
        """The primitive (and what a caller all-gathers across ranks): dets [k,5] = (x1,y1,x2,y2,score) with per-row
        image and class ids. Ids on the host raise the image count by themselves; with ids on the device pass
        `num_images` (an upper bound of image index + 1), because nothing is read back."""
        dets = self._dev(dets, torch.float32).reshape(-1, 5)
        k = dets.size(0)
        host_img = _host_ints(img_ids)
        if num_images is not None:
            self.num_images = max(self.num_images, int(num_images))
        elif host_img is None:
            raise ValueError("add_packed: img_ids live on the device; pass num_images (the evaluator reads nothing back)")
        elif host_img.size:
            self.num_images = max(self.num_images, int(host_img.max()) + 1)
        img = self._dev(img_ids, torch.int32).reshape(-1)
        cls = self._dev(cls_ids, torch.int32).reshape(-1)
        if img.numel() != k or cls.numel() != k:
            raise ValueError("add_packed: %d rows, %d image ids, %d class ids" % (k, img.numel(), cls.numel()))
        if k == 0:
            return
        self._reserve(k)
        a = self.num_rows
        self._det[a:a + k].copy_(dets)
        self._img[a:a + k].copy_(img)
        self._cls[a:a + k].copy_(cls)
        self.num_rows += k

    def add_batched(self, dets_packed, counts, offsets, image_indices, class_indices):
        """What `postprocess.detections_batched(..., with_layout=True)` returns -- the per-problem detections (the list
        of views, or the one packed buffer they are views of), host `counts` [P] and `offsets` [P+1] -- with the host
        image index and class index of each problem (an int applies to all). One upload of the small tables, one
        append launch (dana_eval_append); nothing is read back."""
        counts = _host_ints(counts)
        offsets = _host_ints(offsets)
        if counts is None or offsets is None:
            raise ValueError("add_batched: counts / offsets are the HOST layout tensors of post-processing")
        P = counts.size
        img = _host_ints(image_indices)
        cls = _host_ints(class_indices)
        if img is None or cls is None:
            raise ValueError("add_batched: image / class indices are host integers")
        img = np.repeat(img, P) if img.size == 1 and P != 1 else img
        cls = np.repeat(cls, P) if cls.size == 1 and P != 1 else cls
        if offsets.size < P or img.size != P or cls.size != P or (counts < 0).any():
            raise ValueError("add_batched: %d problems need as many counts, offsets, image and class indices" % P)
        if isinstance(dets_packed, (list, tuple)):
            parts = [d.reshape(-1, 5) for d in dets_packed]
            if len(parts) != P or any(int(d.size(0)) != int(c) for d, c in zip(parts, counts)):
                raise ValueError("add_batched: the detection list does not match counts")
            src_off = np.concatenate(([0], np.cumsum(counts[:-1], dtype=np.int64))).astype(np.int32) if P else counts
            src = torch.cat(parts, 0) if P else torch.empty((0, 5), device=self.device)
        else:
            src, src_off = dets_packed.reshape(-1, 5), offsets[:P]
            if P and int((src_off.astype(np.int64) + counts).max()) > src.size(0):
                raise ValueError("add_batched: offsets + counts run past the packed buffer")
        src = ops._chk(self._dev(src, torch.float32), "dets_packed")
        rows = int(counts.sum(dtype=np.int64))
        if P and img.size:
            self.num_images = max(self.num_images, int(img.max()) + 1)
        if rows == 0:
            return
        self._reserve(rows)
        dst_off = np.concatenate(([0], np.cumsum(counts, dtype=np.int64))).astype(np.int32)
        table = ops._h2d_int32(np.concatenate((dst_off, src_off.astype(np.int32), img, cls)), self.device)
        base = table.data_ptr()
        lib().call("dana_eval_append", ops._p(src), base, base + 4 * (P + 1), base + 4 * (2 * P + 1),
                   base + 4 * (3 * P + 1), P, rows, ops._p(self._det), ops._p(self._img), ops._p(self._cls),
                   self.num_rows, self._cap, ops._stream())
        self.num_rows += rows

    def add_by_class(self, dets_by_class, image_indices):
        """What `postprocess.detections_by_class(..., with_layout=True)` returns for B images (dets[b][c], problem
        p = b*C + c), with the B host image indices. The plain nested list (with_layout=False) works too, through one
        concatenation on the device."""
        img = _host_ints(image_indices)
        if img is None:
            raise ValueError("add_by_class: image indices are host integers")
        B = len(dets_by_class)
        C = self.num_classes
        if img.size != B or any(len(row) != C for row in dets_by_class):
            raise ValueError("add_by_class: need dets[b][c] for %d images x %d classes" % (img.size, C))
        p_img = np.repeat(img, C)
        p_cls = np.tile(np.arange(C, dtype=np.int32), B)
        packed = getattr(dets_by_class, "packed", None)
        if packed is not None:
            return self.add_batched(packed, dets_by_class.counts, dets_by_class.offsets, p_img, p_cls)
        flat = [d for row in dets_by_class for d in row]
        counts = np.asarray([int(d.shape[0]) for d in flat], np.int32)
        offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        return self.add_batched(flat, counts, offsets, p_img, p_cls)

    def _detections(self):
        """-> (det [n,5], img [n], cls [n]): the rows added so far"""
        n = self.num_rows
        if n:
            return self._det[:n], self._img[:n], self._cls[:n]
        ids = torch.empty((0,), dtype=torch.int32, device=self.device)
        return torch.empty((0, 5), dtype=torch.float32, device=self.device), ids, ids


class DetectionEvaluator(_DetectionStore):
    """VOC-protocol evaluator living on `device`. Classes are 0..num_classes-1, images are the caller's indices."""

    def __init__(self, num_classes, iou_thresholds=(0.5,), use_07_metric=False, device="cuda"):
        self.num_classes = int(num_classes)
        thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
        if self.num_classes < 1 or not 1 <= thr.size <= 16:
            raise ValueError("DetectionEvaluator: num_classes >= 1 and 1..16 IoU thresholds")
        self.use_07_metric = bool(use_07_metric)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DetectionEvaluator lives on a CUDA (HIP) device: this build has no CPU path")
        self.iou_thresholds = torch.from_numpy(thr).to(self.device)
        self.reset()

    def reset(self):
        self._reset_detections()
        self._gt = []  # (boxes [k,4] float32, image ids [k] int32, labels [k] int32, difficult [k] uint8) on the device
        self._gt_cat = None

    def add_ground_truth(self, image_index, boxes, labels, difficult=None):
        """the objects of one image: boxes [k,4] (x1,y1,x2,y2), labels [k] class indices, difficult [k] (default none)"""
        boxes = self._dev(boxes, torch.float32).reshape(-1, 4)
        k = boxes.size(0)
        labels = self._dev(labels, torch.int32).reshape(-1)
        diff = (torch.zeros((k,), dtype=torch.uint8, device=self.device) if difficult is None
                else (self._dev(difficult, torch.int32).reshape(-1) != 0).to(torch.uint8))
        if labels.numel() != k or diff.numel() != k:
            raise ValueError("add_ground_truth: %d boxes, %d labels, %d difficult flags" % (k, labels.numel(), diff.numel()))
        image_index = int(image_index)
        if image_index < 0:
            raise ValueError("add_ground_truth: negative image index")
        self.num_images = max(self.num_images, image_index + 1)
        self._gt.append((boxes, torch.full((k,), image_index, dtype=torch.int32, device=self.device), labels, diff))
        self._gt_cat = None

    def add_ground_truth_packed(self, boxes, img_ids, labels, difficult=None, num_images=None):
        """the objects of many images at once, with per-row image ids (the ground-truth counterpart of `add_packed`;
        ids on the device need `num_images`)"""
        boxes = self._dev(boxes, torch.float32).reshape(-1, 4)
        k = boxes.size(0)
        host_img = _host_ints(img_ids)
        if num_images is not None:
            self.num_images = max(self.num_images, int(num_images))
        elif host_img is None:
            raise ValueError("add_ground_truth_packed: img_ids live on the device; pass num_images")
        elif host_img.size:
            self.num_images = max(self.num_images, int(host_img.max()) + 1)
        img = self._dev(img_ids, torch.int32).reshape(-1)
        labels = self._dev(labels, torch.int32).reshape(-1)
        diff = (torch.zeros((k,), dtype=torch.uint8, device=self.device) if difficult is None
                else (self._dev(difficult, torch.int32).reshape(-1) != 0).to(torch.uint8))
        if img.numel() != k or labels.numel() != k or diff.numel() != k:
            raise ValueError("add_ground_truth_packed: %d boxes need as many image ids, labels and flags" % k)
        self._gt.append((boxes, img, labels, diff))
        self._gt_cat = None

    def _ground_truth(self):
        if self._gt_cat is None:
            if self._gt:
                self._gt_cat = tuple(torch.cat([g[i] for g in self._gt], 0).contiguous() for i in range(4))
            else:
                self._gt_cat = (torch.empty((0, 4), dtype=torch.float32, device=self.device),
                                torch.empty((0,), dtype=torch.int32, device=self.device),
                                torch.empty((0,), dtype=torch.int32, device=self.device),
                                torch.empty((0,), dtype=torch.uint8, device=self.device))
        return self._gt_cat

    def compute(self, curves=False):
        """-> EvalResult (device tensors; nothing is synchronised or read back here)"""
        gbox, gimg, gcls, gdiff = self._ground_truth()
        n = self.num_rows
        if n:
            det, img, cls = self._det[:n], self._img[:n], self._cls[:n]
        else:
            det = torch.empty((0, 5), dtype=torch.float32, device=self.device)
            img = cls = torch.empty((0,), dtype=torch.int32, device=self.device)
        return eval_ap(det, img, cls, gbox, gimg, gcls, gdiff, max(self.num_images, 1), self.num_classes,
                       self.iou_thresholds, self.use_07_metric, curves)


def evaluate_all_boxes(all_boxes, ground_truth, iou_thresholds=(0.5,), use_07_metric=False, device="cuda", add_one=False,
                       curves=False):
    """Drop-in for `imdb.evaluate_detections(all_boxes, output_dir)` (inference.py:181): all_boxes[j][i] is the [k,5]
    numpy array of class j on image i (an empty list where nothing was detected), ground_truth[i] = (boxes [k,4],
    labels [k] indexing all_boxes' j, difficult [k] or None). Every class j of all_boxes is evaluated; a background
    class 0 the caller leaves empty comes out with npos == 0 and AP = NaN, outside `mean_ap()`. add_one=True adds 1 to
    the detection coordinates first, as pascal_voc.py:288-291 does when it writes them. -> EvalResult"""
    C = len(all_boxes)
    n_img = len(ground_truth)
    ev = DetectionEvaluator(C, iou_thresholds, use_07_metric, device)
    rows, imgs, clss = [], [], []
    for j in range(C):
        for i in range(len(all_boxes[j])):
            d = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            if d.shape[0]:
                rows.append(d)
                imgs.append(np.full(d.shape[0], i, np.int32))
                clss.append(np.full(d.shape[0], j, np.int32))
            n_img = max(n_img, i + 1)
    for i, gt in enumerate(ground_truth):
        boxes, labels = gt[0], gt[1]
        ev.add_ground_truth(i, boxes, labels, gt[2] if len(gt) > 2 else None)
    if rows:
        d = np.concatenate(rows, 0)
        if add_one:
            d = d.copy()
            d[:, :4] += 1.
        ev.add_packed(d, np.concatenate(imgs), np.concatenate(clss), num_images=n_img)
    ev.num_images = max(ev.num_images, n_img)
    return ev.compute(curves=curves)


# ==== the COCO protocol ======================================================================================================

COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)  # COCOeval's Params
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_AREA_RNG = np.asarray([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
COCO_MAX_DETS = (1, 10, 100)
COCO_EPS = float(np.spacing(1))  # 2^-52
COCO_SUMMARY_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small",
                      "AR_medium", "AR_large")


def _coco_params(iou_thrs, rec_thrs, area_rng, max_dets):
    """-> the four parameter arrays, checked against what the kernels take"""
    iou = np.ascontiguousarray(np.asarray(COCO_IOU_THRS if iou_thrs is None else iou_thrs, np.float64).reshape(-1))
    rec = np.ascontiguousarray(np.asarray(COCO_REC_THRS if rec_thrs is None else rec_thrs, np.float64).reshape(-1))
    area = np.ascontiguousarray(np.asarray(COCO_AREA_RNG if area_rng is None else area_rng, np.float64).reshape(-1, 2))
    md = np.ascontiguousarray(np.asarray(COCO_MAX_DETS if max_dets is None else max_dets, np.int64).reshape(-1))
    if not (1 <= iou.size <= 16 and 1 <= rec.size <= 128 and 1 <= area.shape[0] <= 4 and 1 <= md.size <= 4):
        raise ValueError("COCO parameters: 1..16 iou_thrs, 1..128 rec_thrs, 1..4 area ranges, 1..4 max_dets")
    if (np.diff(rec) < 0).any() or (np.diff(md) < 0).any() or md[0] < 1 or md[-1] >= 1 << 30:
        raise ValueError("COCO parameters: rec_thrs and max_dets ascend, max_dets >= 1")
    return iou, rec, area, md.astype(np.int32)


def _coco_is_default(iou, rec, area, md):
    return (np.array_equal(iou, COCO_IOU_THRS) and np.array_equal(rec, COCO_REC_THRS) and
            np.array_equal(area, COCO_AREA_RNG) and np.array_equal(md, np.asarray(COCO_MAX_DETS)))


def _bb_iou(d, g, crowd):
    """maskApi bbIou: d [nd,4], g [ng,4] as (x, y, w, h) float64, crowd [ng] bool -> [nd,ng]"""
    d = d[:, None, :]
    g = g[None, :, :]
    iw = np.minimum(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.maximum(d[..., 0], g[..., 0])
    ih = np.minimum(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.maximum(d[..., 1], g[..., 1])
    i = iw * ih
    da = d[..., 2] * d[..., 3]
    u = np.where(crowd[None, :], np.broadcast_to(da, i.shape), da + g[..., 2] * g[..., 3] - i)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = i / u
    return np.where((iw <= 0) | (ih <= 0), 0., o)


def _last_argmax(x):
    """x [..., ng] -> (max, the LAST index holding it) along the last axis"""
    ng = x.shape[-1]
    j = ng - 1 - np.argmax(x[..., ::-1], axis=-1)
    return np.take_along_axis(x, j[..., None], -1)[..., 0], j


def coco_numpy(det, det_img, det_cls, gt_bbox, gt_img, gt_cls, n_img, n_cls, gt_iscrowd=None, gt_area=None,
               gt_ignore=None, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=None):
    """The COCO evaluator's semantics in numpy float64 (host). det [n,5] = (x1,y1,x2,y2,score), gt_bbox [g,4] =
    (x,y,w,h). -> dict(order [n], cls_offsets [K+1], segpos [n] by rank (-1: takes no part), codes uint8 [A,T,n] by rank
    (1 TP, 2 FP, 0 ignored, 3 past max_dets[-1] or no part), matched [A,T,n] by rank (the ground-truth row matched, -1),
    npig [K,A], precision / scores [T,R,K,A,M], recall [T,K,A,M])."""
    iou_t, rec_t, area_r, md = _coco_params(iou_thrs, rec_thrs, area_rng, max_dets)
    det = np.asarray(det, np.float32).reshape(-1, 5)
    det_img = np.asarray(det_img, np.int64).reshape(-1)
    det_cls = np.asarray(det_cls, np.int64).reshape(-1)
    gt_bbox = np.asarray(gt_bbox, np.float32).reshape(-1, 4)
    gt_img = np.asarray(gt_img, np.int64).reshape(-1)
    gt_cls = np.asarray(gt_cls, np.int64).reshape(-1)
    n, g = det.shape[0], gt_bbox.shape[0]
    T, R, A, M = iou_t.size, rec_t.size, area_r.shape[0], md.size
    K = int(n_cls)
    gt64 = gt_bbox.astype(np.float64)
    crowd = np.zeros(g, bool) if gt_iscrowd is None else np.asarray(gt_iscrowd).reshape(-1).astype(bool)
    ign = np.zeros(g, bool) if gt_ignore is None else np.asarray(gt_ignore).reshape(-1).astype(bool)
    area = gt64[:, 2] * gt64[:, 3] if gt_area is None else np.asarray(gt_area, np.float64).reshape(-1)
    gt_ig = (ign | crowd)[None, :] | (area[None, :] < area_r[:, :1]) | (area[None, :] > area_r[:, 1:])  # [A,g]
    d64 = det[:, :4].astype(np.float64)
    dbox = np.stack((d64[:, 0], d64[:, 1], d64[:, 2] - d64[:, 0] + 1., d64[:, 3] - d64[:, 1] + 1.), 1)
    darea = dbox[:, 2] * dbox[:, 3]
    d_out = (darea[None, :] < area_r[:, :1]) | (darea[None, :] > area_r[:, 1:])  # [A,n]
    score = det[:, 4].astype(np.float64)
    thr = np.minimum(iou_t, 1 - 1e-10)

    ok = (det_cls >= 0) & (det_cls < K) & (det_img >= 0) & (det_img < n_img)
    cls_key = np.where(ok, det_cls, K)
    order = np.lexsort((np.arange(n), det_img, -score, cls_key)).astype(np.int64)
    cls_offsets = np.searchsorted(cls_key[order], np.arange(K + 1), side="left").astype(np.int64)
    gok = (gt_cls >= 0) & (gt_cls < K) & (gt_img >= 0) & (gt_img < n_img)
    segpos = np.full(n, -1, np.int64)
    codes = np.full((A, T, n), 3, np.uint8)
    matched = np.full((A, T, n), -1, np.int64)
    npig = np.zeros((K, A), np.int64)
    precision = -np.ones((T, R, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        gsel = np.nonzero(gok & (gt_cls == k))[0]
        npig[k] = (~gt_ig[:, gsel]).sum(1)
        r0, r1 = int(cls_offsets[k]), int(cls_offsets[k + 1])
        ranks = np.arange(r0, r1)
        imgs = det_img[order[r0:r1]]
        by_img = np.argsort(imgs, kind="stable")  # each image's ranks stay ascending: by score, then arrival
        bounds = np.nonzero(np.diff(imgs[by_img]))[0] + 1
        g_img = gt_img[gsel]
        for seg in np.split(by_img, bounds) if r1 > r0 else []:
            gi = gsel[g_img == imgs[seg[0]]]  # arrival order
            seg_ranks = ranks[seg]
            segpos[seg_ranks] = np.arange(seg_ranks.size)
            seg_ranks = seg_ranks[:md[-1]]
            rows = order[seg_ranks]
            ng = gi.size
            if ng == 0:
                codes[:, :, seg_ranks] = np.where(d_out[:, rows], 0, 2)[:, None, :]
                continue
            ious = _bb_iou(dbox[rows], gt64[gi], crowd[gi])
            ig = gt_ig[:, gi][:, None, :]  # [A,1,ng]
            cr = crowd[gi][None, None, :]
            taken = np.zeros((A, T, ng), bool)
            aa, tt = np.meshgrid(np.arange(A), np.arange(T), indexing="ij")
            for d in range(seg_ranks.size):
                v = ious[d][None, None, :]
                reach = v >= thr[None, :, None]
                best_ni, j_ni = _last_argmax(np.where(~ig & ~taken & reach, v, -1.))
                best_ig, j_ig = _last_argmax(np.where(ig & (cr | ~taken) & reach, v, -1.))
                has_ni, has_ig = best_ni >= 0, best_ig >= 0
                j = np.where(has_ni, j_ni, j_ig)
                hit = has_ni | has_ig
                taken[aa[hit], tt[hit], j[hit]] = True
                codes[:, :, seg_ranks[d]] = np.where(has_ni, 1, np.where(has_ig | d_out[:, rows[d]][:, None], 0, 2))
                matched[:, :, seg_ranks[d]] = np.where(hit, gi[j], -1)
        sc = score[order[r0:r1]]
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m in range(M):
                inside = segpos[r0:r1] < md[m]
                for t in range(T):
                    c = codes[a, t, r0:r1]
                    keep = inside & ((c == 1) | (c == 2))
                    tp = np.cumsum(c[keep] == 1).astype(np.float64)
                    fp = np.cumsum(c[keep] == 2).astype(np.float64)
                    nd = tp.size
                    rc = tp / float(npig[k, a])
                    pr = tp / (fp + tp + COCO_EPS)
                    recall[t, k, a, m] = rc[-1] if nd else 0.
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, rec_t, side="left")
                    q, ss = np.zeros(R), np.zeros(R)
                    q[inds < nd] = pr[inds[inds < nd]]
                    ss[inds < nd] = sc[keep][inds[inds < nd]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return dict(order=order, cls_offsets=cls_offsets, segpos=segpos, codes=codes, matched=matched, npig=npig,
                precision=precision, recall=recall, scores=scores)


def coco_min_iou_margin(det, det_img, det_cls, gt_bbox, gt_img, gt_cls, n_img, iou_thrs, gt_iscrowd=None):
    """min |bbIou - min(thr, 1 - 1e-10)| over every (detection, same class-and-image object, threshold): seeded cases assert
    it stays above 1e-9, so that a last-bit difference in one double division cannot flip a decision"""
    det = np.asarray(det, np.float32).reshape(-1, 5)
    gt64 = np.asarray(gt_bbox, np.float32).reshape(-1, 4).astype(np.float64)
    g = gt64.shape[0]
    crowd = np.zeros(g, bool) if gt_iscrowd is None else np.asarray(gt_iscrowd).reshape(-1).astype(bool)
    thr = np.minimum(np.asarray(iou_thrs, np.float64).reshape(-1), 1 - 1e-10)
    d64 = det[:, :4].astype(np.float64)
    dbox = np.stack((d64[:, 0], d64[:, 1], d64[:, 2] - d64[:, 0] + 1., d64[:, 3] - d64[:, 1] + 1.), 1)
    dseg = np.asarray(det_cls, np.int64).reshape(-1) * n_img + np.asarray(det_img, np.int64).reshape(-1)
    gseg = np.asarray(gt_cls, np.int64).reshape(-1) * n_img + np.asarray(gt_img, np.int64).reshape(-1)
    margin = np.inf
    for s in np.unique(dseg):
        gi = np.nonzero(gseg == s)[0]
        if gi.size == 0:
            continue
        ov = _bb_iou(dbox[dseg == s], gt64[gi], crowd[gi])
        margin = min(margin, float(np.abs(ov[:, :, None] - thr[None, None, :]).min()))
    return margin


def _mean_valid_numpy(x):
    x = np.asarray(x)[np.asarray(x) > -1]
    return float(np.mean(x)) if x.size else -1.


def coco_summarize_numpy(precision, recall):
    """COCOeval.summarize() for the default parameters: the twelve numbers (COCO_SUMMARY_NAMES), each the mean of the
    selected entries that are > -1, -1 when there are none"""
    p, r = np.asarray(precision), np.asarray(recall)
    if p.shape[:2] != (10, 101) or p.shape[3:] != (4, 3):
        raise ValueError("summarize() is defined for COCOeval's default parameters only")
    return np.asarray([_mean_valid_numpy(p[:, :, :, 0, 2]), _mean_valid_numpy(p[0, :, :, 0, 2]),
                       _mean_valid_numpy(p[5, :, :, 0, 2]), _mean_valid_numpy(p[:, :, :, 1, 2]),
                       _mean_valid_numpy(p[:, :, :, 2, 2]), _mean_valid_numpy(p[:, :, :, 3, 2]),
                       _mean_valid_numpy(r[:, :, 0, 0]), _mean_valid_numpy(r[:, :, 0, 1]), _mean_valid_numpy(r[:, :, 0, 2]),
                       _mean_valid_numpy(r[:, :, 1, 2]), _mean_valid_numpy(r[:, :, 2, 2]), _mean_valid_numpy(r[:, :, 3, 2])])


def _mean_valid(x, dims=None):
    """device: the mean of the entries > -1 (over `dims`, default all), -1 where there are none"""
    mask = x > -1
    dims = tuple(range(x.dim())) if dims is None else dims
    cnt = mask.sum(dims)
    tot = torch.where(mask, x, torch.zeros_like(x)).sum(dims)
    return torch.where(cnt > 0, tot / cnt.clamp(min=1).to(torch.float64), torch.full_like(tot, -1.))


class CocoEvalResult:
    """Device tensors of one COCO `compute()`: precision / scores [T,R,K,A,M] and recall [T,K,A,M] float64 (-1 where the
    class has no non-ignored object under the area range), npig [K,A] int32, order [n] and cls_offsets [K+1] int32; with
    codes=True also codes uint8 [A,T,n] and segpos int32 [n], both by rank. The parameters are kept as host arrays."""

    def __init__(self, precision, recall, scores, npig, order, cls_offsets, codes, segpos, params):
        self.precision, self.recall, self.scores, self.npig = precision, recall, scores, npig
        self.order, self.cls_offsets, self.codes, self.segpos = order, cls_offsets, codes, segpos
        self.iou_thrs, self.rec_thrs, self.area_rng, self.max_dets = params

    def summarize(self):
        """-> [12] float64 device tensor, COCOeval.summarize()'s stats in its order (COCO_SUMMARY_NAMES). Defined for the
        default parameters only, as COCOeval's is."""
        if not _coco_is_default(self.iou_thrs, self.rec_thrs, self.area_rng, self.max_dets):
            raise ValueError("summarize() is defined for COCOeval's default parameters only; precision / recall hold "
                             "everything for others")
        p, r = self.precision, self.recall
        return torch.stack([_mean_valid(p[:, :, :, 0, 2]), _mean_valid(p[0, :, :, 0, 2]), _mean_valid(p[5, :, :, 0, 2]),
                            _mean_valid(p[:, :, :, 1, 2]), _mean_valid(p[:, :, :, 2, 2]), _mean_valid(p[:, :, :, 3, 2]),
                            _mean_valid(r[:, :, 0, 0]), _mean_valid(r[:, :, 0, 1]), _mean_valid(r[:, :, 0, 2]),
                            _mean_valid(r[:, :, 1, 2]), _mean_valid(r[:, :, 2, 2]), _mean_valid(r[:, :, 3, 2])])

    def per_class_ap(self):
        """-> [K] float64 device tensor: the per-category AP of `_print_detection_eval_metrics` (coco_split.py:254-285),
        the mean of precision[:, :, k, 0, -1] > -1 (-1 for a class without non-ignored objects)"""
        return _mean_valid(self.precision[:, :, :, 0, -1], (0, 1))


def eval_coco(det, det_img, det_cls, gt_bbox, gt_img, gt_cls, gt_area, gt_flags, n_img, n_cls, iou_thrs, rec_thrs,
              area_rng, max_dets, params=None, codes=False):
    """One `dana_eval_coco` call on device tensors: det [n,5] float32, ids int32, gt_bbox [g,4] float32 (x,y,w,h),
    gt_area float64 [g], gt_flags uint8 [g] (bit 0 iscrowd, bit 1 ignore), iou_thrs [T] / rec_thrs [R] / area_rng [A,2]
    float64 and max_dets [M] int32 -> CocoEvalResult. No synchronisation, no device-to-host copy. `params` are the host
    copies of the four parameter arrays the result keeps for `summarize()`."""
    det = ops._chk(det, "det")
    dev = det.device
    n, g = det.size(0), gt_bbox.size(0)
    T, R, A, M = iou_thrs.numel(), rec_thrs.numel(), area_rng.numel() // 2, max_dets.numel()
    K = int(n_cls)
    ops._chk(det_img, "det_img", torch.int32), ops._chk(det_cls, "det_cls", torch.int32)
    ops._chk(gt_bbox, "gt_bbox"), ops._chk(gt_img, "gt_img", torch.int32), ops._chk(gt_cls, "gt_cls", torch.int32)
    ops._chk(gt_area, "gt_area", torch.float64), ops._chk(gt_flags, "gt_flags", torch.uint8)
    ops._chk(iou_thrs, "iou_thrs", torch.float64), ops._chk(rec_thrs, "rec_thrs", torch.float64)
    ops._chk(area_rng, "area_rng", torch.float64), ops._chk(max_dets, "max_dets", torch.int32)
    if (det_img.numel() != n or det_cls.numel() != n or gt_img.numel() != g or gt_cls.numel() != g or gt_area.numel() != g
            or gt_flags.numel() != g):
        raise ValueError("eval_coco: id / area / flag tensors do not match %d detections / %d objects" % (n, g))
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    cls_offsets = torch.empty((K + 1,), dtype=torch.int32, device=dev)
    segpos = torch.empty((n,), dtype=torch.int32, device=dev)
    cds = torch.empty((A, T, n), dtype=torch.uint8, device=dev)
    npig = torch.empty((K, A), dtype=torch.int32, device=dev)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    ws = ops._ws(lib().query("dana_eval_coco_workspace_bytes", n, g, int(n_img), K, T, R, A, M), dev)
    lib().call("dana_eval_coco", ops._p(det), ops._p(det_img), ops._p(det_cls), n, ops._p(gt_bbox), ops._p(gt_img),
               ops._p(gt_cls), ops._p(gt_area), ops._p(gt_flags), g, int(n_img), K, ops._p(iou_thrs), T, ops._p(rec_thrs), R,
               ops._p(area_rng), A, ops._p(max_dets), M, ops._p(order), ops._p(cls_offsets), ops._p(segpos), ops._p(cds),
               ops._p(npig), ops._p(precision), ops._p(recall), ops._p(scores), ops._p(ws), ws.numel(), ops._stream())
    if params is None:
        params = (None, None, None, None)
    return CocoEvalResult(precision, recall, scores, npig, order, cls_offsets, cds if codes else None,
                          segpos if codes else None, params)


class CocoEvaluator(_DetectionStore):
    """COCO-protocol evaluator living on `device`: COCOeval for iouType = 'bbox' with its default parameters unless given.
    Classes are 0..num_classes-1, images are the caller's indices. Detections come in as for `DetectionEvaluator`
    (`add_packed`, `add_batched`, `add_by_class`: rows (x1,y1,x2,y2,score)); ground truth is COCO's own (x,y,w,h)."""

    def __init__(self, num_classes, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=None, device="cuda"):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("CocoEvaluator: num_classes >= 1")
        self.params = _coco_params(iou_thrs, rec_thrs, area_rng, max_dets)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CocoEvaluator lives on a CUDA (HIP) device: this build has no CPU path")
        self._params_dev = tuple(torch.from_numpy(p).to(self.device) for p in self.params)
        self.reset()

    def reset(self):
        self._reset_detections()
        self._gt = []  # (bbox [k,4] float32, image ids, labels int32, area [k] float64, flags [k] uint8) on the device
        self._gt_cat = None

    def _gt_rows(self, who, bbox, labels, iscrowd, area, ignore):
        bbox = self._dev(bbox, torch.float32).reshape(-1, 4)
        k = bbox.size(0)
        labels = self._dev(labels, torch.int32).reshape(-1)
        flags = torch.zeros((k,), dtype=torch.uint8, device=self.device)
        for bit, x in ((1, iscrowd), (2, ignore)):
            if x is not None:
                x = self._dev(x, torch.int32).reshape(-1)
                if x.numel() != k:
                    raise ValueError("%s: %d objects, %d flags" % (who, k, x.numel()))
                flags = flags | ((x != 0).to(torch.uint8) * bit)
        if area is None:
            b64 = bbox.to(torch.float64)
            area = b64[:, 2] * b64[:, 3]
        else:
            area = self._dev(area, torch.float64).reshape(-1)
        if labels.numel() != k or area.numel() != k:
            raise ValueError("%s: %d objects, %d labels, %d areas" % (who, k, labels.numel(), area.numel()))
        return bbox, labels, area.contiguous(), flags

    def add_ground_truth(self, image_index, bbox_xywh, labels, iscrowd=None, area=None, ignore=None):
        """the objects of one image: bbox [k,4] (x,y,w,h), labels [k] class indices, and per object iscrowd (default 0),
        area (default w*h; COCO's annotation area is the segmentation's) and ignore (default 0)"""
        bbox, labels, area, flags = self._gt_rows("add_ground_truth", bbox_xywh, labels, iscrowd, area, ignore)
        image_index = int(image_index)
        if image_index < 0:
            raise ValueError("add_ground_truth: negative image index")
        self.num_images = max(self.num_images, image_index + 1)
        img = torch.full((bbox.size(0),), image_index, dtype=torch.int32, device=self.device)
        self._gt.append((bbox, img, labels, area, flags))
        self._gt_cat = None

    def add_ground_truth_packed(self, bbox_xywh, img_ids, labels, iscrowd=None, area=None, ignore=None, num_images=None):
        """the objects of many images at once, with per-row image ids (ids on the device need `num_images`)"""
        bbox, labels, area, flags = self._gt_rows("add_ground_truth_packed", bbox_xywh, labels, iscrowd, area, ignore)
        host_img = _host_ints(img_ids)
        if num_images is not None:
            self.num_images = max(self.num_images, int(num_images))
        elif host_img is None:
            raise ValueError("add_ground_truth_packed: img_ids live on the device; pass num_images")
        elif host_img.size:
            self.num_images = max(self.num_images, int(host_img.max()) + 1)
        img = self._dev(img_ids, torch.int32).reshape(-1)
        if img.numel() != bbox.size(0):
            raise ValueError("add_ground_truth_packed: %d objects, %d image ids" % (bbox.size(0), img.numel()))
        self._gt.append((bbox, img, labels, area, flags))
        self._gt_cat = None

    def _ground_truth(self):
        if self._gt_cat is None:
            if self._gt:
                self._gt_cat = tuple(torch.cat([g[i] for g in self._gt], 0).contiguous() for i in range(5))
            else:
                e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
                self._gt_cat = (e((0, 4), torch.float32), e((0,), torch.int32), e((0,), torch.int32),
                                e((0,), torch.float64), e((0,), torch.uint8))
        return self._gt_cat

    def compute(self, codes=False):
        """-> CocoEvalResult (device tensors; nothing is synchronised or read back here)"""
        gbox, gimg, gcls, garea, gflags = self._ground_truth()
        det, img, cls = self._detections()
        return eval_coco(det, img, cls, gbox, gimg, gcls, garea, gflags, max(self.num_images, 1), self.num_classes,
                         *self._params_dev, params=self.params, codes=codes)


def _annotation_arrays(objs):
    """one image's objects -> (bbox, labels, iscrowd, area, ignore): a dict of arrays (bbox, labels and optionally
    iscrowd / area / ignore), a tuple in that order, or a list of per-object dicts with bbox, category (the class index)
    and optionally iscrowd / area / ignore"""
    if isinstance(objs, dict):
        return tuple(objs.get(k) for k in ("bbox", "labels", "iscrowd", "area", "ignore"))
    if isinstance(objs, tuple):
        return tuple(objs) + (None,) * (5 - len(objs))
    bbox = np.asarray([o["bbox"] for o in objs], np.float32).reshape(-1, 4)
    labels = np.asarray([o["category"] for o in objs], np.int32)
    crowd = np.asarray([o.get("iscrowd", 0) for o in objs], np.int32)
    ignore = np.asarray([o.get("ignore", 0) for o in objs], np.int32)
    area = np.asarray([o["area"] if "area" in o else float(np.float32(o["bbox"][2])) * float(np.float32(o["bbox"][3]))
                       for o in objs], np.float64)
    return bbox, labels, crowd, area, ignore


def evaluate_coco_boxes(all_boxes, annotations, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=None, device="cuda",
                        codes=False):
    """Drop-in for what coco_split.py:338-349 (`_write_coco_results_file` + `_do_detection_eval`) does with
    `all_boxes`: all_boxes[j][i] is the [k,5] array (x1,y1,x2,y2,score) of class j on image i, as inference.py fills it
    (an empty list where nothing was detected); annotations[i] are image i's objects (see `_annotation_arrays`), their
    class indices indexing all_boxes' j. A background class 0 the caller leaves empty has no objects and comes out -1,
    outside every mean. -> CocoEvalResult: `.summarize()` are the twelve numbers COCOeval prints, `.per_class_ap()` the
    per-category table."""
    C = len(all_boxes)
    n_img = len(annotations)
    ev = CocoEvaluator(C, iou_thrs, rec_thrs, area_rng, max_dets, device)
    rows, imgs, clss = [], [], []
    for j in range(C):
        for i in range(len(all_boxes[j])):
            d = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            if d.shape[0]:
                rows.append(d)
                imgs.append(np.full(d.shape[0], i, np.int32))
                clss.append(np.full(d.shape[0], j, np.int32))
            n_img = max(n_img, i + 1)
    for i, objs in enumerate(annotations):
        bbox, labels, crowd, area, ignore = _annotation_arrays(objs)
        if len(labels):
            ev.add_ground_truth(i, bbox, labels, crowd, area, ignore)
    if rows:
        ev.add_packed(np.concatenate(rows, 0), np.concatenate(imgs), np.concatenate(clss), num_images=n_img)
    ev.num_images = max(ev.num_images, n_img)
    return ev.compute(codes=codes)


# ==== proposal recall ========================================================================================================

RECALL_AREA_NAMES = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")  # imdb.py:150-160
RECALL_AREA_RNG = np.asarray([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2],
                              [96 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]], np.float64)
RECALL_LIMITS = (10, 100, 300, 1000)
RECALL_MAX_CANDIDATES = 65536  # rows of one proposal list (the matching kernel's bitmap of used candidates)


def _recall_area(area):
    """None -> the eight named ranges; a 1-d list of names / numbers -> those rows of RECALL_AREA_RNG; a 2-d array ->
    [A,2] ranges as given. -> (names or None, float64 [A,2])"""
    if area is None:
        return RECALL_AREA_NAMES, RECALL_AREA_RNG.copy()
    if isinstance(area, (str, int, np.integer)):
        area = [area]
    if not isinstance(area, np.ndarray) and len(area) and all(isinstance(x, (str, int, np.integer)) for x in area):
        rows = []
        for x in area:
            if isinstance(x, str):
                if x not in RECALL_AREA_NAMES:
                    raise ValueError("unknown area range %r: one of %s" % (x, ", ".join(RECALL_AREA_NAMES)))
                rows.append(RECALL_AREA_NAMES.index(x))
            else:
                if not 0 <= int(x) < len(RECALL_AREA_NAMES):
                    raise ValueError("unknown area range %d: 0..%d" % (int(x), len(RECALL_AREA_NAMES) - 1))
                rows.append(int(x))
        return tuple(RECALL_AREA_NAMES[r] for r in rows), RECALL_AREA_RNG[rows].copy()
    rng = np.ascontiguousarray(np.asarray(area, np.float64))
    if rng.ndim != 2 or rng.shape[1] != 2:
        raise ValueError("area ranges: names, numbers or an [A,2] array of (low, high)")
    return None, rng


def _recall_params(iou_thrs, limits, area):
    """-> (iou_thrs float64 [T], limits int32 [L], area_rng float64 [A,2], area names or None), checked against what the
    kernels take"""
    thr = np.ascontiguousarray(np.asarray(COCO_THRESHOLDS if iou_thrs is None else iou_thrs, np.float64).reshape(-1))
    lim = np.asarray(limits).reshape(-1)
    names, rng = _recall_area(area)
    if not (1 <= thr.size <= 16 and 1 <= lim.size <= 8 and 1 <= rng.shape[0] <= 8):
        raise ValueError("proposal recall: 1..16 IoU thresholds, 1..8 limits, 1..8 area ranges (got %d, %d, %d)"
                         % (thr.size, lim.size, rng.shape[0]))
    if (np.abs(lim.astype(np.float64)) >= 2 ** 31).any() or (lim != np.round(lim)).any():
        raise ValueError("proposal recall: limits are integers (<= 0: the whole list)")
    return thr, np.ascontiguousarray(lim.astype(np.int32)), rng, names


def _recall_tables(prob_img, prob_cls, counts, offsets, gt_img, gt_cls, n_cls, others=False):
    """The host bookkeeping of proposal recall. Problems (image, class, count, first row) and ground-truth ids ->
    dict(unit_tab int32 [U,9] = (box_off, box_count, gt0_begin, gt0_end, gt1_begin, gt1_end, pair_off, cls, role),
    gt_order int32 [g] (the stable (image, class) order), n_pairs, pair_unit / pair_gt int64 [n_pairs]: the unit and the
    ground-truth row of every pair). Units: the target unit of every problem in arrival order, then (others=True) the
    other unit of every problem."""
    K = int(n_cls)
    p_img = np.asarray(prob_img, np.int64).reshape(-1)
    p_cls = np.asarray(prob_cls, np.int64).reshape(-1)
    cnt = np.asarray(counts, np.int64).reshape(-1)
    P = cnt.size
    off = np.asarray(offsets, np.int64).reshape(-1)[:P]
    g_img = np.asarray(gt_img, np.int64).reshape(-1)
    g_cls = np.asarray(gt_cls, np.int64).reshape(-1)
    if K < 1 or p_img.size != P or p_cls.size != P or off.size != P or g_img.size != g_cls.size:
        raise ValueError("proposal recall: %d problems need as many image ids, class ids and offsets; ground truth needs "
                         "one image id and one class id per box" % P)
    if P and ((p_img < 0).any() or (p_cls < 0).any() or (p_cls >= K).any() or (cnt < 0).any() or (off < 0).any()):
        raise ValueError("proposal recall: problem ids outside [0, inf) x [0, %d), or a negative count / offset" % K)
    if P and int(cnt.max()) > RECALL_MAX_CANDIDATES:
        raise ValueError("proposal recall: a list of %d rows; at most %d candidates per list" % (int(cnt.max()),
                                                                                                  RECALL_MAX_CANDIDATES))
    if g_img.size and ((g_img < 0).any() or (g_cls < 0).any() or (g_cls >= K).any()):
        raise ValueError("proposal recall: ground-truth ids outside [0, inf) x [0, %d)" % K)
    gt_order = np.lexsort((g_cls, g_img))  # stable: by image, then class, then arrival
    key = g_img[gt_order] * K + g_cls[gt_order]
    b0 = np.searchsorted(key, p_img * K + p_cls, side="left")
    e0 = np.searchsorted(key, p_img * K + p_cls, side="right")
    ib = np.searchsorted(key, p_img * K, side="left")
    ie = np.searchsorted(key, (p_img + 1) * K, side="left")
    zero = np.zeros(P, np.int64)
    tab = np.stack((off, cnt, b0, e0, zero, zero, zero, p_cls, zero), 1)
    if others:
        tab = np.concatenate((tab, np.stack((off, cnt, ib, b0, e0, ie, zero, p_cls, zero + 1), 1)), 0)
    n_obj = (tab[:, 3] - tab[:, 2]) + (tab[:, 5] - tab[:, 4])
    tab[:, 6] = np.cumsum(n_obj) - n_obj
    n_pairs = int(n_obj.sum())
    if n_pairs >= 2 ** 31 - 1 or tab.shape[0] >= 2 ** 31 - 1 or (P and int((off + cnt).max()) >= 2 ** 31 - 1):
        raise ValueError("proposal recall: %d pairs / %d units overflow the int32 tables" % (n_pairs, tab.shape[0]))
    pair_unit = np.repeat(np.arange(tab.shape[0], dtype=np.int64), n_obj)
    within = np.arange(n_pairs, dtype=np.int64) - tab[pair_unit, 6]
    n0 = (tab[:, 3] - tab[:, 2])[pair_unit]
    pos = np.where(within < n0, tab[pair_unit, 2] + within, tab[pair_unit, 4] + within - n0)
    return dict(unit_tab=np.ascontiguousarray(tab.astype(np.int32)), gt_order=gt_order.astype(np.int32), n_pairs=n_pairs,
                pair_unit=pair_unit, pair_gt=gt_order[pos].astype(np.int64))


def _recall_ratios(hits, npos):
    """counts -> (recalls [2,T,L,A], ar [2,L,A]) in numpy float64: the classes are summed before the one division
    (imdb.py:221), ar is the mean over the thresholds (:223); NaN where there are no objects"""
    with np.errstate(divide="ignore", invalid="ignore"):
        recalls = hits.sum(-1).astype(np.float64) / npos.sum(-1).astype(np.float64)[:, None, None, :]
    return recalls, recalls.mean(1)


def proposal_recall_numpy(boxes, prob_img, prob_cls, counts, offsets, gt_box, gt_img, gt_cls, n_cls, iou_thrs=None,
                          limits=(0,), area_rng=None, gt_area=None, others=False):
    """Proposal recall in numpy float64 (host), the tests' yardstick: imdb.py:137-225 per (unit, limit, area range), as
    the matrix procedure -- the IoU matrix of candidates x objects; the column maxima; the best-covered object and the
    candidate that covers it best (two argmax calls: the lowest object, then the lowest row among equals); record; take
    the row and the column out. Taken entries are set to -inf, so that they lose against every IoU. boxes [n,4] with
    problem p at rows offsets[p] : offsets[p] + counts[p]; area_rng as `_recall_area` takes it (None: the eight named
    ranges). -> dict(unit_tab, gt_order, n_pairs, pair_unit, pair_gt, ov float64 [L,A,n_pairs], match int64
    [L,A,n_pairs], hits int64 [2,T,L,A,K], npos int64 [2,A,K], recalls [2,T,L,A], ar [2,L,A])."""
    thr, lim, rng, _ = _recall_params(iou_thrs, limits, area_rng)
    K = int(n_cls)
    T, L, A = thr.size, lim.size, rng.shape[0]
    out = _recall_tables(prob_img, prob_cls, counts, offsets, gt_img, gt_cls, K, others)
    tab, n_pairs, pair_gt = out["unit_tab"].astype(np.int64), out["n_pairs"], out["pair_gt"]
    b64 = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64)
    g64 = np.asarray(gt_box, np.float32).reshape(-1, 4).astype(np.float64)
    if gt_area is None:
        area = (g64[:, 2] - g64[:, 0] + 1.) * (g64[:, 3] - g64[:, 1] + 1.)
    else:
        area = np.asarray(gt_area, np.float64).reshape(-1)
    if area.size != g64.shape[0] or g64.shape[0] != np.asarray(gt_img).size:
        raise ValueError("proposal recall: %d ground-truth boxes need as many ids and areas" % g64.shape[0])
    ov = np.full((L, A, n_pairs), -1.)
    match = np.full((L, A, n_pairs), -1, np.int64)
    for u in range(tab.shape[0]):
        off, cnt, p0 = tab[u, 0], tab[u, 1], tab[u, 6]
        rows = pair_gt[p0:p0 + (tab[u, 3] - tab[u, 2]) + (tab[u, 5] - tab[u, 4])]
        if rows.size == 0:
            continue
        for li in range(L):
            m = int(cnt if lim[li] <= 0 else min(lim[li], cnt))
            full = _iou_matrix(b64[off:off + m], g64[rows]) if m else np.zeros((0, rows.size))
            for a in range(A):
                inside = np.nonzero((rng[a, 0] <= area[rows]) & (area[rows] <= rng[a, 1]))[0]
                mat = full[:, inside].copy()
                o = np.zeros(inside.size)
                r = np.full(inside.size, -1, np.int64)
                for _ in range(min(m, inside.size)):
                    col_arg = mat.argmax(axis=0)
                    col_max = mat.max(axis=0)
                    j = int(col_max.argmax())
                    i = int(col_arg[j])
                    o[j], r[j] = mat[i, j], i
                    mat[i, :] = -np.inf
                    mat[:, j] = -np.inf
                ov[li, a, p0 + inside] = o
                match[li, a, p0 + inside] = r
    role, k = tab[out["pair_unit"], 8], tab[out["pair_unit"], 7]
    hits = np.zeros((2, T, L, A, K), np.int64)
    npos = np.zeros((2, A, K), np.int64)
    for a in range(A):
        part = ov[0, a] != -1.
        np.add.at(npos[:, a, :], (role[part], k[part]), 1)
        for li in range(L):
            for t in range(T):
                hit = part & (ov[li, a] >= thr[t])
                np.add.at(hits[:, t, li, a, :], (role[hit], k[hit]), 1)
    recalls, ar = _recall_ratios(hits, npos)
    out.update(ov=ov, match=match, hits=hits, npos=npos, recalls=recalls, ar=ar)
    return out


def eval_proposal_recall(boxes, unit_tab, gt_box, gt_area, gt_order, n_pairs, n_cls, iou_thr, limits, area_rng):
    """One `dana_eval_proposal_recall` call on device tensors: boxes [n,4] float32, unit_tab int32 [U,9], gt_box [g,4]
    float32, gt_area float64 [g] or None, gt_order int32 [g], iou_thr float64 [T], limits int32 [L], area_rng float64
    [A,2]; n_pairs is the host's count. -> (ov float64 [L,A,n_pairs], match int32 [L,A,n_pairs], hits int64
    [2,T,L,A,K], npos int64 [2,A,K]). No synchronisation, no device-to-host copy."""
    boxes = ops._chk(boxes, "boxes")
    dev = boxes.device
    ops._chk(unit_tab, "unit_tab", torch.int32), ops._chk(gt_box, "gt_box"), ops._chk(gt_order, "gt_order", torch.int32)
    ops._chk(iou_thr, "iou_thr", torch.float64), ops._chk(limits, "limits", torch.int32)
    ops._chk(area_rng, "area_rng", torch.float64)
    if gt_area is not None:
        ops._chk(gt_area, "gt_area", torch.float64)
    U, g = unit_tab.numel() // 9, gt_box.numel() // 4
    T, L, A, K = iou_thr.numel(), limits.numel(), area_rng.numel() // 2, int(n_cls)
    n_pairs = int(n_pairs)
    if unit_tab.numel() != 9 * U or gt_order.numel() != g or (gt_area is not None and gt_area.numel() != g):
        raise ValueError("eval_proposal_recall: unit_tab is [U,9]; gt_order and gt_area match the %d ground-truth boxes" % g)
    ov = torch.empty((L, A, n_pairs), dtype=torch.float64, device=dev)
    match = torch.empty((L, A, n_pairs), dtype=torch.int32, device=dev)
    hits = torch.empty((2, T, L, A, K), dtype=torch.int64, device=dev)
    npos = torch.empty((2, A, K), dtype=torch.int64, device=dev)
    ws = ops._ws(lib().query("dana_eval_proposal_recall_workspace_bytes", boxes.size(0), U, n_pairs, T, L, A), dev)
    lib().call("dana_eval_proposal_recall", ops._p(boxes), ops._p(unit_tab), U, ops._p(gt_box), ops._p(gt_area),
               ops._p(gt_order), g, n_pairs, K, ops._p(iou_thr), T, ops._p(limits), L, ops._p(area_rng), A, ops._p(ov),
               ops._p(match), ops._p(hits), ops._p(npos), ops._p(ws), ws.numel(), ops._stream())
    return ov, match, hits, npos


class ProposalRecallResult:
    """Device tensors of one proposal-recall `compute()`. Role 0 is the target units (the objects of the class the list
    was proposed for), role 1 the other units (the image's other objects under the same list).
      hits int64 [2,T,L,A,K], npos int64 [2,A,K]: the raw counts (K: the class the proposals were made for);
      recalls [2,T,L,A]: the classes summed before the division; ar [2,L,A]: its mean over the thresholds (imdb.py:223);
      per_class_recalls [2,T,L,A,K], per_class_ar [2,L,A,K]; all float64, NaN where npos == 0.
    From `compute()` also ov float64 / match int32 [L,A,n_pairs] and the host pair tables: pair_gt[n_pairs] is the
    ground-truth row (in the order it was added) and pair_unit[n_pairs] the row of unit_tab of every pair.
    `params` = (iou_thrs, limits, area_rng, area names or None) as host arrays."""

    def __init__(self, hits, npos, params, ov=None, match=None, tables=None):
        self.hits, self.npos, self.params = hits, npos, params
        self.iou_thrs, self.limits, self.area_rng, self.area_names = params
        self.ov, self.match = ov, match
        tables = tables or {}
        self.unit_tab, self.pair_unit, self.pair_gt = (tables.get(k) for k in ("unit_tab", "pair_unit", "pair_gt"))
        h, n = hits.to(torch.float64), npos.to(torch.float64)
        self.recalls = h.sum(-1) / n.sum(-1)[:, None, None, :]
        self.ar = self.recalls.mean(1)
        self.per_class_recalls = h / n[:, None, None, :, :]
        self.per_class_ar = self.per_class_recalls.mean(1)

    @classmethod
    def from_counts(cls, hits, npos, params):
        """the result of pooled counts: a caller that all-reduces (sums) `hits` and `npos` across ranks gets the pooled
        recalls from here. `params` as `ProposalRecallEvaluator.params` / a result's `.params`."""
        T, L, A = len(params[0]), len(params[1]), len(params[2])
        if hits.dim() != 5 or npos.dim() != 3 or tuple(hits.shape[:4]) != (2, T, L, A) or \
                tuple(npos.shape) != (2, A, hits.size(4)):
            raise ValueError("from_counts: hits [2,%d,%d,%d,K] and npos [2,%d,K] expected, got %s and %s"
                             % (T, L, A, A, tuple(hits.shape), tuple(npos.shape)))
        return cls(hits, npos, params)

    def _index(self, limit, area):
        lim = [int(x) for x in self.limits]
        if int(limit) not in lim:
            raise ValueError("limit %r is not one of %s" % (limit, lim))
        if isinstance(area, str):
            if self.area_names is None or area not in self.area_names:
                raise ValueError("area range %r is not one of %s" % (area, self.area_names))
            area = self.area_names.index(area)
        if not 0 <= int(area) < len(self.area_rng):
            raise ValueError("area range %r outside 0..%d" % (area, len(self.area_rng) - 1))
        return lim.index(int(limit)), int(area)

    def gt_overlaps(self, limit, area=0):
        """-> [n_pairs] float64 view: the matched IoU of every pair under this limit (its value) and area range (its name
        or its index): -1 outside the range, 0 when the candidates ran out. `pair_gt` / `pair_unit` name the pairs."""
        if self.ov is None:
            raise ValueError("gt_overlaps needs a result of compute(), not of from_counts()")
        li, a = self._index(limit, area)
        return self.ov[li, a]

    def matched_rows(self, limit, area=0):
        """-> [n_pairs] int32 view: the row, within its list, of the proposal matched to every pair (-1: none)"""
        if self.match is None:
            raise ValueError("matched_rows needs a result of compute(), not of from_counts()")
        li, a = self._index(limit, area)
        return self.match[li, a]

    def selectivity(self):
        """-> [L,A] float64: ar[0] / ar[1], the recall the list gives its own class over the recall it gives the image's
        other objects. NaN without `others` (no other unit has an object)."""
        return self.ar[0] / self.ar[1]


def _box_rows(x):
    """rows of an [*,4] array or tensor, read from its shape"""
    n = int(np.prod(np.shape(x)))
    if n % 4:
        raise ValueError("boxes are [*,4] rows (x1, y1, x2, y2); got shape %s" % (tuple(np.shape(x)),))
    return n // 4


class ProposalRecallEvaluator:
    """Proposal recall living on `device`: py-faster-rcnn's `evaluate_recall` (imdb.py:137-225) per proposal list, fed
    from the `rois` an eval-mode forward returns. A list is made for one image under one class (a class sweep makes C per
    image); it is measured on the image's objects of that class (the target unit) and, with others=True, also on the
    image's other objects (the other unit): ar[0] beside ar[1] is the RPN's selectivity. A list added twice (shot views of
    one class) is two trials; ground truth of a class for which no list of its image was added does not count. Classes
    are 0..num_classes-1, images the caller's indices; all ids are host integers, boxes may live on the device, no method
    reads from the device."""

    def __init__(self, num_classes, device="cuda", iou_thresholds=COCO_THRESHOLDS, limits=RECALL_LIMITS, area_ranges=None,
                 others=False):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("ProposalRecallEvaluator: num_classes >= 1")
        self.params = _recall_params(iou_thresholds, limits, area_ranges)
        self.others = bool(others)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ProposalRecallEvaluator lives on a CUDA (HIP) device: this build has no CPU path")
        self._params_dev = None  # uploaded by the first compute()
        self.reset()

    def reset(self):
        self.num_rows = 0
        self._cap = 0
        self._box = None
        self._prob = []  # (image ids, class ids, counts, first rows) per add, host int64
        self._gt = []    # (boxes [k,4] float32 on the device, area [k] float64 on the device or None, image ids, labels)

    _dev = _DetectionStore._dev

    def _reserve(self, rows):
        need = self.num_rows + rows
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 1024)
        box = torch.empty((cap, 4), dtype=torch.float32, device=self.device)
        if self.num_rows:
            box[:self.num_rows].copy_(self._box[:self.num_rows])
        self._box, self._cap = box, cap

    # -- ground truth
    def _add_gt(self, who, boxes, img, labels, area):
        k = _box_rows(boxes)  # (every check comes before the first byte moves to the device)
        if img is None or labels is None:
            raise ValueError("%s: image indices and labels are host integers (nothing is read back)" % who)
        if img.size != k or labels.size != k:
            raise ValueError("%s: %d boxes, %d image ids, %d labels" % (who, k, img.size, labels.size))
        if k and ((img < 0).any() or (labels < 0).any() or (labels >= self.num_classes).any()):
            raise ValueError("%s: ids outside [0, inf) x [0, %d)" % (who, self.num_classes))
        if area is not None:
            if int(np.prod(np.shape(area))) != k:
                raise ValueError("%s: %d boxes, %d areas" % (who, k, int(np.prod(np.shape(area)))))
            area = self._dev(area, torch.float64).reshape(-1)
        boxes = self._dev(boxes, torch.float32).reshape(-1, 4)
        self._gt.append((boxes, area, img.astype(np.int64), labels.astype(np.int64)))

    def add_ground_truth(self, image_index, boxes, labels, area=None):
        """the objects of one image: boxes [k,4] (x1,y1,x2,y2) in original-image pixels, labels [k] host class indices,
        area [k] (default (x2 - x1 + 1) * (y2 - y1 + 1); a dataset's `seg_areas` go here)"""
        labels = _host_ints(labels)
        img = None if labels is None else np.full(labels.size, int(image_index), np.int32)
        self._add_gt("add_ground_truth", boxes, img, labels, area)

    def add_ground_truth_packed(self, boxes, img_ids, labels, area=None):
        """the objects of many images at once, with per-row host image ids"""
        self._add_gt("add_ground_truth_packed", boxes, _host_ints(img_ids), _host_ints(labels), area)

    # -- proposals
    def add_proposals(self, boxes_packed, counts, offsets, image_indices, class_indices):
        """The primitive: P proposal lists, list p the rows offsets[p] : offsets[p] + counts[p] of boxes_packed [*,4]
        (x1,y1,x2,y2 in original-image pixels, best first), made for image image_indices[p] under class class_indices[p]
        (host integers; an int applies to all). offsets=None: the lists follow each other. The rows are appended to the
        evaluator's device buffer; nothing is read back."""
        counts = _host_ints(counts)
        if counts is None:
            raise ValueError("add_proposals: counts are host integers")
        P = counts.size
        if offsets is None:
            offsets = np.concatenate(([0], np.cumsum(counts[:-1], dtype=np.int64))) if P else counts
        offsets = _host_ints(offsets)
        img, cls = _host_ints(image_indices), _host_ints(class_indices)
        if offsets is None or img is None or cls is None:
            raise ValueError("add_proposals: offsets, image and class indices are host integers (nothing is read back)")
        img = np.repeat(img, P) if img.size == 1 and P != 1 else img
        cls = np.repeat(cls, P) if cls.size == 1 and P != 1 else cls
        offsets = offsets[:P].astype(np.int64)
        if offsets.size != P or img.size != P or cls.size != P or (counts < 0).any() or (offsets < 0).any():
            raise ValueError("add_proposals: %d lists need as many counts, offsets, image and class indices" % P)
        if P and ((img < 0).any() or (cls < 0).any() or (cls >= self.num_classes).any()):
            raise ValueError("add_proposals: ids outside [0, inf) x [0, %d)" % self.num_classes)
        if P and int(counts.max()) > RECALL_MAX_CANDIDATES:
            raise ValueError("add_proposals: a list of %d rows; at most %d candidates per list"
                             % (int(counts.max()), RECALL_MAX_CANDIDATES))
        cnt = counts.astype(np.int64)
        if P and int((offsets + cnt).max()) > _box_rows(boxes_packed):
            raise ValueError("add_proposals: offsets + counts run past the %d packed rows" % _box_rows(boxes_packed))
        src = self._dev(boxes_packed, torch.float32).reshape(-1, 4)
        rows = int(cnt.sum())
        dst = self.num_rows + np.cumsum(cnt) - cnt
        self._prob.append((img.astype(np.int64), cls.astype(np.int64), cnt, dst))
        if rows == 0:
            return
        self._reserve(rows)
        a = self.num_rows
        live = cnt > 0
        first = offsets[live]
        if (first[1:] == first[:-1] + cnt[live][:-1]).all():  # one run of rows
            self._box[a:a + rows].copy_(src[int(first[0]):int(first[0]) + rows])
        else:
            within = np.arange(rows, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            idx = ops._h2d_int32((np.repeat(offsets, cnt) + within).astype(np.int32), self.device)
            self._box[a:a + rows].copy_(src.index_select(0, idx))
        self.num_rows += rows

    def add_rois(self, rois, im_info, image_indices, class_indices, counts=None):
        """The `rois` [P,R,5] of an eval-mode forward (column 0 the problem, columns 1..4 the box in network-input pixels)
        with the forward's im_info [B,3]: the boxes are divided by the image's scale im_info[.., 2] -- one fp32 division,
        as inference.py:125 does for the detections. P == B: image_indices [B], class_indices [B] or an int. A class sweep
        (P == B * C, problem p = b * C + c uses im_info[b]): `add_rois(rois, im_info, image_indices, sweep.classes)` with
        the B image indices and the C classes. counts=None: all R rows count -- the proposal layer pads a short list with
        zero rows, which then stand as one-pixel boxes at the origin (they are last in the list and overlap next to
        nothing, but they do fill a budget); a caller that knows the real lengths passes them as `counts` [P]."""
        if not isinstance(rois, torch.Tensor) or rois.dim() != 3 or rois.size(2) != 5:
            raise ValueError("add_rois: rois are the [P,R,5] tensor of an eval-mode forward")
        P, R = int(rois.size(0)), int(rois.size(1))
        img, cls = _host_ints(image_indices), _host_ints(class_indices)
        if img is None or cls is None:
            raise ValueError("add_rois: image and class indices are host integers (nothing is read back)")
        if not isinstance(im_info, torch.Tensor):
            im_info = torch.from_numpy(np.ascontiguousarray(np.asarray(im_info, np.float32)))
        im_info = im_info.reshape(-1, 3)
        B = int(im_info.size(0))
        if B < 1 or P % B:
            raise ValueError("add_rois: %d problems over %d rows of im_info" % (P, B))
        C = P // B
        if img.size == P and cls.size == P:
            p_img, p_cls = img, cls
        elif img.size == B and cls.size == C:
            p_img, p_cls = np.repeat(img, C), np.tile(cls, B)
        elif img.size == B and cls.size == 1:
            p_img, p_cls = np.repeat(img, C), np.repeat(cls, P)
        else:
            raise ValueError("add_rois: %d problems = %d images x %d classes; got %d image and %d class indices"
                             % (P, B, C, img.size, cls.size))
        scale = im_info[:, 2].to(device=self.device, dtype=torch.float32).repeat_interleave(C)
        boxes = (rois.to(self.device)[:, :, 1:5] / scale.view(P, 1, 1)).reshape(-1, 4)
        if counts is None:
            cnt = np.full(P, R, np.int32)
        else:
            cnt = _host_ints(counts)
            if cnt is None or cnt.size != P or (cnt < 0).any() or (cnt > R).any():
                raise ValueError("add_rois: counts are %d host integers in 0..%d" % (P, R))
        self.add_proposals(boxes, cnt, np.arange(P, dtype=np.int64) * R, p_img, p_cls)

    def proposals(self):
        """-> (boxes [n,4] device view of the rows added so far, image ids, class ids, counts, first rows: host int64 [P])"""
        box = self._box[:self.num_rows] if self.num_rows else torch.empty((0, 4), dtype=torch.float32, device=self.device)
        return (box,) + self._problems()

    # -- the host tables and the call
    def _problems(self):
        if not self._prob:
            e = np.zeros(0, np.int64)
            return e, e, e, e
        return tuple(np.concatenate([p[i] for p in self._prob]) for i in range(4))

    def _ground_truth(self):
        """-> (boxes [g,4] device, area [g] float64 device or None, image ids, labels): area is None when no add gave one"""
        if not self._gt:
            e = np.zeros(0, np.int64)
            return torch.empty((0, 4), dtype=torch.float32, device=self.device), None, e, e
        box = torch.cat([g[0] for g in self._gt], 0).contiguous()
        area = None
        if any(g[1] is not None for g in self._gt):
            parts = []
            for b, ar, _, _ in self._gt:
                if ar is None:
                    b64 = b.to(torch.float64)
                    ar = (b64[:, 2] - b64[:, 0] + 1.) * (b64[:, 3] - b64[:, 1] + 1.)
                parts.append(ar)
            area = torch.cat(parts, 0).contiguous()
        return box, area, np.concatenate([g[2] for g in self._gt]), np.concatenate([g[3] for g in self._gt])

    def tables(self):
        """the host bookkeeping `compute()` uploads (see `_recall_tables`)"""
        p_img, p_cls, cnt, off = self._problems()
        _, _, g_img, g_cls = self._ground_truth()
        return _recall_tables(p_img, p_cls, cnt, off, g_img, g_cls, self.num_classes, self.others)

    def compute(self):
        """-> ProposalRecallResult (device tensors; one upload of the unit table and the ground-truth order, one C call,
        nothing synchronised or read back)"""
        gbox, garea, g_img, g_cls = self._ground_truth()
        p_img, p_cls, cnt, off = self._problems()
        tb = _recall_tables(p_img, p_cls, cnt, off, g_img, g_cls, self.num_classes, self.others)
        U, g = tb["unit_tab"].shape[0], tb["gt_order"].size
        small = ops._h2d_int32(np.concatenate((tb["unit_tab"].reshape(-1), tb["gt_order"], np.zeros(1, np.int32))),
                               self.device)
        boxes = self.proposals()[0]
        if self._params_dev is None:
            self._params_dev = tuple(torch.from_numpy(p).to(self.device) for p in self.params[:3])
        thr, lim, rng = self._params_dev
        ov, match, hits, npos = eval_proposal_recall(boxes, small[:9 * U].view(U, 9), gbox, garea, small[9 * U:9 * U + g],
                                                     tb["n_pairs"], self.num_classes, thr, lim, rng)
        return ProposalRecallResult(hits, npos, self.params, ov, match, tb)
