"""Detection evaluation on the device: what `imdb.evaluate_detections(all_boxes, output_dir)` (inference.py:181) ends
in -- lib/datasets/voc_eval.py -- without the text files, the parse and the per-detection Python loop.

`DetectionEvaluator` accumulates detections across forwards in device buffers (no method reads from the device: the
row counts come from the host layout that post-processing has already read) and `compute()` gives per-class AP at every
IoU threshold in one C call (csrc/evaluate.hip: two radix sorts, one wavefront per (class, image) for the TP/FP
marking, one workgroup per (class, threshold) for the curves). All arithmetic is float64.

This is the VOC protocol: the TP/FP marking of voc_eval.py:165-199, the curves of :202-207, both `voc_ap` metrics of
:35-66. Thresholds 0.50:0.05:0.95 are ten `voc_eval` calls in one pass. It is NOT COCOeval: crowd regions, area ranges
and maxDets are not modelled.

Defined where the reference is not, or differs:
  * equal scores within a class are ranked in arrival order (the reference's `np.argsort(-confidence)` is not stable);
  * a class without non-difficult ground truth (npos == 0) has AP = NaN under BOTH metrics (the reference: 0 under the
    11-point metric, NaN under the area metric) and `mean_ap()` averages the classes with npos > 0;
  * boxes are taken as given: pascal_voc.py:288-291 adds 1 to the detection coordinates before voc_eval sees them, so a
    caller that wants the reference's numbers adds it (`evaluate_all_boxes(..., add_one=True)` does).

`voc_numpy` is the same semantics restated in plain numpy float64 (host): the tests' yardstick, pinned to the reference
by tests/golden/eval_voc.npz.
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


class DetectionEvaluator:
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
        self.num_rows = 0
        self.num_images = 0
        self._cap = 0
        self._det = self._img = self._cls = None
        self._gt = []  # (boxes [k,4] float32, image ids [k] int32, labels [k] int32, difficult [k] uint8) on the device
        self._gt_cat = None

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
