"""Error diagnosis on the device: why the AP is not higher. TIDE (Bolya et al., "TIDE: A General Toolbox for Identifying
Object Detection Errors", ECCV 2020) on the lists `DetectionEvaluator` accumulates: every false positive and every
undetected object gets one of six error types, and every type gets the AP that repairing it alone would give.

`DetectionDiagnoser` is a `DetectionEvaluator` with one foreground and one background threshold; `compute()` is one C
call (csrc/diagnose.hip) and reads nothing back; `DiagnosisResult.summary()` is the one method that does. For a class
sweep (`cache.sweep(classes)`) the telling numbers are `Cls` against `Loc` / `Miss`: an object claimed by several
classes' supports is a classification error (the attention, the class head), a proposal that never covered the object a
miss or a localisation error (the RPN).

Restated from the paper: the reference tree has nothing of the kind and tidecv is not installed, so nothing here was
generated from it. The rules, with every choice the paper leaves open:

  * Step 1 is `voc_numpy` / `dana_eval_ap` at the single threshold t_f: the same rank (class, score descending, arrival),
    codes 1 = TP, 2 = FP, 0 = matched a difficult box, the same npos and AP, bit for bit.
  * Step 2 looks at the counted objects of the detection's image only: ids in range and NOT difficult (a difficult object
    is never a ref). For a detection of class c, (ov_same, j_same) are the largest IoU and the lowest index among equal
    maxima over the counted objects of class c, (ov_other, j_other) the same over every other class; no objects: -inf.
    The first rule that holds decides -- so Loc is asked before Cls:
      Dupe  ov_same > t_f   (strict, as voc_eval has it)       ref j_same
      Loc   t_b <= ov_same <= t_f  (`>=` at t_b)               ref j_same
      Cls   ov_other > t_f                                     ref j_other
      Both  t_b <= ov_other <= t_f                             ref j_other
      Bkg   otherwise                                          ref -1
  * An object is detected (1), covered (2: undetected, but a Loc or Cls detection refers to it) or a Miss (3).
  * Step 3, each oracle alone on step 1's marking, then the evaluator's own curve rule: Both / Dupe / Bkg / FP remove
    their detections; Loc turns the highest-ranked Loc detection of an undetected ref into a TP and removes the other Loc
    detections; Cls turns the winner of an undetected ref (the highest score among all Cls detections with that ref
    whatever their class, equal scores to the lower detection row) into a TP of the ref's class with its own score --
    ranked again by (class, score descending, arrival) -- and removes the other Cls detections; Miss takes the missed
    objects out of npos; FN makes npos the TP count. A class whose npos is 0 under the oracle is NaN. The area metric's
    terms are the evaluator's; a repaired AP is their correctly rounded sum (double-double on the device, math.fsum in
    `tide_numpy`), so it does not depend on the order of the sum. `ap` keeps the evaluator's bits: an oracle that
    changes nothing may differ from it in the last bit.
  * `delta_map()` averages the classes that are finite under the oracle (a NaN class is left out, as `mean_ap()` does).

`tide_numpy` is these rules in plain numpy float64 (host): the tests' yardstick, pinned by the hand-worked cases of
tests/diagnose_cases.py.
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import lib
from .evaluate import DetectionEvaluator, _ap_numpy, _iou_matrix, voc_numpy

TYPE_NAMES = ("TP", "Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")          # the columns of `counts`
ORACLE_NAMES = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")  # the rows of `ap_fixed`
T_OUT, T_TP, T_CLS, T_LOC, T_BOTH, T_DUPE, T_BKG = range(7)               # det_type


def _check_thresholds(t_f, t_b):
    t_f, t_b = float(t_f), float(t_b)
    if not (0. <= t_b < t_f):  # (also refuses NaN)
        raise ValueError("diagnose: need 0 <= t_b < t_f, got t_f=%r t_b=%r" % (t_f, t_b))
    return t_f, t_b


# ---- host restatement ----------------------------------------------------------------------------------------------------

def _ap_fixed_numpy(rec, prec, use_07_metric):
    """`_ap_numpy`, with the area metric's terms -- the same rounded products, in the same float64 -- added exactly and
    rounded once (math.fsum). A repaired AP then does not depend on the order of a sum: the device adds in a workgroup's
    tree, numpy in blocks, and over some hundred terms the two orders drift apart by more than the last bit."""
    if use_07_metric:
        return _ap_numpy(rec, prec, True)
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return math.fsum(((mrec[i + 1] - mrec[i]) * mpre[i + 1]).tolist())


def _ap_by_class(codes, cls_offsets, npos, use_07_metric):
    """voc_numpy's curve rule for codes [n] by rank -> ap [C] (the area metric's sum: `_ap_fixed_numpy`)"""
    C = len(npos)
    ap = np.full(C, np.nan)
    for c in range(C):
        if npos[c] <= 0:
            continue
        f = codes[int(cls_offsets[c]):int(cls_offsets[c + 1])]
        tp = np.cumsum(f == 1).astype(np.float64)
        fp = np.cumsum(f == 2).astype(np.float64)
        rc = tp / float(npos[c])
        pr = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap[c] = _ap_fixed_numpy(rc, pr, use_07_metric)
    return ap


def _nanmean_rows(x):
    fin = ~np.isnan(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(fin, x, 0.).sum(-1) / fin.sum(-1)


def tide_numpy(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls, t_f=0.5, t_b=0.1,
               use_07_metric=False):
    """The module's rules in numpy float64 -> dict(order [n], cls_offsets [C+1], tpfp uint8 [n], npos [C], ap [C],
    det_type uint8 [n] and det_ref int64 [n] by rank, gt_state uint8 [g], counts int64 [C,7], confusion int64 [C+1,C+1],
    ap_fixed [8,C], delta_ap [8,C], delta_map [8], mean_ap)."""
    t_f, t_b = _check_thresholds(t_f, t_b)
    det = np.asarray(det, np.float32).reshape(-1, 5)
    det_img = np.asarray(det_img, np.int64).reshape(-1)
    det_cls = np.asarray(det_cls, np.int64).reshape(-1)
    gt_box = np.asarray(gt_box, np.float32).reshape(-1, 4)
    gt_img = np.asarray(gt_img, np.int64).reshape(-1)
    gt_cls = np.asarray(gt_cls, np.int64).reshape(-1)
    gt_difficult = np.asarray(gt_difficult).reshape(-1).astype(bool)
    n, g, C = det.shape[0], gt_box.shape[0], int(n_cls)
    base = voc_numpy(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, C, [t_f], use_07_metric)
    order, cls_offsets, tpfp = base["order"], base["cls_offsets"], base["tpfp"][0]
    npos, ap = base["npos"], base["ap"][:, 0]
    valid = int(cls_offsets[-1])  # the ranks behind it are the rows with ids out of range
    counted = (gt_cls >= 0) & (gt_cls < C) & (gt_img >= 0) & (gt_img < n_img) & ~gt_difficult
    gt_state = np.where(counted, 3, 0).astype(np.uint8)
    det_type = np.zeros(n, np.uint8)
    det_ref = np.full(n, -1, np.int64)
    det64, gt64 = det[:, :4].astype(np.float64), gt_box.astype(np.float64)
    # step 2, image by image: the image's ranks (every class) against its counted objects in arrival order
    rank_img = det_img[order[:valid]]
    crow = np.nonzero(counted)[0]
    crow = crow[np.argsort(gt_img[crow], kind="stable")]
    cimg = gt_img[crow]
    for im in np.unique(rank_img):
        ranks = np.nonzero(rank_img == im)[0]
        rows = crow[np.searchsorted(cimg, im, "left"):np.searchsorted(cimg, im, "right")]
        c = det_cls[order[ranks]]
        nd = ranks.size
        ov_same = np.full(nd, -np.inf)
        ov_other = np.full(nd, -np.inf)
        j_same = np.full(nd, -1, np.int64)
        j_other = np.full(nd, -1, np.int64)
        if rows.size:
            ov = _iou_matrix(det64[order[ranks]], gt64[rows])
            same = gt_cls[rows][None, :] == c[:, None]
            for mask, ovm, jm in ((same, ov_same, j_same), (~same, ov_other, j_other)):
                m = np.where(mask, ov, -np.inf)
                has = mask.any(1)
                ovm[has] = m.max(1)[has]
                jm[has] = rows[m.argmax(1)][has]  # the lowest index among equal maxima
        code = tpfp[ranks]
        fp = code == 2
        dupe = fp & (ov_same > t_f)
        loc = fp & ~dupe & (ov_same >= t_b)
        cls = fp & ~dupe & ~loc & (ov_other > t_f)
        both = fp & ~dupe & ~loc & ~cls & (ov_other >= t_b)
        bkg = fp & ~dupe & ~loc & ~cls & ~both
        ty = np.zeros(nd, np.uint8)
        ty[code == 1], ty[dupe], ty[loc], ty[cls], ty[both], ty[bkg] = T_TP, T_DUPE, T_LOC, T_CLS, T_BOTH, T_BKG
        ref = np.where((code == 1) | dupe | loc, j_same, np.where(cls | both, j_other, -1))
        det_type[ranks], det_ref[ranks] = ty, ref
    gt_state[det_ref[det_type == T_TP]] = 1
    refs = det_ref[(det_type == T_LOC) | (det_type == T_CLS)]
    refs = refs[gt_state[refs] == 3]
    gt_state[refs] = 2
    # counts and confusion
    rank_cls = np.full(n, C, np.int64)
    rank_cls[:valid] = det_cls[order[:valid]]
    counts = np.zeros((C, 7), np.int64)
    confusion = np.zeros((C + 1, C + 1), np.int64)
    typed = np.nonzero(det_type)[0]
    c, ty = rank_cls[typed], det_type[typed].astype(np.int64)
    np.add.at(counts, (c, ty - 1), 1)
    ref_cls = gt_cls[det_ref[typed]] if g else np.full(typed.size, C, np.int64)  # (a ref of -1 is not a Cls row's)
    oc = np.where(ty == T_TP, c, np.where(ty == T_CLS, ref_cls, C))
    np.add.at(confusion, (oc, c), 1)
    np.add.at(confusion, (gt_cls[gt_state >= 2], C), 1)
    np.add.at(counts, (gt_cls[gt_state == 3], 6), 1)
    # step 3
    ap_fixed = np.full((8, C), np.nan)

    def removed(sel):
        f = tpfp.copy()
        f[sel] = 0
        return f

    # Cls: the winner of each ref moves to the ref's class; all rows ranked again
    score = det[:, 4].astype(np.float64)
    code_row = np.zeros(n, np.uint8)
    code_row[order] = tpfp
    new_cls = np.full(n, C, np.int64)
    new_cls[order[:valid]] = rank_cls[:valid]
    cr = np.nonzero(det_type == T_CLS)[0]
    rows, refs = order[cr], det_ref[cr]
    code_row[rows] = 0
    by = np.lexsort((rows, -score[rows], refs))  # ref, then score descending, then the lower detection row
    first = by[np.concatenate(([True], refs[by][1:] != refs[by][:-1]))] if by.size else by
    win = first[gt_state[refs[first]] == 2]
    code_row[rows[win]] = 1
    new_cls[rows[win]] = gt_cls[refs[win]]
    order2 = np.lexsort((np.arange(n), -score, new_cls))
    offsets2 = np.searchsorted(new_cls[order2], np.arange(C + 1), side="left")
    ap_fixed[0] = _ap_by_class(code_row[order2], offsets2, npos, use_07_metric)
    # Loc: the highest-ranked Loc detection of an undetected ref becomes a TP
    lr = np.nonzero(det_type == T_LOC)[0]  # ascending ranks
    f = removed(lr)
    _, firsts = np.unique(det_ref[lr], return_index=True)
    w = lr[firsts]
    f[w[gt_state[det_ref[w]] == 2]] = 1
    ap_fixed[1] = _ap_by_class(f, cls_offsets, npos, use_07_metric)
    for o, ty in ((2, T_BOTH), (3, T_DUPE), (4, T_BKG)):
        ap_fixed[o] = _ap_by_class(removed(det_type == ty), cls_offsets, npos, use_07_metric)
    ap_fixed[5] = _ap_by_class(tpfp, cls_offsets, npos - counts[:, 6], use_07_metric)
    ap_fixed[6] = _ap_by_class(removed(tpfp == 2), cls_offsets, npos, use_07_metric)
    ap_fixed[7] = _ap_by_class(tpfp, cls_offsets, counts[:, 0], use_07_metric)
    mean_ap = float(_nanmean_rows(ap))
    return dict(order=order, cls_offsets=cls_offsets, tpfp=tpfp, npos=npos, ap=ap, det_type=det_type, det_ref=det_ref,
                gt_state=gt_state, counts=counts, confusion=confusion, ap_fixed=ap_fixed, delta_ap=ap_fixed - ap[None, :],
                delta_map=_nanmean_rows(ap_fixed) - mean_ap, mean_ap=mean_ap)


def diagnose_min_iou_margin(det, det_img, det_cls, gt_box, gt_img, gt_cls, n_img, n_cls, t_f=0.5, t_b=0.1):
    """min |IoU - t| for t in (t_b, t_f) over every detection and every object of the same image, all classes (rows with
    ids in range): fixtures assert it stays above 1e-9, so that a last-bit difference in one double division cannot
    flip a type"""
    det = np.asarray(det, np.float32).reshape(-1, 5)
    gt_box = np.asarray(gt_box, np.float32).reshape(-1, 4)
    det_img, det_cls = np.asarray(det_img, np.int64).reshape(-1), np.asarray(det_cls, np.int64).reshape(-1)
    gt_img, gt_cls = np.asarray(gt_img, np.int64).reshape(-1), np.asarray(gt_cls, np.int64).reshape(-1)
    dok = (det_cls >= 0) & (det_cls < n_cls) & (det_img >= 0) & (det_img < n_img)
    gok = (gt_cls >= 0) & (gt_cls < n_cls) & (gt_img >= 0) & (gt_img < n_img)
    thr = np.asarray([t_b, t_f], np.float64)
    margin = np.inf
    for im in np.unique(det_img[dok]):
        d, o = np.nonzero(dok & (det_img == im))[0], np.nonzero(gok & (gt_img == im))[0]
        if o.size:
            ov = _iou_matrix(det[d, :4].astype(np.float64), gt_box[o].astype(np.float64))
            margin = min(margin, float(np.abs(ov[:, :, None] - thr[None, None, :]).min()))
    return margin


# ---- device ----------------------------------------------------------------------------------------------------------------

def diagnose_errors(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls, thresholds,
                    use_07_metric=False):
    """One `dana_diagnose_errors` call on device tensors (det [n,5] float32, ids int32, gt_difficult uint8, thresholds
    float64 [2] = (t_f, t_b) with 0 <= t_b < t_f) -> DiagnosisResult. No synchronisation, no device-to-host copy."""
    det = ops._chk(det, "det")
    dev = det.device
    n, g, C = det.size(0), gt_box.size(0), int(n_cls)
    ops._chk(det_img, "det_img", torch.int32), ops._chk(det_cls, "det_cls", torch.int32)
    ops._chk(gt_box, "gt_box"), ops._chk(gt_img, "gt_img", torch.int32), ops._chk(gt_cls, "gt_cls", torch.int32)
    ops._chk(gt_difficult, "gt_difficult", torch.uint8), ops._chk(thresholds, "thresholds", torch.float64)
    if det_img.numel() != n or det_cls.numel() != n or gt_img.numel() != g or gt_cls.numel() != g or gt_difficult.numel() != g:
        raise ValueError("diagnose_errors: id tensors do not match %d detections / %d ground-truth boxes" % (n, g))
    if thresholds.numel() != 2:
        raise ValueError("diagnose_errors: thresholds are the two doubles (t_f, t_b)")
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    order, cls_offsets, npos, det_ref = i32(n), i32(C + 1), i32(C), i32(n)
    tpfp, det_type, gt_state = u8(n), u8(n), u8(g)
    ap = torch.empty((C,), dtype=torch.float64, device=dev)
    ap_fixed = torch.empty((8, C), dtype=torch.float64, device=dev)
    counts = torch.empty((C, 7), dtype=torch.int64, device=dev)
    confusion = torch.empty((C + 1, C + 1), dtype=torch.int64, device=dev)
    size = lib().query("dana_diagnose_errors_workspace_bytes", n, g, int(n_img), C)
    if size == 0:
        raise ValueError("diagnose_errors: shape refused (n=%d g=%d n_img=%d n_cls=%d)" % (n, g, n_img, C))
    ws = ops._ws(size, dev)
    lib().call("dana_diagnose_errors", ops._p(det), ops._p(det_img), ops._p(det_cls), n, ops._p(gt_box), ops._p(gt_img),
               ops._p(gt_cls), ops._p(gt_difficult), g, int(n_img), C, ops._p(thresholds), int(bool(use_07_metric)),
               ops._p(order), ops._p(cls_offsets), ops._p(tpfp), ops._p(npos), ops._p(ap), ops._p(det_type),
               ops._p(det_ref), ops._p(gt_state), ops._p(counts), ops._p(confusion), ops._p(ap_fixed), ops._p(ws),
               ws.numel(), ops._stream())
    return DiagnosisResult(ap, npos, order, cls_offsets, tpfp, det_type, det_ref, gt_state, counts, confusion, ap_fixed,
                           thresholds)


class DiagnosisResult:
    """Device tensors of one `compute()`: step 1 as `EvalResult` has it (ap [C] float64, npos [C], order [n], cls_offsets
    [C+1], tpfp uint8 [n] by rank); det_type uint8 [n] and det_ref int32 [n] by rank; gt_state uint8 [g] by the caller's
    row; counts int64 [C,7] (TYPE_NAMES); confusion int64 [C+1,C+1] ([object class][detection class]); ap_fixed float64
    [8,C] (ORACLE_NAMES)."""

    def __init__(self, ap, npos, order, cls_offsets, tpfp, det_type, det_ref, gt_state, counts, confusion, ap_fixed,
                 thresholds):
        self.ap, self.npos, self.order, self.cls_offsets, self.tpfp = ap, npos, order, cls_offsets, tpfp
        self.det_type, self.det_ref, self.gt_state = det_type, det_ref, gt_state
        self.counts, self.confusion, self.ap_fixed, self.thresholds = counts, confusion, ap_fixed, thresholds

    def mean_ap(self):
        """-> 0-d float64 device tensor: the mean over the classes that have non-difficult ground truth"""
        has = (self.npos > 0).to(torch.float64).unsqueeze(1)  # (EvalResult.mean_ap's expression, for its bits)
        ap = self.ap.unsqueeze(1)
        return (torch.where(has > 0, ap, torch.zeros_like(ap)).sum(0) / has.sum(0))[0]

    def delta_ap(self):
        """-> [8,C]: what repairing each error type alone adds to each class's AP (NaN where either side is)"""
        return self.ap_fixed - self.ap.unsqueeze(0)

    def delta_map(self):
        """-> [8]: the mean over the classes finite under the oracle, minus `mean_ap()`"""
        fin = ~torch.isnan(self.ap_fixed)
        return torch.where(fin, self.ap_fixed, torch.zeros_like(self.ap_fixed)).sum(1) / fin.sum(1) - self.mean_ap()

    def summary(self):
        """The one method that reads from the device (one copy) -> dict of host numbers: mean_ap, count[type name] summed
        over the classes, delta_map[oracle name], and per class ap [C], delta_ap[oracle name] [C], count_by_class
        [type name] [C]."""
        C = self.ap.numel()
        flat = torch.cat([self.mean_ap().reshape(1), self.delta_map(), self.ap, self.delta_ap().reshape(-1),
                          self.counts.to(torch.float64).reshape(-1)]).cpu().numpy()  # counts < 2^53: exact
        dap = flat[9 + C:9 + 9 * C].reshape(8, C)
        cnt = flat[9 + 9 * C:].reshape(C, 7).astype(np.int64)
        return dict(mean_ap=float(flat[0]), delta_map={k: float(flat[1 + o]) for o, k in enumerate(ORACLE_NAMES)},
                    count={k: int(cnt[:, j].sum()) for j, k in enumerate(TYPE_NAMES)}, ap=flat[9:9 + C].tolist(),
                    delta_ap={k: dap[o].tolist() for o, k in enumerate(ORACLE_NAMES)},
                    count_by_class={k: cnt[:, j].tolist() for j, k in enumerate(TYPE_NAMES)})


class DetectionDiagnoser(DetectionEvaluator):
    """A `DetectionEvaluator` at one foreground threshold t_f and one background threshold t_b (0 <= t_b < t_f): the same
    `add_*` and `add_ground_truth*` methods; `compute()` -> DiagnosisResult (device tensors; nothing is read back)."""

    def __init__(self, num_classes, t_f=0.5, t_b=0.1, use_07_metric=False, device="cuda"):
        self.t_f, self.t_b = _check_thresholds(t_f, t_b)
        super().__init__(num_classes, (self.t_f,), use_07_metric, device)
        self.thresholds = torch.from_numpy(np.asarray([self.t_f, self.t_b], np.float64)).to(self.device)

    def compute(self):
        gbox, gimg, gcls, gdiff = self._ground_truth()
        det, img, cls = self._detections()
        return diagnose_errors(det, img, cls, gbox, gimg, gcls, gdiff, max(self.num_images, 1), self.num_classes,
                               self.thresholds, self.use_07_metric)


def all_boxes_arrays(all_boxes, ground_truth, add_one=False):
    """The reference's all_boxes[j][i] ([k,5] of class j on image i, an empty list where nothing was detected) and
    ground_truth[i] = (boxes [k,4], labels [k], difficult [k] or None) -> dict of the packed host arrays (det, det_img,
    det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls): rows class by class, image by image."""
    C = len(all_boxes)
    n_img = len(ground_truth)
    rows, imgs, clss = [np.zeros((0, 5), np.float32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    for j in range(C):
        for i in range(len(all_boxes[j])):
            d = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            rows.append(d)
            imgs.append(np.full(d.shape[0], i, np.int32))
            clss.append(np.full(d.shape[0], j, np.int32))
            n_img = max(n_img, i + 1)
    det = np.concatenate(rows, 0)
    if add_one:
        det[:, :4] += 1.
    gb, gi, gc, gd = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros(0, np.uint8)]
    for i, gt in enumerate(ground_truth):
        b = np.asarray(gt[0], np.float32).reshape(-1, 4)
        lab = np.asarray(gt[1], np.int32).reshape(-1)
        diff = gt[2] if len(gt) > 2 and gt[2] is not None else np.zeros(b.shape[0])
        diff = (np.asarray(diff).reshape(-1) != 0).astype(np.uint8)
        if lab.size != b.shape[0] or diff.size != b.shape[0]:
            raise ValueError("ground_truth[%d]: %d boxes, %d labels, %d difficult flags" % (i, b.shape[0], lab.size, diff.size))
        gb.append(b), gi.append(np.full(b.shape[0], i, np.int32)), gc.append(lab), gd.append(diff)
    return dict(det=det, det_img=np.concatenate(imgs), det_cls=np.concatenate(clss), gt_box=np.concatenate(gb, 0),
                gt_img=np.concatenate(gi), gt_cls=np.concatenate(gc), gt_difficult=np.concatenate(gd), n_img=n_img, n_cls=C)


def diagnose_all_boxes(all_boxes, ground_truth, t_f=0.5, t_b=0.1, use_07_metric=False, device="cuda", add_one=False):
    """`evaluate_all_boxes`' counterpart: the reference's all_boxes[j][i] and ground_truth[i] = (boxes, labels, difficult
    or None) -> DiagnosisResult. add_one=True adds 1 to the detection coordinates first (pascal_voc.py:288-291)."""
    a = all_boxes_arrays(all_boxes, ground_truth, add_one)
    dg = DetectionDiagnoser(a["n_cls"], t_f, t_b, use_07_metric, device)
    dg.add_ground_truth_packed(a["gt_box"], a["gt_img"], a["gt_cls"], a["gt_difficult"], num_images=a["n_img"])
    dg.add_packed(a["det"], a["det_img"], a["det_cls"], num_images=a["n_img"])
    return dg.compute()
