"""Emit tests/golden/eval_voc.npz: a small detection set with the REFERENCE's own answers from lib/datasets/voc_eval.py.

The reference module is loaded by file path (it imports only the standard library and numpy) and driven the way
pascal_voc.py drives it: VOC XML annotations, an image-set file and one detection file per class in a temporary
directory, then `voc_eval` for every class, for the ten thresholds np.arange(0.5, 0.96, 0.05) and for both metrics.
Floats are written with repr, so the float32 inputs survive the text round trip exactly. The file stores the inputs and
the reference's rec / prec / ap -- nothing of the reference's text.

Content the tests rely on: difficult boxes, duplicated ground-truth boxes (an argmax tie), images without ground
truth, detections on images without ground truth of their class, one (class, image) with more than 64 boxes, every
class with npos > 0. Asserted, with the seed redrawn otherwise: scores pairwise distinct within a class (the
reference's argsort is not stable) and |IoU - thr| >= 1e-9 for every (detection, box, threshold).

Run in the build container only:  python tests/golden/make_eval_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from dana_amd import evaluate as E  # noqa: E402

N_IMG, N_CLS, MAX_DET = 120, 4, 10
THR = np.arange(0.5, 0.96, 0.05)


def draw(seed):
    rng = np.random.RandomState(seed)
    gt_box, gt_img, gt_cls, gt_diff = [], [], [], []
    for i in range(N_IMG):
        if i % 9 == 4:
            continue  # an image without ground truth
        for c in range(N_CLS):
            k = int(rng.randint(0, 4))
            if (i, c) == (7, 2):
                k = 70  # more than one 64-lane chunk
            for q in range(k):
                x1, y1 = int(rng.randint(0, 400)), int(rng.randint(0, 300))
                w, h = int(rng.randint(20, 200)), int(rng.randint(20, 200))
                box = [x1, y1, x1 + w, y1 + h]
                if q and rng.rand() < 0.15:
                    box = list(gt_box[-1])  # a duplicate of the previous box of this (image, class): an argmax tie
                gt_box.append(box)
                gt_img.append(i)
                gt_cls.append(c)
                gt_diff.append(int(rng.rand() < 0.2))
    gt_box = np.asarray(gt_box, np.float32)
    gt_img, gt_cls, gt_diff = np.asarray(gt_img, np.int32), np.asarray(gt_cls, np.int32), np.asarray(gt_diff, np.uint8)
    det, det_img, det_cls = [], [], []
    for i in range(N_IMG):
        for c in range(N_CLS):
            mine = np.nonzero((gt_img == i) & (gt_cls == c))[0]
            for _ in range(int(rng.randint(0, MAX_DET + 1))):
                if mine.size and rng.rand() < 0.7:  # a jittered copy of one of the boxes
                    b = gt_box[mine[rng.randint(mine.size)]] + rng.uniform(-1, 1, 4) * rng.choice([2., 8., 25.])
                else:
                    x1, y1 = rng.uniform(0, 400), rng.uniform(0, 300)
                    b = np.asarray([x1, y1, x1 + rng.uniform(20, 200), y1 + rng.uniform(20, 200)])
                b[2], b[3] = max(b[2], b[0] + 1.), max(b[3], b[1] + 1.)
                det.append(b)
                det_img.append(i)
                det_cls.append(c)
    det = np.asarray(det, np.float32)
    det_img, det_cls = np.asarray(det_img, np.int32), np.asarray(det_cls, np.int32)
    score = np.zeros(det.shape[0], np.float32)
    for c in range(N_CLS):  # a permutation of distinct values: no ties within a class
        sel = np.nonzero(det_cls == c)[0]
        score[sel] = ((rng.permutation(sel.size) + 1.0) / (sel.size + 1.0)).astype(np.float32)
    det = np.concatenate((det, score[:, None]), 1).astype(np.float32)
    return det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_diff


def conditions_hold(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_diff):
    for c in range(N_CLS):
        s = det[det_cls == c, 4]
        if np.unique(s).size != s.size or not ((gt_cls == c) & (gt_diff == 0)).any():
            return False
    if not (gt_diff == 1).any():
        return False
    return E.min_iou_margin(det, det_img, det_cls, gt_box, gt_img, gt_cls, N_IMG, THR) >= 1e-9


def run_reference(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_diff):
    spec = importlib.util.spec_from_file_location("ref_voc_eval", os.path.join(ref_import.REF, "lib", "datasets", "voc_eval.py"))
    ref = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(ref)
    n = det.shape[0]
    order = np.lexsort((-det[:, 4].astype(np.float64), det_cls))
    rec = np.zeros((THR.size, n))
    prec = np.zeros((THR.size, n))
    ap = np.zeros((2, N_CLS, THR.size))
    with tempfile.TemporaryDirectory() as tmp:
        names = ["img%04d" % i for i in range(N_IMG)]
        with open(os.path.join(tmp, "set.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        for i, name in enumerate(names):
            objs = []
            for j in np.nonzero(gt_img == i)[0]:
                b = gt_box[j]
                objs.append("<object><name>c%d</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                            "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                            % (gt_cls[j], gt_diff[j], b[0], b[1], b[2], b[3]))
            with open(os.path.join(tmp, name + ".xml"), "w") as f:
                f.write("<annotation>" + "".join(objs) + "</annotation>")
        for c in range(N_CLS):
            with open(os.path.join(tmp, "det_c%d.txt" % c), "w") as f:
                for k in np.nonzero(det_cls == c)[0]:
                    f.write("%s %s %s %s %s %s\n" % ((names[det_img[k]], repr(float(det[k, 4]))) +
                                                     tuple(repr(float(v)) for v in det[k, :4])))
        pos = 0
        for c in range(N_CLS):
            nc = int((det_cls == c).sum())
            for t, thr in enumerate(THR):
                for m, use07 in enumerate((False, True)):
                    with contextlib.redirect_stdout(io.StringIO()):
                        r, p, a = ref.voc_eval(os.path.join(tmp, "det_{:s}.txt"), os.path.join(tmp, "{:s}.xml"),
                                               os.path.join(tmp, "set.txt"), "c%d" % c, os.path.join(tmp, "cache"),
                                               ovthresh=thr, use_07_metric=use07)
                    assert r.shape == (nc,)
                    rec[t, pos:pos + nc], prec[t, pos:pos + nc] = r, p
                    ap[m, c, t] = a
            pos += nc
    return order, rec, prec, ap


def main():
    if not ref_import.available():
        raise SystemExit("the reference tree is not on this machine")
    seed = 20
    while True:
        data = draw(seed)
        if conditions_hold(*data):
            break
        seed += 1
    det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_diff = data
    assert ((gt_img == 7) & (gt_cls == 2)).sum() > 64
    order, rec, prec, ap = run_reference(*data)
    out = os.path.join(HERE, "eval_voc.npz")
    np.savez_compressed(out, det=det, det_img=det_img, det_cls=det_cls, gt_box=gt_box, gt_img=gt_img, gt_cls=gt_cls,
                        gt_difficult=gt_diff, n_img=np.int32(N_IMG), n_cls=np.int32(N_CLS), iou_thr=THR, seed=np.int32(seed),
                        ref_order=order.astype(np.int32), ref_rec=rec, ref_prec=prec, ref_ap_area=ap[0], ref_ap_07=ap[1])
    print("wrote %s: seed %d, %d detections, %d boxes, %d bytes" % (out, seed, det.shape[0], gt_box.shape[0], os.path.getsize(out)))


if __name__ == "__main__":
    main()
