"""Cases for the error diagnosis (dana_amd/diagnose.py), shared by tests/test_diagnose_host.py and
tests/test_gpu_diagnose.py.

`hand_cases()`: small inputs whose answers were worked out by hand from the rules in the module's docstring, not taken
from any code. t_f = 0.5, t_b = 0.1, the area metric unless a case says otherwise. Boxes are 100 x 100 pixels under the
`+ 1.` convention, so the IoUs are simple fractions:
  * the same box: 1;
  * shifted by 2 pixels along one axis: 98 * 100 / (2 * 10000 - 9800) = 9800 / 10200;
  * shifted by 50 pixels along one axis: 5000 / 15000 = 1 / 3;
  * disjoint: 0.
`det_type`, `det_ref` are by rank; NaN in an expected AP means "NaN there".

`random_case()` / `find_case()`: seeded inputs for the restatement and the device, drawn again until no IoU of a
detection with an object of its image sits within 1e-9 of a threshold (`diagnose_min_iou_margin`).
"""
import numpy as np

from dana_amd import diagnose as D

NAN = float("nan")
TP, CLS, LOC, BOTH, DUPE, BKG = 1, 2, 3, 4, 5, 6
ARG_NAMES = ("det", "det_img", "det_cls", "gt_box", "gt_img", "gt_cls", "gt_difficult", "n_img", "n_cls")


def _args(det, det_img, det_cls, gt_box, gt_img, gt_cls, gt_difficult, n_img, n_cls):
    return dict(det=np.asarray(det, np.float32).reshape(-1, 5), det_img=np.asarray(det_img, np.int32),
                det_cls=np.asarray(det_cls, np.int32), gt_box=np.asarray(gt_box, np.float32).reshape(-1, 4),
                gt_img=np.asarray(gt_img, np.int32), gt_cls=np.asarray(gt_cls, np.int32),
                gt_difficult=np.asarray(gt_difficult, np.uint8), n_img=n_img, n_cls=n_cls)


def hand_cases():
    cases = {}
    # ---- the six types at once (the issue's case). Objects A0, A1 of class 0, B0, B1 of class 1; class 0 detects, class 1
    # does not. Rank = row. TP on A0; a 2-pixel shift of A0 is a Dupe (9800/10200 > 0.5, A0 taken); a 50-pixel shift of A1
    # is a Loc (1/3); B0's own box under class 0 is a Cls; a 50-pixel shift of B0 is a Both; a far box is Bkg.
    # A1 and B0 are covered (2), B1 is missed (3).
    # ap[0]: codes 1,2,2,2,2,2 with npos 2: recall 0.5 at precision 1 -> 0.5. ap[1]: no detections, npos 2 -> 0.
    # Loc oracle: rank 2 becomes a TP (A1 undetected): codes 1,2,1,2,2,2 -> recall 0.5 at envelope 1, recall 1 at 2/3.
    # Cls oracle: rank 3 moves to class 1 as a TP with score .6: class 1 has one TP of npos 2 -> 0.5; class 0 keeps 0.5.
    # Both / Dupe / Bkg / FP remove false positives behind the only TP: nothing changes. Miss: npos[1] = 2 - 1, still no
    # detections -> 0. FN: npos = TP counts (1, 0): class 0 has recall 1 at precision 1 -> 1, class 1 -> NaN.
    cases["six_types"] = dict(
        args=_args(det=[[0, 0, 99, 99, .9], [2, 0, 101, 99, .8], [0, 250, 99, 349, .7], [200, 0, 299, 99, .6],
                        [250, 0, 349, 99, .5], [500, 500, 599, 599, .4]],
                   det_img=[0] * 6, det_cls=[0] * 6,
                   gt_box=[[0, 0, 99, 99], [0, 200, 99, 299], [200, 0, 299, 99], [400, 0, 499, 99]],
                   gt_img=[0] * 4, gt_cls=[0, 0, 1, 1], gt_difficult=[0] * 4, n_img=1, n_cls=2),
        expect=dict(order=[0, 1, 2, 3, 4, 5], cls_offsets=[0, 6, 6], det_type=[TP, DUPE, LOC, CLS, BOTH, BKG],
                    det_ref=[0, 0, 1, 2, 2, -1], gt_state=[1, 2, 2, 3],
                    counts=[[1, 1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0, 1]],
                    confusion=[[1, 0, 1], [1, 0, 2], [4, 0, 0]], npos=[2, 2], ap=[0.5, 0.],
                    ap_fixed=dict(Cls=[0.5, 0.5], Loc=[0.5 + 0.5 * (2. / 3.), 0.], Both=[0.5, 0.], Dupe=[0.5, 0.],
                                  Bkg=[0.5, 0.], Miss=[0.5, 0.], FP=[0.5, 0.], FN=[1.0, NAN]),
                    mean_ap=0.25,
                    delta_map=dict(Cls=0.25, Loc=0.5 * (0.5 + 0.5 * (2. / 3.)) - 0.25, Both=0., Dupe=0., Bkg=0., Miss=0.,
                                   FP=0., FN=0.75)))
    # ---- a Loc whose ref is already detected. One object A; the 50-pixel shift (score .95, IoU 1/3) ranks above A's own box
    # (.9). Codes 2,1 with npos 1: recall 1 at precision 1/2 -> ap 0.5. The Loc's ref A is detected (state 1), so the Loc
    # oracle removes it and turns nothing into a TP: codes 0,1 -> 1.0, the same as the FP oracle; one TP either way.
    cases["loc_ref_detected"] = dict(
        args=_args(det=[[0, 50, 99, 149, .95], [0, 0, 99, 99, .9]], det_img=[0, 0], det_cls=[0, 0], gt_box=[[0, 0, 99, 99]],
                   gt_img=[0], gt_cls=[0], gt_difficult=[0], n_img=1, n_cls=1),
        expect=dict(order=[0, 1], cls_offsets=[0, 2], det_type=[LOC, TP], det_ref=[0, 0], gt_state=[1],
                    counts=[[1, 0, 1, 0, 0, 0, 0]], confusion=[[1, 0], [1, 0]], npos=[1], ap=[0.5],
                    ap_fixed=dict(Cls=[0.5], Loc=[1.0], Both=[0.5], Dupe=[0.5], Bkg=[0.5], Miss=[0.5], FP=[1.0], FN=[0.5]),
                    mean_ap=0.5, delta_map=dict(Loc=0.5, FP=0.5, Cls=0., FN=0.)))
    # ---- two classes' Cls detections on one object, equal scores. Object X of class 2. Row 0 (class 1) and row 1 (class 0)
    # are X's own box at score .7; row 2 is a class-2 detection far away at .8 (Bkg). Ranks run class by class: rank 0 = row
    # 1, rank 1 = row 0, rank 2 = row 2. X is covered (2). Classes 0 and 1 have no objects: NaN everywhere. ap[2]: one FP,
    # npos 1 -> 0. Cls oracle: the lower row (row 0) wins X and moves to class 2, row 1 is removed; class 2 is then ranked
    # .8 (FP), .7 (TP): recall 1 at precision 1/2 -> 0.5. Had both moved the class would hold two TPs of one object.
    # Bkg / FP oracles: class 2 has no detections left -> 0. Miss: X is covered, not missed: npos stays 1 -> 0. FN: no TP -> NaN.
    cases["cls_tie"] = dict(
        args=_args(det=[[0, 0, 99, 99, .7], [0, 0, 99, 99, .7], [500, 500, 599, 599, .8]], det_img=[0, 0, 0],
                   det_cls=[1, 0, 2], gt_box=[[0, 0, 99, 99]], gt_img=[0], gt_cls=[2], gt_difficult=[0], n_img=1, n_cls=3),
        expect=dict(order=[1, 0, 2], cls_offsets=[0, 1, 2, 3], det_type=[CLS, CLS, BKG], det_ref=[0, 0, -1], gt_state=[2],
                    counts=[[0, 1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0]],
                    confusion=[[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 1], [0, 0, 1, 0]], npos=[0, 0, 1], ap=[NAN, NAN, 0.],
                    ap_fixed=dict(Cls=[NAN, NAN, 0.5], Loc=[NAN, NAN, 0.], Both=[NAN, NAN, 0.], Dupe=[NAN, NAN, 0.],
                                  Bkg=[NAN, NAN, 0.], Miss=[NAN, NAN, 0.], FP=[NAN, NAN, 0.], FN=[NAN, NAN, NAN]),
                    mean_ap=0., delta_map=dict(Cls=0.5, Loc=0., Miss=0., FN=NAN)))
    # ---- a difficult object. D (difficult) and E (200 pixels away), class 0. Rank 0 is D's own box: step 1 matches the
    # difficult box, code 0, type 0, no ref. Rank 1 is a 50-pixel shift of D: step 1 sees IoU 1/3 -> FP; step 2 does not look
    # at D, and E is disjoint (IoU 0 < t_b) -> Bkg, not Loc. Rank 2 is E's own box: TP. Codes 0,2,1 with npos 1: recall 1 at
    # precision 1/2 -> 0.5; without the Bkg detection -> 1.0.
    cases["difficult"] = dict(
        args=_args(det=[[0, 0, 99, 99, .9], [0, 50, 99, 149, .8], [200, 0, 299, 99, .7]], det_img=[0] * 3, det_cls=[0] * 3,
                   gt_box=[[0, 0, 99, 99], [200, 0, 299, 99]], gt_img=[0, 0], gt_cls=[0, 0], gt_difficult=[1, 0], n_img=1,
                   n_cls=1),
        expect=dict(order=[0, 1, 2], cls_offsets=[0, 3], det_type=[0, BKG, TP], det_ref=[-1, -1, 1], gt_state=[0, 1],
                    counts=[[1, 0, 0, 0, 0, 1, 0]], confusion=[[1, 0], [1, 0]], npos=[1], ap=[0.5],
                    ap_fixed=dict(Cls=[0.5], Loc=[0.5], Both=[0.5], Dupe=[0.5], Bkg=[1.0], Miss=[0.5], FP=[1.0], FN=[0.5]),
                    mean_ap=0.5, delta_map=dict(Bkg=0.5, FP=0.5, Loc=0.)))
    # ---- rows out of range. One image, one class. Ground-truth rows 1 (image 3) and 2 (class 5) and detection rows 1
    # (image 7) and 2 (class -1) take no part: the detections are ranked last (by score), type 0, and the objects have state 0.
    # What is left is one TP of one object: every AP is 1.
    cases["out_of_range"] = dict(
        args=_args(det=[[0, 0, 99, 99, .9], [0, 0, 99, 99, .95], [0, 0, 99, 99, .5]], det_img=[0, 7, 0], det_cls=[0, 0, -1],
                   gt_box=[[0, 0, 99, 99]] * 3, gt_img=[0, 3, 0], gt_cls=[0, 0, 5], gt_difficult=[0] * 3, n_img=1, n_cls=1),
        expect=dict(order=[0, 1, 2], cls_offsets=[0, 1], det_type=[TP, 0, 0], det_ref=[0, -1, -1], gt_state=[1, 0, 0],
                    counts=[[1, 0, 0, 0, 0, 0, 0]], confusion=[[1, 0], [0, 0]], npos=[1], ap=[1.0],
                    ap_fixed={k: [1.0] for k in D.ORACLE_NAMES}, mean_ap=1.0, delta_map={k: 0. for k in D.ORACLE_NAMES}))
    # ---- an image with no objects. The one object (class 0) is in image 0, both detections (class 0 and class 1) in image 1:
    # all Bkg, the object is missed. ap = (0, NaN). Miss: npos[0] = 1 - 1 = 0 -> NaN (the class that turns NaN had AP 0);
    # FN: no TP -> NaN. No finite class under Miss / FN: their delta_map is NaN.
    cases["image_without_objects"] = dict(
        args=_args(det=[[0, 0, 99, 99, .9], [10, 10, 50, 50, .8]], det_img=[1, 1], det_cls=[0, 1], gt_box=[[0, 0, 99, 99]],
                   gt_img=[0], gt_cls=[0], gt_difficult=[0], n_img=2, n_cls=2),
        expect=dict(order=[0, 1], cls_offsets=[0, 1, 2], det_type=[BKG, BKG], det_ref=[-1, -1], gt_state=[3],
                    counts=[[0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 1, 0]], confusion=[[0, 0, 1], [0, 0, 0], [1, 1, 0]],
                    npos=[1, 0], ap=[0., NAN],
                    ap_fixed=dict(Cls=[0., NAN], Loc=[0., NAN], Both=[0., NAN], Dupe=[0., NAN], Bkg=[0., NAN],
                                  Miss=[NAN, NAN], FP=[0., NAN], FN=[NAN, NAN]),
                    mean_ap=0., delta_map=dict(Bkg=0., FP=0., Miss=NAN, FN=NAN)))
    # ---- a class with objects and no detections. A (class 0) is detected by its own box, B (class 1) has no detection of
    # any class near it: a Miss. ap = (1, 0). Miss and FN leave class 1 without positives -> NaN, so their mean runs over
    # class 0 alone: 1 - 0.5.
    cases["class_without_detections"] = dict(
        args=_args(det=[[0, 0, 99, 99, .9]], det_img=[0], det_cls=[0], gt_box=[[0, 0, 99, 99], [300, 300, 399, 399]],
                   gt_img=[0, 0], gt_cls=[0, 1], gt_difficult=[0, 0], n_img=1, n_cls=2),
        expect=dict(order=[0], cls_offsets=[0, 1, 1], det_type=[TP], det_ref=[0], gt_state=[1, 3],
                    counts=[[1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1]], confusion=[[1, 0, 0], [0, 0, 1], [0, 0, 0]],
                    npos=[1, 1], ap=[1.0, 0.],
                    ap_fixed=dict(Cls=[1., 0.], Loc=[1., 0.], Both=[1., 0.], Dupe=[1., 0.], Bkg=[1., 0.], Miss=[1., NAN],
                                  FP=[1., 0.], FN=[1., NAN]),
                    mean_ap=0.5, delta_map=dict(Cls=0., Miss=0.5, FN=0.5)))
    return cases


def random_case(seed, n_img, n_cls, objs_per_img, dets_per_seg, difficult=0.2, tie_scores=False, stray=0):
    """Objects of random classes; a detection of (class c, image i) is, a third each, a slightly jittered copy of ANY object
    of its image (a TP or Dupe when the class agrees, a Cls when not), a copy shifted by 20-70 % of its size (Loc / Both),
    or an unrelated box. `stray` rows with ids out of range are appended to both lists. Arrival order is shuffled."""
    rng = np.random.RandomState(seed)
    gb, gi, gc = [], [], []
    for i in range(n_img):
        for _ in range(objs_per_img(i)):
            x, y = rng.randint(0, 600, 2)
            gb.append([x, y, x + rng.randint(20, 160), y + rng.randint(20, 160)])
            gi.append(i)
            gc.append(rng.randint(n_cls))
    gb = np.asarray(gb, np.float32).reshape(-1, 4)
    gi, gc = np.asarray(gi, np.int32), np.asarray(gc, np.int32)
    db, di, dc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            mine = np.nonzero(gi == i)[0]
            for _ in range(dets_per_seg(c, i)):
                u = rng.rand()
                if mine.size and u < 0.66:
                    b = gb[mine[rng.randint(mine.size)]].astype(np.float64)
                    w, h = b[2] - b[0], b[3] - b[1]
                    if u < 0.33:
                        b = b + rng.uniform(-4, 4, 4)
                    else:
                        sx, sy = rng.uniform(0.2, 0.7) * w * rng.choice([-1, 1]), rng.uniform(0, 0.3) * h
                        b = b + np.asarray([sx, sy, sx, sy]) + rng.uniform(-1, 1, 4)
                else:
                    x, y = rng.uniform(0, 600, 2)
                    b = np.asarray([x, y, x + rng.uniform(20, 160), y + rng.uniform(20, 160)])
                db.append(b)
                di.append(i)
                dc.append(c)
    for k in range(stray):  # ids out of range, boxes on top of real objects
        db.append(gb[k % max(len(gb), 1)].astype(np.float64) if len(gb) else np.asarray([0., 0., 50., 50.]))
        di.append([n_img, 0, -1][k % 3])
        dc.append([0, n_cls, 0][k % 3])
    n = len(db)
    score = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    if tie_scores:
        score = (np.floor(score * 4) / 4).astype(np.float32)  # four distinct values: ranks and claims decided by arrival
    perm = rng.permutation(n)
    det = np.concatenate((np.asarray(db, np.float64).reshape(-1, 4), score[:, None]), 1).astype(np.float32)[perm]
    diff = (rng.rand(gb.shape[0]) < difficult).astype(np.uint8)
    if stray and len(gb):
        gb = np.concatenate((gb, gb[:stray]))
        gi = np.concatenate((gi, np.asarray([[n_img, 0, -1][k % 3] for k in range(min(stray, len(diff)))], np.int32)))
        gc = np.concatenate((gc, np.asarray([[0, n_cls, 0][k % 3] for k in range(min(stray, len(diff)))], np.int32)))
        diff = np.concatenate((diff, np.zeros(min(stray, len(diff)), np.uint8)))
    return dict(det=det, det_img=np.asarray(di, np.int32)[perm], det_cls=np.asarray(dc, np.int32)[perm], gt_box=gb,
                gt_img=gi, gt_cls=gc, gt_difficult=diff, n_img=n_img, n_cls=n_cls)


def contested_case(seed, n_cls=5, per_class=40):
    """One object of class 0 in one image, and per_class near-copies of it under EVERY class with tied scores: the other
    classes' rows are Cls detections fighting for one ref (the winner is decided by score, then row), class 0's own rows a
    TP and Dupes. A second image holds an object of the last class, which has no detections anywhere; only class 1 and
    class 2 claim it, so the Cls oracle moves a row into a class that had no detections of its own."""
    rng = np.random.RandomState(seed)
    gb = np.asarray([[100, 100, 260, 240], [300, 50, 420, 200]], np.float32)
    db, di, dc = [], [], []
    for c in range(n_cls - 1):
        for _ in range(per_class):
            db.append(gb[0] + rng.uniform(-5, 5, 4)), di.append(0), dc.append(c)
    for c in (1, 2):
        for _ in range(7):
            db.append(gb[1] + rng.uniform(-5, 5, 4)), di.append(1), dc.append(c)
    n = len(db)
    score = (np.floor(rng.rand(n) * 5) / 5 + 0.1).astype(np.float32)
    det = np.concatenate((np.asarray(db), score[:, None]), 1).astype(np.float32)
    return dict(det=det, det_img=np.asarray(di, np.int32), det_cls=np.asarray(dc, np.int32), gt_box=gb,
                gt_img=np.asarray([0, 1], np.int32), gt_cls=np.asarray([0, n_cls - 1], np.int32),
                gt_difficult=np.zeros(2, np.uint8), n_img=2, n_cls=n_cls)


def margin(case, t_f=0.5, t_b=0.1):
    return D.diagnose_min_iou_margin(case["det"], case["det_img"], case["det_cls"], case["gt_box"], case["gt_img"],
                                     case["gt_cls"], case["n_img"], case["n_cls"], t_f, t_b)


def find_case(make, seed, t_f=0.5, t_b=0.1, tries=20):
    """the first of make(seed), make(seed + 1), ... whose IoUs all stay 1e-9 away from both thresholds; none: an error"""
    for s in range(seed, seed + tries):
        case = make(s)
        if margin(case, t_f, t_b) >= 1e-9:
            return case
    raise AssertionError("no seed in %d..%d with the 1e-9 IoU margin" % (seed, seed + tries - 1))


def host(case, t_f=0.5, t_b=0.1, use_07_metric=False):
    return D.tide_numpy(*[case[k] for k in ARG_NAMES], t_f, t_b, use_07_metric)
