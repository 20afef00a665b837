"""Host-side checks of the COCO-protocol evaluator (dana_amd/evaluate.py): `coco_numpy`, the numpy restatement of
COCOeval's evaluateImg / accumulate / summarize for boxes, against hand-worked cases and -- where the two protocols must
agree -- against the reference-pinned `voc_numpy`; and the argument validation of the C entry points, which answers
before any HIP call. pycocotools is not part of the reference tree, so no fixture could be generated from it."""
import inspect
import os

import numpy as np
import pytest

from coco_cases import HAND_THRS, disjoint_case, hand_case, mean_valid
from dana_amd import _lib, evaluate as E

EPS = 2.0 ** -52
ONE = 1.0 / (1.0 + EPS)  # tp / (fp + tp + eps) with tp = 1, fp = 0


def _hand(name):
    d = hand_case(name)
    r = E.coco_numpy(d["det"], d["det_img"], d["det_cls"], d["gt_bbox"], d["gt_img"], d["gt_cls"], 1, 1, d["gt_iscrowd"],
                     d["gt_area"], d["gt_ignore"], iou_thrs=HAND_THRS)
    ap = lambda t, a, m: mean_valid(r["precision"][t, :, 0, a, m])
    ar = lambda t, a, m: float(r["recall"][t, 0, a, m])
    return r, ap, ar


def _eq(got, want):
    assert abs(got - want) <= 1e-12, (got, want)


def test_hand_case_crowd():
    r, ap, ar = _hand("crowd")
    for t in (0, 1):
        for m, want_ap, want_ar in ((0, 0., 0.), (1, ONE, 1.), (2, ONE, 1.)):  # the top detection is a crowd match: ignored
            _eq(ap(t, 0, m), want_ap)
            _eq(ar(t, 0, m), want_ar)
        _eq(ap(t, 1, 2), ONE)
        _eq(ap(t, 2, 2), -1.)
        _eq(ap(t, 3, 2), -1.)
    assert list(r["codes"][0, 0]) == [0, 0, 1, 2] and list(r["npig"][0]) == [1, 1, 0, 0]
    assert list(r["matched"][0, 0]) == [1, 1, 0, -1]  # a crowd is matched any number of times


def test_hand_case_crowd_flag_off():
    r, ap, ar = _hand("crowd flag off")
    for t in (0, 1):
        _eq(ap(t, 0, 2), 17. / 101.)
        for m, want in ((0, 0.), (1, .5), (2, .5)):
            _eq(ar(t, 0, m), want)
        _eq(ap(t, 1, 2), 1. / 3.)
        _eq(ap(t, 3, 2), 0.)


def test_hand_case_max_dets():
    r, ap, ar = _hand("maxDets")
    for t in (0, 1):
        for m, want_ap, want_ar in ((0, 0., 0.), (1, 2. / 3., 1.), (2, 2. / 3., 1.)):
            _eq(ap(t, 0, m), want_ap)
            _eq(ar(t, 0, m), want_ar)
    assert list(r["segpos"]) == [0, 1, 2]


def test_hand_case_area():
    r, ap, ar = _hand("area")
    for t in (0, 1):
        _eq(ap(t, 0, 2), 2. / 3.)
        _eq(ap(t, 1, 2), ONE)
        _eq(ap(t, 2, 2), -1.)
        _eq(ap(t, 3, 2), ONE)


def test_hand_case_duplicates():
    r, ap, ar = _hand("duplicates")
    for t in (0, 1):
        for m, want_ap, want_ar in ((0, 51. / 101., .5), (1, ONE, 1.), (2, ONE, 1.)):
            _eq(ap(t, 0, m), want_ap)
            _eq(ar(t, 0, m), want_ar)
        assert list(r["codes"][0, t]) == [1, 1]
        assert list(r["matched"][0, t]) == [1, 0]  # the first detection takes the LAST of the equal IoUs


def test_hand_case_ignore_preference():
    r, ap, ar = _hand("ignore preference")
    # t = .5: the non-ignored object (IoU .625) wins although the ignored one overlaps more
    assert r["codes"][0, 0, 0] == 1 and r["matched"][0, 0, 0] == 0
    assert r["codes"][0, 1, 0] == 0 and r["matched"][0, 1, 0] == 1
    for m in range(3):
        _eq(ap(0, 0, m), ONE)
        _eq(ar(0, 0, m), 1.)
        _eq(ap(1, 0, m), 0.)
        _eq(ar(1, 0, m), 0.)


def test_hand_case_ignored_only():
    r, ap, ar = _hand("ignored only")
    for t in (0, 1):
        for m, want_ap, want_ar in ((0, 0., 0.), (1, ONE, 1.), (2, ONE, 1.)):
            _eq(ap(t, 0, m), want_ap)
            _eq(ar(t, 0, m), want_ar)
    assert list(r["codes"][0, 0]) == [0, 1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cross_check_against_the_reference_pinned_restatement(seed):
    d, n_img, n_cls = disjoint_case(seed)
    thr = np.arange(.5, .96, .05)
    n = d["det"].shape[0]
    margin = E.min_iou_margin(d["det"], d["det_img"], d["det_cls"], d["gt_box"], d["gt_img"], d["gt_cls"], n_img, thr)
    assert margin >= 1e-9
    for c in range(n_cls):
        s = d["det"][d["det_cls"] == c, 4]
        assert np.unique(s).size == s.size
    voc = E.voc_numpy(d["det"], d["det_img"], d["det_cls"], d["gt_box"], d["gt_img"], d["gt_cls"],
                      np.zeros(d["gt_box"].shape[0], np.uint8), n_img, n_cls, thr)
    coco = E.coco_numpy(d["det"], d["det_img"], d["det_cls"], d["gt_bbox"], d["gt_img"], d["gt_cls"], n_img, n_cls,
                        iou_thrs=thr, area_rng=[[0, 1e10]], max_dets=[1000])
    tp_share = float((voc["tpfp"][0] == 1).mean())
    print("seed %d: %d detections, %d boxes, margin %.2e, TP share at .5 = %.2f" % (seed, n, d["gt_box"].shape[0], margin, tp_share))
    assert tp_share >= 0.2
    assert np.array_equal(coco["cls_offsets"], voc["cls_offsets"])
    for c in range(n_cls):
        a, b = voc["cls_offsets"][c], voc["cls_offsets"][c + 1]
        assert np.array_equal(coco["order"][a:b], voc["order"][a:b])
    assert np.array_equal(coco["codes"][0] == 1, voc["tpfp"] == 1)
    assert not (coco["codes"] == 0).any() and not (coco["codes"] == 3).any()
    assert np.array_equal(coco["npig"][:, 0], voc["npos"])
    for c in range(n_cls):
        last = voc["cls_offsets"][c + 1] - 1
        for t in range(thr.size):
            want, got = voc["rec"][t, last], coco["recall"][t, c, 0, 0]
            assert abs(got - want) <= EPS * abs(want)


def test_summarize_equals_the_means_spelled_out():
    from coco_cases import mixed_case
    d = mixed_case(4, 3, 2, lambda c, i: 6, lambda c, i: 0 if (c, i) == (1, 0) else 3)
    r = E.coco_numpy(d["det"], d["det_img"], d["det_cls"], d["gt_bbox"], d["gt_img"], d["gt_cls"], 3, 2, d["gt_iscrowd"],
                     d["gt_area"], d["gt_ignore"])
    p, rc = r["precision"], r["recall"]
    assert p.shape == (10, 101, 2, 4, 3) and rc.shape == (10, 2, 4, 3)
    s = E.coco_summarize_numpy(p, rc)
    want = [mean_valid(p[:, :, :, 0, 2]), mean_valid(p[0, :, :, 0, 2]), mean_valid(p[5, :, :, 0, 2]),
            mean_valid(p[:, :, :, 1, 2]), mean_valid(p[:, :, :, 2, 2]), mean_valid(p[:, :, :, 3, 2]),
            mean_valid(rc[:, :, 0, 0]), mean_valid(rc[:, :, 0, 1]), mean_valid(rc[:, :, 0, 2]),
            mean_valid(rc[:, :, 1, 2]), mean_valid(rc[:, :, 2, 2]), mean_valid(rc[:, :, 3, 2])]
    assert np.array_equal(s, np.asarray(want)) and len(E.COCO_SUMMARY_NAMES) == 12
    assert E.COCO_IOU_THRS[0] == 0.5 and E.COCO_IOU_THRS[5] == 0.75 and (s[:3] > 0).all()
    # the hand case "crowd" at the default parameters: every AP that exists is 1 / (1 + eps), AR@1 = 0
    h = hand_case("crowd")
    rh = E.coco_numpy(h["det"], h["det_img"], h["det_cls"], h["gt_bbox"], h["gt_img"], h["gt_cls"], 1, 1, h["gt_iscrowd"],
                      None, h["gt_ignore"])
    sh = E.coco_summarize_numpy(rh["precision"], rh["recall"])
    assert np.abs(sh - np.asarray([ONE, ONE, ONE, ONE, -1, -1, 0, 1, 1, 1, -1, -1])).max() <= 1e-12
    with pytest.raises(ValueError, match="default parameters"):
        E.coco_summarize_numpy(p[:2], rc[:2])
    res = E.CocoEvalResult(None, None, None, None, None, None, None, None, E._coco_params([0.5], None, None, None))
    with pytest.raises(ValueError, match="default parameters"):
        res.summarize()
    assert E.COCO_IOU_THRS.size == 10 and E.COCO_REC_THRS.size == 101 and E.COCO_AREA_RNG.shape == (4, 2)
    assert len(E.COCO_THRESHOLDS) == 10  # the VOC constant is another one and stays


def test_coco_entry_points_validate_arguments_without_a_device():
    P = 0x1000  # never dereferenced: validation comes first
    names = ["det", "det_img", "det_cls", "n", "gt_bbox", "gt_img", "gt_cls", "gt_area", "gt_flags", "g", "n_img", "n_cls",
             "iou_thrs", "n_thr", "rec_thrs", "n_rec", "area_rng", "n_area", "max_dets", "n_max_dets", "order",
             "cls_offsets", "segpos", "codes", "npig", "precision", "recall", "scores", "ws", "ws_bytes", "stream"]
    ok = [P, P, P, 8, P, P, P, P, P, 4, 3, 2, P, 10, P, 101, P, 4, P, 3, P, P, P, P, P, P, P, P, P, 1 << 30, None]
    assert len(names) == len(ok) == len(_lib.lib().protos["dana_eval_coco"][1])
    assert [a for _, a in _lib.lib().protos["dana_eval_coco"][1]][:4] == names[:4]

    def coco(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return _lib.lib().call("dana_eval_coco", *a)

    for key, bads in (("n_thr", (0, 17, -1)), ("n_rec", (0, 129)), ("n_area", (0, 5)), ("n_max_dets", (0, 5))):
        for bad in bads:
            with pytest.raises(_lib.DanaError, match=key):
                coco(**{key: bad})
    for kw in (dict(n=-1), dict(g=-2), dict(n_cls=0), dict(n_img=0)):
        with pytest.raises(_lib.DanaError, match="bad shape"):
            coco(**kw)
    with pytest.raises(_lib.DanaError, match="overflows"):
        coco(n_img=1 << 20, n_cls=1 << 12)
    for name in ("iou_thrs", "rec_thrs", "area_rng", "max_dets", "cls_offsets", "npig", "precision", "recall", "scores",
                 "ws", "det", "det_img", "order", "segpos", "codes", "gt_bbox", "gt_area", "gt_flags"):
        with pytest.raises(_lib.DanaError, match="null"):
            coco(**{name: None})
    with pytest.raises(_lib.DanaError, match="workspace too small"):
        coco(ws_bytes=16)
    q = _lib.lib().query
    base = q("dana_eval_coco_workspace_bytes", 1 << 20, 1000, 500, 20, 10, 101, 4, 3)
    assert base > 0
    for bad in ((-1, 4, 3, 2, 10, 101, 4, 3), (8, 4, 3, 2, 17, 101, 4, 3), (8, 4, 3, 2, 10, 129, 4, 3),
                (8, 4, 3, 2, 10, 101, 5, 3), (8, 4, 3, 2, 10, 101, 4, 0), (8, 4, 1 << 20, 1 << 12, 10, 101, 4, 3)):
        assert q("dana_eval_coco_workspace_bytes", *bad) == 0
    assert base > q("dana_eval_coco_workspace_bytes", 1 << 20, 1000, 500, 20, 1, 101, 1, 1)


def test_coco_evaluator_refuses_the_host_and_checks_its_parameters():
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.CocoEvaluator(3, device="cpu")
    with pytest.raises(ValueError, match="1..16"):
        E.CocoEvaluator(3, iou_thrs=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match="ascend"):
        E.CocoEvaluator(3, max_dets=[10, 1])
    with pytest.raises(ValueError, match="ascend"):
        E.CocoEvaluator(3, rec_thrs=[0.5, 0.1])
    for name in ("add_packed", "add_batched", "add_by_class"):  # one implementation for both evaluators
        assert getattr(E.CocoEvaluator, name) is getattr(E.DetectionEvaluator, name)


def test_detection_evaluator_is_unchanged(golden_dir):
    sig = inspect.signature(E.DetectionEvaluator.__init__)
    assert list(sig.parameters) == ["self", "num_classes", "iou_thresholds", "use_07_metric", "device"]
    assert sig.parameters["iou_thresholds"].default == (0.5,) and sig.parameters["device"].default == "cuda"
    for name in ("reset", "add_ground_truth", "add_ground_truth_packed", "add_packed", "add_batched", "add_by_class", "compute"):
        assert callable(getattr(E.DetectionEvaluator, name))
    assert list(inspect.signature(E.DetectionEvaluator.add_ground_truth).parameters) == ["self", "image_index", "boxes",
                                                                                          "labels", "difficult"]
    with pytest.raises(RuntimeError, match="DetectionEvaluator lives on a CUDA"):
        E.DetectionEvaluator(3, device="cpu")
    with pytest.raises(ValueError, match="1..16"):
        E.DetectionEvaluator(3, iou_thresholds=np.linspace(0.1, 0.9, 17))
    g = dict(np.load(os.path.join(golden_dir, "eval_voc.npz")))
    r = E.voc_numpy(g["det"], g["det_img"], g["det_cls"], g["gt_box"], g["gt_img"], g["gt_cls"], g["gt_difficult"],
                    int(g["n_img"]), int(g["n_cls"]), g["iou_thr"], False)
    assert np.array_equal(r["order"], g["ref_order"]) and np.array_equal(r["rec"], g["ref_rec"])
    assert np.array_equal(r["prec"], g["ref_prec"])
    assert np.abs(r["ap"] - g["ref_ap_area"]).max() <= (g["det"].shape[0] + 16) * EPS
