"""Host-side checks of the detection evaluator (dana_amd/evaluate.py): the numpy restatement of its semantics against
the reference's own answers (tests/golden/eval_voc.npz, emitted by tests/golden/make_eval_golden.py from
lib/datasets/voc_eval.py), and the argument validation of the new C entry points, which must answer before any HIP
call -- so without a device."""
import inspect
import os

import numpy as np
import pytest

from dana_amd import _lib, evaluate as E, postprocess

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "eval_voc.npz")))


def _restate(g, use07):
    return E.voc_numpy(g["det"], g["det_img"], g["det_cls"], g["gt_box"], g["gt_img"], g["gt_cls"], g["gt_difficult"],
                       int(g["n_img"]), int(g["n_cls"]), g["iou_thr"], use07)


def test_fixture_holds_what_the_tests_rely_on(gold):
    g = gold
    n_img, n_cls = int(g["n_img"]), int(g["n_cls"])
    assert g["iou_thr"].dtype == np.float64 and np.array_equal(g["iou_thr"], np.arange(0.5, 0.96, 0.05))
    assert (g["gt_difficult"] == 1).any()
    seg = g["gt_cls"].astype(np.int64) * n_img + g["gt_img"]
    assert np.bincount(seg).max() > 64  # more than one 64-lane chunk in one (class, image)
    assert np.setdiff1d(np.arange(n_img), g["gt_img"]).size > 0  # images without ground truth
    dseg = g["det_cls"].astype(np.int64) * n_img + g["det_img"]
    assert np.setdiff1d(dseg, seg).size > 0  # detections where their class has no ground truth
    both = np.concatenate((seg[:, None].astype(np.float64), g["gt_box"].astype(np.float64)), 1)
    assert np.unique(both, axis=0).shape[0] < both.shape[0]  # duplicated boxes: an argmax tie
    for c in range(n_cls):
        s = g["det"][g["det_cls"] == c, 4]
        assert np.unique(s).size == s.size  # the reference's argsort is not stable
        assert ((g["gt_cls"] == c) & (g["gt_difficult"] == 0)).any()
    assert E.min_iou_margin(g["det"], g["det_img"], g["det_cls"], g["gt_box"], g["gt_img"], g["gt_cls"], n_img,
                            g["iou_thr"]) >= 1e-9


@pytest.mark.parametrize("use07", [False, True])
def test_restatement_equals_the_reference(gold, use07):
    g = gold
    r = _restate(g, use07)
    n = g["det"].shape[0]
    assert np.array_equal(r["order"], g["ref_order"])
    assert np.array_equal(r["rec"], g["ref_rec"])  # bit-equal
    assert np.array_equal(r["prec"], g["ref_prec"])
    ref_ap = g["ref_ap_07"] if use07 else g["ref_ap_area"]
    err = np.abs(r["ap"] - ref_ap).max()
    print("restatement vs reference, use_07_metric=%s: max |d ap| = %.3e (bound %.3e)" % (use07, err, (n + 16) * EPS))
    assert err <= (n + 16) * EPS
    assert (r["npos"] > 0).all()


def test_restatement_defined_deviations():
    # npos == 0 -> NaN under both metrics; tied scores rank in arrival order; a class without detections has AP 0
    det = np.asarray([[0, 0, 10, 10, 0.5], [0, 0, 10, 10, 0.5], [50, 50, 60, 60, 0.5]], np.float32)
    gt = np.asarray([[0, 0, 10, 10], [0, 0, 9, 9]], np.float32)
    for use07 in (False, True):
        r = E.voc_numpy(det, [0, 0, 0], [0, 0, 0], gt, [0, 0], [0, 2], [0, 0], 1, 3, [0.5], use07)
        assert list(r["order"]) == [0, 1, 2] and list(r["tpfp"][0]) == [1, 2, 2]
        assert abs(r["ap"][0, 0] - 1.0) < 1e-12 and np.isnan(r["ap"][1, 0]) and r["ap"][2, 0] == 0.0
        assert list(r["npos"]) == [1, 0, 1]


def _call(name, *args):
    return _lib.lib().call(name, *args)


def test_eval_entry_points_validate_arguments_without_a_device():
    P = 0x1000  # never dereferenced: validation comes first
    ok_ap = [P, P, P, 8, P, P, P, P, 4, 3, 2, P, 1, 0, P, P, P, None, None, P, P, P, 1 << 30, None]

    def ap(**kw):
        names = ["det", "det_img", "det_cls", "n", "gt_box", "gt_img", "gt_cls", "gt_difficult", "g", "n_img", "n_cls",
                 "iou_thr", "n_thr", "use07", "order", "cls_offsets", "tpfp", "rec", "prec", "ap", "npos", "ws", "ws_bytes",
                 "stream"]
        a = list(ok_ap)
        for k, v in kw.items():
            a[names.index(k)] = v
        return _call("dana_eval_ap", *a)

    for bad in (0, 17, -1):
        with pytest.raises(_lib.DanaError, match="n_thr"):
            ap(n_thr=bad)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        ap(n=-1)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        ap(g=-2)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        ap(n_cls=0)
    with pytest.raises(_lib.DanaError, match="overflows"):
        ap(n_img=1 << 20, n_cls=1 << 12)
    for name in ("iou_thr", "cls_offsets", "ap", "npos", "ws", "det", "det_cls", "order", "tpfp", "gt_box", "gt_difficult"):
        with pytest.raises(_lib.DanaError, match="null"):
            ap(**{name: None})
    with pytest.raises(_lib.DanaError, match="together"):
        ap(rec=P)
    with pytest.raises(_lib.DanaError, match="workspace too small"):
        ap(ws_bytes=16)
    q = _lib.lib().query
    assert q("dana_eval_ap_workspace_bytes", 8, 4, 3, 2, 1) > 0
    assert q("dana_eval_ap_workspace_bytes", 8, 4, 3, 2, 17) == 0
    assert q("dana_eval_ap_workspace_bytes", -1, 4, 3, 2, 1) == 0
    assert q("dana_eval_ap_workspace_bytes", 8, 4, 1 << 20, 1 << 12, 1) == 0
    # more thresholds or more rows never need less
    assert q("dana_eval_ap_workspace_bytes", 1 << 20, 1000, 500, 20, 10) > q("dana_eval_ap_workspace_bytes", 1 << 20, 1000, 500, 20, 1)

    ok_app = [P, P, P, P, P, 2, 10, P, P, P, 0, 16, None]
    with pytest.raises(_lib.DanaError, match="bad shape"):
        _call("dana_eval_append", *(ok_app[:5] + [-1] + ok_app[6:]))
    with pytest.raises(_lib.DanaError, match="bad shape"):
        _call("dana_eval_append", *(ok_app[:6] + [-1] + ok_app[7:]))
    with pytest.raises(_lib.DanaError, match="capacity"):
        _call("dana_eval_append", *(ok_app[:10] + [8] + ok_app[11:]))
    with pytest.raises(_lib.DanaError, match="null"):
        _call("dana_eval_append", *([None] + ok_app[1:]))
    with pytest.raises(_lib.DanaError, match="bad shape"):
        _call("dana_debug_radix_sort_pairs", P, P, P, P, 4, 65, P, 1 << 20, None)
    with pytest.raises(_lib.DanaError, match="null"):
        _call("dana_debug_radix_sort_pairs", P, None, P, P, 4, 64, P, 1 << 20, None)
    with pytest.raises(_lib.DanaError, match="workspace too small"):
        _call("dana_debug_radix_sort_pairs", P, P, P, P, 4, 64, P, 8, None)


def test_evaluator_refuses_the_host_and_reads_nothing_back():
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.DetectionEvaluator(3, device="cpu")
    with pytest.raises(ValueError, match="1..16"):
        E.DetectionEvaluator(3, iou_thresholds=np.linspace(0.1, 0.9, 17))
    assert len(E.COCO_THRESHOLDS) == 10 and E.COCO_THRESHOLDS[0] == 0.5


def test_detections_by_class_default_return_is_unchanged():
    sig = inspect.signature(postprocess.detections_by_class)
    assert sig.parameters["with_layout"].default is False
    assert list(sig.parameters)[:7] == ["rois", "cls_prob", "bbox_pred", "im_info", "num_classes", "thresh", "nms_inclusive"]
    # the layout-carrying result IS the nested list (same indexing, equality and length)
    cd = postprocess.ClassDetections([[1, 2], [3, 4]])
    assert cd == [[1, 2], [3, 4]] and isinstance(cd, list) and cd[1][0] == 3
