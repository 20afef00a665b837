"""The device COCO evaluator (dana_amd/evaluate.py, csrc/evaluate.hip: dana_eval_coco) against the numpy restatement
`evaluate.coco_numpy`, which tests/test_coco_eval_host.py pins to hand-worked cases and to the reference-pinned VOC
restatement.

Bars: order, cls_offsets, segpos, codes, npig equal as integers; precision / recall / scores have -1 and 0 in the same
places and are otherwise within 1 ulp (each is one double division of exact integers, or a copied score); summarize()
within (count of averaged entries + 16) * 2^-52. Every seeded case asserts on the host, before the device runs, that
|IoU - thr| >= 1e-9 for every (detection, object, threshold) and that scores are distinct within a class (the tie case
excepted), so a last-bit difference in one double division cannot flip a decision."""
import numpy as np
import pytest
import torch

from coco_cases import HAND, HAND_THRS, hand_case, mixed_case
from dana_amd import evaluate as E

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GT_KEYS = ("gt_iscrowd", "gt_area", "gt_ignore")


def _host(d, n_img, n_cls, **params):
    return E.coco_numpy(d["det"], d["det_img"], d["det_cls"], d["gt_bbox"], d["gt_img"], d["gt_cls"], n_img, n_cls,
                        d.get("gt_iscrowd"), d.get("gt_area"), d.get("gt_ignore"), **params)


def _device(dev, d, n_img, n_cls, **params):
    iou, rec, area, md = E._coco_params(params.get("iou_thrs"), params.get("rec_thrs"), params.get("area_rng"),
                                        params.get("max_dets"))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    box = np.asarray(d["gt_bbox"], np.float32).reshape(-1, 4)
    g = box.shape[0]
    crowd = np.zeros(g, np.uint8) if d.get("gt_iscrowd") is None else (np.asarray(d["gt_iscrowd"]) != 0).astype(np.uint8)
    ign = np.zeros(g, np.uint8) if d.get("gt_ignore") is None else (np.asarray(d["gt_ignore"]) != 0).astype(np.uint8)
    area_in = box[:, 2].astype(np.float64) * box[:, 3] if d.get("gt_area") is None else d["gt_area"]
    return E.eval_coco(t(d["det"], np.float32).reshape(-1, 5), t(d["det_img"], np.int32), t(d["det_cls"], np.int32),
                       t(box, np.float32), t(d["gt_img"], np.int32), t(d["gt_cls"], np.int32), t(area_in, np.float64),
                       t(crowd | (ign << 1), np.uint8), n_img, n_cls, t(iou, np.float64), t(rec, np.float64),
                       t(area, np.float64), t(md, np.int32), params=(iou, rec, area, md), codes=True)


def _same_or_ulp(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, tag
    assert np.array_equal(got == -1, want == -1) and np.array_equal(got == 0, want == 0), tag
    assert bool((np.abs(got - want) <= EPS * np.abs(want)).all()), tag


def _check(res, ref, tag=""):
    offs = res.cls_offsets.cpu().numpy()
    assert np.array_equal(offs, ref["cls_offsets"]), tag
    valid = int(offs[-1])
    assert np.array_equal(res.order.cpu().numpy()[:valid], ref["order"][:valid]), tag
    assert np.array_equal(res.segpos.cpu().numpy()[:valid], ref["segpos"][:valid]), tag
    assert (res.segpos.cpu().numpy()[valid:] == -1).all() and (ref["segpos"][valid:] == -1).all(), tag
    assert np.array_equal(res.codes.cpu().numpy(), ref["codes"]), tag
    assert np.array_equal(res.npig.cpu().numpy(), ref["npig"]), tag
    _same_or_ulp(res.precision.cpu().numpy(), ref["precision"], tag + ": precision")
    _same_or_ulp(res.recall.cpu().numpy(), ref["recall"], tag + ": recall")
    _same_or_ulp(res.scores.cpu().numpy(), ref["scores"], tag + ": scores")
    if E._coco_is_default(res.iou_thrs, res.rec_thrs, res.area_rng, res.max_dets):
        got = res.summarize().cpu().numpy()
        want = E.coco_summarize_numpy(ref["precision"], ref["recall"])
        count = ref["precision"][:, :, :, 0, 0].size
        err = float(np.abs(got - want).max())
        print("%s: summarize max |d| = %.3e (bound %.3e)" % (tag, err, (count + 16) * EPS))
        assert err <= (count + 16) * EPS, tag
        k_ap = res.per_class_ap().cpu().numpy()
        want_k = np.asarray([E._mean_valid_numpy(ref["precision"][:, :, k, 0, -1]) for k in range(k_ap.size)])
        assert np.abs(k_ap - want_k).max() <= (count + 16) * EPS, tag


def _preconditions(d, n_img, thrs, ties=False):
    ok = E.coco_min_iou_margin(d["det"], d["det_img"], d["det_cls"], d["gt_bbox"], d["gt_img"], d["gt_cls"], n_img, thrs,
                               d.get("gt_iscrowd")) >= 1e-9
    if not ties:
        for c in np.unique(d["det_cls"]):
            s = d["det"][d["det_cls"] == c, 4]
            ok = ok and np.unique(s).size == s.size
    return ok


def _seeded(make, n_img, thrs, ties=False, also=None):
    """the first of eight seeds whose case keeps every IoU 1e-9 away from every threshold (and satisfies `also`)"""
    for seed in range(8):
        d = make(seed)
        if _preconditions(d, n_img, thrs, ties) and (also is None or also(d)):
            return d
    raise AssertionError("no seed with the 1e-9 IoU margin")


# ---- 1. the hand cases through dana_eval_coco ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_through_dana_eval_coco(dev, name):
    d = hand_case(name)
    res = _device(dev, d, 1, 1, iou_thrs=HAND_THRS)
    _check(res, _host(d, 1, 1, iou_thrs=HAND_THRS), name)
    if name == "duplicates":
        assert res.codes.cpu().numpy()[0].tolist() == [[1, 1], [1, 1]]
    if name == "ignore preference":
        assert res.codes.cpu().numpy()[0, :, 0].tolist() == [1, 0]


# ---- 2. seeded cases ----------------------------------------------------------------------------------------------------------

T16 = np.linspace(0.2, 0.95, 16)


def _cases():
    few = lambda c, i: 7
    three = lambda c, i: 3
    return {
        # crowd, ignore, overlapping objects, every area range populated, segments without objects / without detections
        "mix": (lambda s: mixed_case(s, 6, 3, lambda c, i: 0 if (c, i) == (2, 1) else 9, lambda c, i: 0 if (c, i) == (0, 3) else 4),
                6, 3, {}),
        "T = 16, A = 4": (lambda s: mixed_case(10 + s, 4, 2, few, three), 4, 2, dict(iou_thrs=T16)),
        "T = A = M = 1": (lambda s: mixed_case(20 + s, 3, 2, few, three), 3, 2,
                          dict(iou_thrs=[0.5], area_rng=[[0, 1e10]], max_dets=[2], rec_thrs=[0.3])),
        "70 objects in one segment": (lambda s: mixed_case(30 + s, 2, 2, lambda c, i: 40 if (c, i) == (1, 0) else 3,
                                                           lambda c, i: 70 if (c, i) == (1, 0) else 2), 2, 2,
                                      dict(iou_thrs=[0.5, 0.7, 0.9])),
        "130 detections, max_dets 100": (lambda s: mixed_case(50 + s, 2, 2, lambda c, i: 130 if (c, i) == (0, 1) else 5,
                                                              lambda c, i: 12), 2, 2, dict(iou_thrs=[0.5, 0.75])),
        "5000 detections in one class": (lambda s: mixed_case(60 + s, 50, 2, lambda c, i: 100 if c == 0 else 2, three,
                                                              crowd=0.1), 50, 2, dict(iou_thrs=[0.5, 0.75])),
    }


@pytest.mark.parametrize("tag", sorted(_cases()))
def test_seeded_cases_against_the_restatement(dev, tag):
    make, n_img, n_cls, params = _cases()[tag]
    thrs = params.get("iou_thrs", E.COCO_IOU_THRS)
    d = _seeded(make, n_img, thrs)
    ref = _host(d, n_img, n_cls, **params)
    if tag == "mix":
        assert d["gt_iscrowd"].any() and d["gt_ignore"].any() and (ref["npig"].sum(0) > 0).all()
        assert (ref["codes"] == 0).any() and (ref["codes"] == 1).any() and (ref["codes"] == 2).any()
    if tag == "130 detections, max_dets 100":
        assert (ref["codes"] == 3).any() and ref["segpos"].max() == 129
    if tag == "5000 detections in one class":
        assert ref["cls_offsets"][1] == 5000  # more than one 2048-rank curve tile
    _check(_device(dev, d, n_img, n_cls, **params), ref, tag)


def test_overflow_tier_of_the_taken_bitmaps(dev):
    """2 100 objects in one segment: chunks past the 32nd keep their taken words in global memory"""
    thrs = [0.5, 0.75]
    make = lambda s: mixed_case(40 + s, 2, 1, lambda c, i: 60 if i == 1 else 3, lambda c, i: 2100 if i == 1 else 2,
                                crowd=0.02, ignore=0.02)
    d = _seeded(make, 2, thrs)
    ref = _host(d, 2, 1, iou_thrs=thrs, area_rng=E.COCO_AREA_RNG[:2])
    first = int(np.nonzero(d["gt_img"] == 1)[0][0])
    assert (ref["matched"] - first >= 64 * 32).any()  # a match lands in the overflow words
    _check(_device(dev, d, 2, 1, iou_thrs=thrs, area_rng=E.COCO_AREA_RNG[:2]), ref, "2100 objects")


def test_tied_scores_rank_by_image_then_arrival(dev):
    d = _seeded(lambda s: mixed_case(70 + s, 5, 2, lambda c, i: 12, lambda c, i: 3, tie_scores=True), 5, HAND_THRS, ties=True)
    ref = _host(d, 5, 2, iou_thrs=HAND_THRS)
    sc, im = d["det"][ref["order"], 4], d["det_img"][ref["order"]]
    a, b = ref["cls_offsets"][0], ref["cls_offsets"][1]
    same = sc[a + 1:b] == sc[a:b - 1]
    assert same.sum() > 20 and (im[a + 1:b][same] >= im[a:b - 1][same]).all() and (im[a + 1:b][same] > im[a:b - 1][same]).any()
    _check(_device(dev, d, 5, 2, iou_thrs=HAND_THRS), ref, "tied scores")


def test_class_without_objects_in_some_area_ranges(dev):
    def make(s):
        d = mixed_case(80 + s, 4, 3, lambda c, i: 6, lambda c, i: 0 if c == 2 else 3, crowd=0.0, ignore=0.0)
        d["gt_area"] = np.where(d["gt_cls"] == 1, 500.0, d["gt_area"])  # class 1: every annotation area is small
        return d
    d = _seeded(make, 4, E.COCO_IOU_THRS)
    ref = _host(d, 4, 3)
    assert ref["npig"][1].tolist()[1] > 0 and ref["npig"][1].tolist()[2:] == [0, 0] and (ref["npig"][2] == 0).all()
    res = _device(dev, d, 4, 3)
    _check(res, ref, "npig == 0 in some ranges")
    p = res.precision.cpu().numpy()
    assert (p[:, :, 1, 2:, :] == -1).all() and (p[:, :, 1, :2, :] > -1).all() and (p[:, :, 2] == -1).all()
    assert res.per_class_ap().cpu().numpy()[2] == -1


def test_out_of_range_ids_empty_inputs_and_repeatability(dev):
    stray = dict(det=[[10, 10, 50, 50, 0.9], [10, 10, 50, 50, 0.8], [10, 10, 50, 50, 0.7], [11, 10, 50, 50, 0.6]],
                 det_img=[0, 5, 0, 1], det_cls=[0, 0, -1, 1], gt_bbox=[[12, 11, 39, 42], [12, 11, 39, 42], [12, 11, 39, 42]],
                 gt_img=[0, 0, -1], gt_cls=[0, 3, 0])
    _check(_device(dev, stray, 2, 2, iou_thrs=[0.5]), _host(stray, 2, 2, iou_thrs=[0.5]), "ids out of range")
    none = dict(stray, det=np.zeros((0, 5), np.float32), det_img=[], det_cls=[])
    _check(_device(dev, none, 2, 2), _host(none, 2, 2), "no detections")
    nogt = dict(stray, gt_bbox=np.zeros((0, 4), np.float32), gt_img=[], gt_cls=[])
    _check(_device(dev, nogt, 2, 2), _host(nogt, 2, 2), "no objects")
    ev = E.CocoEvaluator(3, device=dev)  # nothing added
    res = ev.compute(codes=True)
    assert (res.precision == -1).all() and (res.recall == -1).all() and (res.npig == 0).all() and res.order.numel() == 0
    assert (res.summarize() == -1).all() and (res.per_class_ap() == -1).all()
    # two compute() calls give the same bits
    d = mixed_case(90, 6, 3, lambda c, i: 30, lambda c, i: 5)
    ev = E.CocoEvaluator(3, device=dev)
    for i in range(6):
        sel = d["gt_img"] == i
        ev.add_ground_truth(i, d["gt_bbox"][sel], d["gt_cls"][sel], d["gt_iscrowd"][sel], d["gt_area"][sel], d["gt_ignore"][sel])
    ev.add_packed(d["det"], d["det_img"], d["det_cls"])
    a, b = ev.compute(codes=True), ev.compute(codes=True)
    for name in ("precision", "recall", "scores", "npig", "order", "cls_offsets", "codes", "segpos"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.float64 else x,
                           y.view(torch.uint8) if y.dtype == torch.float64 else y), name
    # the packed form of the ground truth goes the same way
    ev2 = E.CocoEvaluator(3, device=dev)
    ev2.add_ground_truth_packed(d["gt_bbox"], d["gt_img"], d["gt_cls"], d["gt_iscrowd"], d["gt_area"], d["gt_ignore"])
    ev2.add_packed(torch.from_numpy(d["det"]).to(dev), torch.from_numpy(d["det_img"]).to(dev),
                   torch.from_numpy(d["det_cls"]).to(dev), num_images=6)
    assert torch.equal(ev2.compute().precision.view(torch.uint8), a.precision.view(torch.uint8))
    # and the drop-in for all_boxes[j][i]
    all_boxes = [[d["det"][(d["det_cls"] == j) & (d["det_img"] == i)] for i in range(6)] for j in range(3)]
    ann = [dict(bbox=d["gt_bbox"][d["gt_img"] == i], labels=d["gt_cls"][d["gt_img"] == i],
                iscrowd=d["gt_iscrowd"][d["gt_img"] == i], area=d["gt_area"][d["gt_img"] == i],
                ignore=d["gt_ignore"][d["gt_img"] == i]) for i in range(6)]
    res3 = E.evaluate_coco_boxes(all_boxes, ann, device=dev)
    assert torch.equal(res3.precision.view(torch.uint8), a.precision.view(torch.uint8))
    assert torch.equal(res3.summarize().view(torch.uint8), a.summarize().view(torch.uint8))


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------

def test_sweep_to_coco_numbers_end_to_end(golden_dir, dev):
    from dana_amd import postprocess as PP
    from test_gpu_support_cache import _build, _episode, _load, _sets
    g = _load(golden_dir, "eval_small_ba")
    m, _, din = _build(g["meta"], dev)
    other = _sets(_episode(dev, 2, shot=int(g["meta"][4]), seed=5)[4])
    with torch.no_grad():
        cache = m.encode_supports(torch.cat([other[:1], _sets(din[4])[:1], other[1:]], 0))
        rois, cls_prob, bbox_pred = m(*din[:4], cache.sweep())[:3]
    info = din[1]
    B, C = info.size(0), 3
    dets = PP.detections_by_class(rois, cls_prob, bbox_pred, info, C, thresh=0.0, with_layout=True)
    image_indices = [5 + 2 * b for b in range(B)]
    n_img = max(image_indices) + 1
    host = [[dets[b][c].cpu().numpy() for c in range(C)] for b in range(B)]
    n = sum(h.shape[0] for row in host for h in row)
    assert n > 0
    det = np.concatenate([h for row in host for h in row])
    det_img = np.concatenate([np.full(host[b][c].shape[0], image_indices[b]) for b in range(B) for c in range(C)])
    det_cls = np.concatenate([np.full(host[b][c].shape[0], c) for b in range(B) for c in range(C)])
    for seed in range(8):  # synthetic objects: rounded copies of some detections, one unrelated box per class, one crowd
        rng = np.random.RandomState(seed)
        gt = []
        for b in range(B):
            boxes, labels = [], []
            for c in range(C):
                for k in rng.permutation(host[b][c].shape[0])[:3]:
                    x1, y1, x2, y2 = np.round(host[b][c][k, :4] + rng.uniform(-3, 3, 4))
                    boxes.append([x1, y1, max(x2 - x1 + 1, 2), max(y2 - y1 + 1, 2)])
                    labels.append(c)
                x, y = rng.randint(0, 100, 2)
                boxes.append([x, y, 40, 30])
                labels.append(c)
            k = len(boxes)
            gt.append((np.asarray(boxes, np.float32), np.asarray(labels, np.int32), (rng.rand(k) < 0.2).astype(np.uint8),
                       None, (rng.rand(k) < 0.15).astype(np.uint8)))
        d = dict(det=det, det_img=det_img, det_cls=det_cls, gt_bbox=np.concatenate([x[0] for x in gt]),
                 gt_cls=np.concatenate([x[1] for x in gt]), gt_iscrowd=np.concatenate([x[2] for x in gt]),
                 gt_ignore=np.concatenate([x[4] for x in gt]),
                 gt_img=np.concatenate([np.full(x[1].size, image_indices[b]) for b, x in enumerate(gt)]))
        if _preconditions(d, n_img, E.COCO_IOU_THRS, ties=True):
            break
    else:
        raise AssertionError("no seed with the 1e-9 IoU margin")
    ev = E.CocoEvaluator(C, device=dev)
    for b, x in enumerate(gt):
        ev.add_ground_truth(image_indices[b], *x)
    ev.add_by_class(dets, image_indices)
    assert ev.num_rows == n and ev.num_images == n_img
    res = ev.compute(codes=True)
    # the same detections read back, in the evaluator's arrival order
    back = dict(d, det=ev._det[:n].cpu().numpy(), det_img=ev._img[:n].cpu().numpy(), det_cls=ev._cls[:n].cpu().numpy())
    _check(res, _host(back, n_img, C), "end to end")
