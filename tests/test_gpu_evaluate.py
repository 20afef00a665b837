"""The device evaluator (dana_amd/evaluate.py, csrc/evaluate.hip) against the reference's answers
(tests/golden/eval_voc.npz) and against the numpy restatement `evaluate.voc_numpy`, which tests/test_evaluate_host.py
pins to the same fixture.

Bars: TP/FP flags and their cumulative counts equal as integers; rec / prec within 1 ulp (2^-52 relative: each is one
double division of exact integers); |d ap| <= (n + 16) * 2^-52 (the terms sum to at most 1 and there are at most
n + 13 rounded operations). Seeded cases assert |IoU - thr| >= 1e-9 on the host before the device runs, so a last-bit
difference in one double division cannot flip a decision."""
import os

import numpy as np
import pytest
import torch

from dana_amd import evaluate as E

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NAMES = ("det", "det_img", "det_cls", "gt_box", "gt_img", "gt_cls", "gt_difficult")


def _gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "eval_voc.npz")))


def _device(dev, d, n_img, n_cls, thr, use07=False, curves=True):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    return E.eval_ap(t(d["det"], np.float32).reshape(-1, 5), t(d["det_img"], np.int32), t(d["det_cls"], np.int32),
                     t(d["gt_box"], np.float32).reshape(-1, 4), t(d["gt_img"], np.int32), t(d["gt_cls"], np.int32),
                     t(d["gt_difficult"], np.uint8), n_img, n_cls, t(thr, np.float64), use07, curves)


def _host(d, n_img, n_cls, thr, use07=False):
    return E.voc_numpy(*[d[k] for k in NAMES], n_img, n_cls, thr, use07)


def _ulp_close(a, b):
    """equal up to 1 ulp, NaN / inf in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
            and bool((np.abs(a[fin] - b[fin]) <= EPS * np.abs(b[fin])).all()))


def _check(res, ref, n, tag=""):
    """device EvalResult (curves=True) against a dict of voc_numpy's layout"""
    offs = res.cls_offsets.cpu().numpy()
    assert np.array_equal(offs, ref["cls_offsets"]), tag
    valid = int(offs[-1])
    assert np.array_equal(res.order.cpu().numpy()[:valid], ref["order"][:valid]), tag
    assert np.array_equal(res.npos.cpu().numpy(), ref["npos"]), tag
    tpfp = res.tpfp.cpu().numpy()
    assert np.array_equal(tpfp, ref["tpfp"]), tag
    assert np.array_equal(np.cumsum(tpfp == 1, 1), np.cumsum(ref["tpfp"] == 1, 1))  # equal as integers
    assert np.array_equal(np.cumsum(tpfp == 2, 1), np.cumsum(ref["tpfp"] == 2, 1))
    assert _ulp_close(res.rec.cpu().numpy()[:, :valid], ref["rec"][:, :valid]), tag
    assert _ulp_close(res.prec.cpu().numpy()[:, :valid], ref["prec"][:, :valid]), tag
    ap = res.ap.cpu().numpy()
    assert np.array_equal(np.isnan(ap), np.isnan(ref["ap"])), tag
    err = float(np.nanmax(np.abs(ap - ref["ap"]))) if (~np.isnan(ap)).any() else 0.0
    print("%s: n = %d, max |d ap| = %.3e (bound %.3e)" % (tag, n, err, (n + 16) * EPS))
    assert err <= (n + 16) * EPS, tag


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use07", [False, True], ids=["area", "07"])
def test_fixture_through_dana_eval_ap(golden_dir, dev, use07):
    g = _gold(golden_dir)
    n, n_img, n_cls, thr = g["det"].shape[0], int(g["n_img"]), int(g["n_cls"]), g["iou_thr"]
    res = _device(dev, g, n_img, n_cls, thr, use07)
    offs = np.searchsorted(g["det_cls"][g["ref_order"]], np.arange(n_cls + 1))
    ref = dict(_host(g, n_img, n_cls, thr, use07), order=g["ref_order"], cls_offsets=offs, rec=g["ref_rec"],
               prec=g["ref_prec"], ap=g["ref_ap_07"] if use07 else g["ref_ap_area"])
    _check(res, ref, n, "fixture vs the reference")
    # all ten thresholds in one call == ten one-threshold calls, bit for bit
    for t in range(thr.size):
        one = _device(dev, g, n_img, n_cls, thr[t:t + 1], use07)
        assert torch.equal(one.tpfp[0], res.tpfp[t]) and torch.equal(one.ap[:, 0], res.ap[:, t])
        assert torch.equal(one.rec[0], res.rec[t]) and torch.equal(one.prec[0], res.prec[t])
    # without the curves: the same AP bits
    assert torch.equal(_device(dev, g, n_img, n_cls, thr, use07, curves=False).ap, res.ap)


def test_fixture_through_the_evaluator(golden_dir, dev):
    g = _gold(golden_dir)
    n, n_img, n_cls, thr = g["det"].shape[0], int(g["n_img"]), int(g["n_cls"]), g["iou_thr"]
    rng = np.random.RandomState(3)
    ev = E.DetectionEvaluator(n_cls, thr, device=dev)
    for i in rng.permutation(n_img):
        sel = g["gt_img"] == i
        if sel.any():  # host arrays and device tensors both
            boxes = g["gt_box"][sel] if i % 2 else torch.from_numpy(g["gt_box"][sel]).to(dev)
            ev.add_ground_truth(int(i), boxes, g["gt_cls"][sel], g["gt_difficult"][sel])
    groups = np.array_split(rng.permutation(n_img), 9)
    for k, imgs in enumerate(groups):
        if k % 3 == 0:  # the primitive, ids on the host
            sel = np.nonzero(np.isin(g["det_img"], imgs))[0]
            ev.add_packed(g["det"][sel], g["det_img"][sel], g["det_cls"][sel])
        elif k % 3 == 1:  # ids on the device
            sel = np.nonzero(np.isin(g["det_img"], imgs))[0]
            ev.add_packed(torch.from_numpy(g["det"][sel]).to(dev), torch.from_numpy(g["det_img"][sel]).to(dev),
                          torch.from_numpy(g["det_cls"][sel]).to(dev), num_images=n_img)
        else:  # a packed buffer with a layout, as post-processing returns it: problems (image, class), padded apart
            parts, counts, offsets, p_img, p_cls, at = [], [], [0], [], [], 0
            for i in imgs:
                for c in range(n_cls):
                    rows = g["det"][(g["det_img"] == i) & (g["det_cls"] == c)]
                    parts += [rows, np.full((2, 5), -7, np.float32)]  # two rows of padding the layout skips
                    counts.append(rows.shape[0])
                    p_img.append(i)
                    p_cls.append(c)
                    at += rows.shape[0] + 2
                    offsets.append(at)
            ev.add_batched(torch.from_numpy(np.concatenate(parts)).to(dev), np.asarray(counts, np.int32),
                           np.asarray(offsets, np.int32), p_img, p_cls)
    assert ev.num_rows == n and ev.num_images == n_img
    res = ev.compute(curves=True)
    order = res.order.cpu().numpy()
    # arrival differs from the fixture's, the ranking does not (no ties): the same rows rank by rank
    assert np.array_equal(ev._det[:n].cpu().numpy()[order], g["det"][g["ref_order"]])
    ref = dict(_host(g, n_img, n_cls, thr), rec=g["ref_rec"], prec=g["ref_prec"], ap=g["ref_ap_area"], order=order)
    _check(res, ref, n, "evaluator vs the reference")
    m = res.mean_ap().cpu().numpy()
    assert np.abs(m - g["ref_ap_area"].mean(0)).max() <= (n + 16) * EPS
    rc, pr = res.class_curves(2, 3)
    a, b = ref["cls_offsets"][2], ref["cls_offsets"][3]
    assert _ulp_close(rc.cpu().numpy(), g["ref_rec"][3, a:b]) and _ulp_close(pr.cpu().numpy(), g["ref_prec"][3, a:b])
    assert torch.equal(ev.compute().ap, res.ap)
    ev.reset()
    assert ev.num_rows == 0 and torch.isnan(ev.compute().ap).all()  # nothing added: no class has ground truth


# ---- 2. edge cases against the restatement ----------------------------------------------------------------------------------

def _case(rng, n_img, n_cls, dets_per_seg, gts_per_seg, difficult=0.2, tie_scores=False):
    """random boxes; detections are jittered copies of their segment's boxes half of the time"""
    gb, gi, gc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            for _ in range(gts_per_seg(c, i)):
                x, y = rng.randint(0, 300, 2)
                gb.append([x, y, x + rng.randint(10, 120), y + rng.randint(10, 120)])
                gi.append(i)
                gc.append(c)
    gb = np.asarray(gb, np.float32).reshape(-1, 4)
    gi, gc = np.asarray(gi, np.int32), np.asarray(gc, np.int32)
    db, di, dc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            mine = np.nonzero((gi == i) & (gc == c))[0]
            for _ in range(dets_per_seg(c, i)):
                if mine.size and rng.rand() < 0.6:
                    b = gb[mine[rng.randint(mine.size)]] + rng.uniform(-6, 6, 4)
                else:
                    x, y = rng.uniform(0, 300, 2)
                    b = np.asarray([x, y, x + rng.uniform(10, 120), y + rng.uniform(10, 120)])
                db.append(b)
                di.append(i)
                dc.append(c)
    n = len(db)
    score = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    if tie_scores:
        score = (np.floor(score * 4) / 4).astype(np.float32)  # four distinct values: ranks decided by arrival
    perm = rng.permutation(n)  # arrival order mixes classes and images
    det = np.concatenate((np.asarray(db, np.float32).reshape(-1, 4), score[:, None]), 1).astype(np.float32)[perm]
    return dict(det=det, det_img=np.asarray(di, np.int32)[perm], det_cls=np.asarray(dc, np.int32)[perm], gt_box=gb,
                gt_img=gi, gt_cls=gc, gt_difficult=(rng.rand(gb.shape[0]) < difficult).astype(np.uint8))


def _margin_ok(d, n_img, thr):
    return E.min_iou_margin(d["det"], d["det_img"], d["det_cls"], d["gt_box"], d["gt_img"], d["gt_cls"], n_img, thr) >= 1e-9


THR16 = np.linspace(0.2, 0.95, 16)


@pytest.mark.parametrize("use07", [False, True], ids=["area", "07"])
def test_edge_cases_against_the_restatement(dev, use07):
    rng = np.random.RandomState(11)
    cases = {
        # class 1 has no detections (AP 0), class 2 no ground truth (NaN, outside the mean)
        "empty classes": (_case(rng, 6, 4, lambda c, i: 0 if c == 1 else 4, lambda c, i: 0 if c == 2 else 2), 6, 4, THR16[:3]),
        "tied scores": (_case(rng, 5, 2, lambda c, i: 12, lambda c, i: 3, tie_scores=True), 5, 2, [0.5, 0.75]),
        "only difficult": (_case(rng, 4, 2, lambda c, i: 5, lambda c, i: 2, difficult=2.0), 4, 2, [0.5]),
        "200 boxes in one segment": (_case(rng, 3, 2, lambda c, i: 150 if (c, i) == (1, 2) else 3,
                                           lambda c, i: 200 if (c, i) == (1, 2) else 1), 3, 2, [0.5, 0.7, 0.9]),
        # past the LDS-held chunks of the taken bitmap (64 * 32 boxes): its words in global memory
        "2500 boxes in one segment": (_case(rng, 2, 2, lambda c, i: 300 if (c, i) == (0, 1) else 2,
                                            lambda c, i: 2500 if (c, i) == (0, 1) else 70, difficult=0.1), 2, 2, [0.3, 0.5]),
        "T = 16": (_case(rng, 8, 3, lambda c, i: 9, lambda c, i: 3), 8, 3, THR16),
    }
    for tag, (d, n_img, n_cls, thr) in cases.items():
        thr = np.asarray(thr, np.float64)
        assert _margin_ok(d, n_img, thr), tag
        n = d["det"].shape[0]
        res = _device(dev, d, n_img, n_cls, thr, use07)
        ref = _host(d, n_img, n_cls, thr, use07)
        _check(res, ref, n, tag)
        if tag == "empty classes":
            ap = res.ap.cpu().numpy()
            assert (ap[1] == 0).all() and np.isnan(ap[2]).all() and (res.npos.cpu().numpy()[2] == 0)
            m = res.mean_ap().cpu().numpy()
            assert np.abs(m - np.nanmean(ref["ap"], 0)).max() <= 1e-12 and np.isfinite(m).all()
        if tag == "only difficult":
            assert (res.npos == 0).all() and torch.isnan(res.ap).all() and not (res.tpfp == 1).any()
    # n = 1, with and without a match; rows with ids out of range take no part
    one = dict(det=[[10, 10, 50, 50, 0.9]], det_img=[0], det_cls=[0], gt_box=[[12, 11, 50, 52]], gt_img=[0], gt_cls=[0],
               gt_difficult=[0])
    _check(_device(dev, one, 1, 1, [0.5], use07), _host(one, 1, 1, [0.5], use07), 1, "n = 1, TP")
    _check(_device(dev, dict(one, gt_box=[[200, 200, 250, 250]]), 1, 1, [0.5], use07),
           _host(dict(one, gt_box=[[200, 200, 250, 250]]), 1, 1, [0.5], use07), 1, "n = 1, FP")
    none = dict(one, det=np.zeros((0, 5), np.float32), det_img=[], det_cls=[])
    _check(_device(dev, none, 1, 1, [0.5], use07), _host(none, 1, 1, [0.5], use07), 0, "n = 0")
    stray = dict(det=[[10, 10, 50, 50, 0.9], [10, 10, 50, 50, 0.8], [10, 10, 50, 50, 0.7]], det_img=[0, 5, 0],
                 det_cls=[0, 0, -1], gt_box=[[12, 11, 50, 52], [12, 11, 50, 52]], gt_img=[0, 0], gt_cls=[0, 3],
                 gt_difficult=[0, 0])
    _check(_device(dev, stray, 2, 2, [0.5], use07), _host(stray, 2, 2, [0.5], use07), 3, "ids out of range")


# ---- 3. the radix sort on its own -------------------------------------------------------------------------------------------

def test_radix_sort_is_a_stable_sort(dev):
    rng = np.random.RandomState(5)
    tile = 4096  # pairs per workgroup of a pass (csrc/evaluate.hip RS_TILE)
    sizes = [1, 2, tile - 1, tile, tile + 1, 3 * tile - 1, 3 * tile, 3 * tile + 1, 1 << 20]
    for n in sizes:
        for tag, keys, bits in (
                ("64-bit keys", rng.randint(0, 1 << 62, n, dtype=np.int64).astype(np.uint64) * np.uint64(3), 64),
                ("many duplicates", rng.randint(0, 7, n).astype(np.uint64) << np.uint64(13), 16),
                ("low 20 bits only", rng.randint(0, 1 << 40, n, dtype=np.int64).astype(np.uint64), 20)):
            vals = rng.permutation(n).astype(np.int32)
            ko, vo = E.radix_sort_pairs(torch.from_numpy(keys.view(np.int64)).to(dev), torch.from_numpy(vals).to(dev), bits)
            masked = keys & np.uint64((1 << bits) - 1) if bits < 64 else keys
            perm = np.argsort(masked, kind="stable")
            assert np.array_equal(vo.cpu().numpy(), vals[perm]), (n, tag)
            assert np.array_equal(ko.cpu().numpy().view(np.uint64), keys[perm]), (n, tag)


# ---- 4. scale ---------------------------------------------------------------------------------------------------------------

def _scale_case(seed, n_img=4096, n_cls=16, n=1 << 18, big=1 << 17):
    rng = np.random.RandomState(seed)
    n_seg = n_img * n_cls
    per = rng.randint(0, 4, n_seg)  # boxes per (class, image)
    g = int(per.sum())
    gseg = np.repeat(np.arange(n_seg), per)
    xy = rng.randint(0, 400, (g, 2))
    gt_box = np.concatenate((xy, xy + rng.randint(10, 150, (g, 2))), 1).astype(np.float32)
    gstart = np.concatenate(([0], np.cumsum(per)))
    dcls = np.concatenate((np.zeros(big, np.int64), rng.randint(1, n_cls, n - big)))
    dimg = rng.randint(0, n_img, n)
    dseg = dcls * n_img + dimg
    xy = rng.uniform(0, 400, (n, 2))
    box = np.concatenate((xy, xy + rng.uniform(10, 150, (n, 2))), 1)
    has = (per[dseg] > 0) & (rng.rand(n) < 0.6)
    pick = gstart[dseg[has]] + (rng.rand(int(has.sum())) * per[dseg[has]]).astype(np.int64)
    box[has] = gt_box[pick] + rng.uniform(-8, 8, (int(has.sum()), 4))
    score = np.zeros(n, np.float32)
    for c in range(n_cls):  # constructed: pairwise distinct within a class
        sel = np.nonzero(dcls == c)[0]
        score[sel] = ((rng.permutation(sel.size) + 1.0) / (sel.size + 1.0)).astype(np.float32)
        assert np.unique(score[sel]).size == sel.size
    perm = rng.permutation(n)
    det = np.concatenate((box, score[:, None]), 1).astype(np.float32)[perm]
    return dict(det=det, det_img=dimg.astype(np.int32)[perm], det_cls=dcls.astype(np.int32)[perm], gt_box=gt_box,
                gt_img=(gseg % n_img).astype(np.int32), gt_cls=(gseg // n_img).astype(np.int32),
                gt_difficult=(rng.rand(g) < 0.15).astype(np.uint8)), n_img, n_cls


def test_scale_against_the_restatement(dev):
    thr = np.asarray([0.5, 0.75, 0.9])
    for seed in range(40, 48):  # redraw until no IoU sits within 1e-9 of a threshold
        d, n_img, n_cls = _scale_case(seed)
        if _margin_ok(d, n_img, thr):
            break
    else:
        raise AssertionError("no seed with the 1e-9 IoU margin")
    n = d["det"].shape[0]
    segs = np.unique(d["det_cls"].astype(np.int64) * n_img + d["det_img"]).size
    assert n >= 1 << 18 and segs >= 1 << 15 and np.bincount(d["det_cls"]).max() >= 1 << 17
    res = _device(dev, d, n_img, n_cls, thr)
    _check(res, _host(d, n_img, n_cls, thr), n, "scale: %d detections, %d segments" % (n, segs))
    res07 = _device(dev, d, n_img, n_cls, thr, use07=True, curves=False)
    ref07 = np.stack([[E._ap_numpy(*[x.cpu().numpy() for x in res.class_curves(c, t)], True) for t in range(thr.size)]
                      for c in range(n_cls)])
    assert np.abs(res07.ap.cpu().numpy() - ref07).max() <= (n + 16) * EPS


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------

def test_sweep_to_average_precision_end_to_end(golden_dir, dev):
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
    plain = PP.detections_by_class(rois, cls_prob, bbox_pred, info, C, thresh=0.0)
    assert type(plain) is list and len(dets) == B  # the default return is unchanged, and the layout form equals it
    assert all(torch.equal(dets[b][c], plain[b][c]) for b in range(B) for c in range(C))
    image_indices = [5 + 2 * b for b in range(B)]
    n_img = max(image_indices) + 1
    host = [[plain[b][c].cpu().numpy() for c in range(C)] for b in range(B)]
    n = sum(h.shape[0] for row in host for h in row)
    assert n > 0
    thr = np.asarray(E.COCO_THRESHOLDS)
    for seed in range(8):  # synthetic ground truth: rounded copies of some detections, shifted ones, unrelated boxes
        rng = np.random.RandomState(seed)
        gt = []
        for b in range(B):
            boxes, labels = [], []
            for c in range(C):
                for k in rng.permutation(host[b][c].shape[0])[:3]:
                    boxes.append(np.round(host[b][c][k, :4] + rng.uniform(-3, 3, 4)))
                    labels.append(c)
                x, y = rng.randint(0, 100, 2)
                boxes.append([x, y, x + 40, y + 30])
                labels.append(c)
            gt.append((np.asarray(boxes, np.float32), np.asarray(labels, np.int32), (rng.rand(len(boxes)) < 0.2).astype(np.uint8)))
        d = dict(det=np.concatenate([h for row in host for h in row]),
                 det_img=np.concatenate([np.full(host[b][c].shape[0], image_indices[b]) for b in range(B) for c in range(C)]),
                 det_cls=np.concatenate([np.full(host[b][c].shape[0], c) for b in range(B) for c in range(C)]),
                 gt_box=np.concatenate([x[0] for x in gt]), gt_cls=np.concatenate([x[1] for x in gt]),
                 gt_img=np.concatenate([np.full(x[1].size, image_indices[b]) for b, x in enumerate(gt)]),
                 gt_difficult=np.concatenate([x[2] for x in gt]))
        if _margin_ok(d, n_img, thr):
            break
    else:
        raise AssertionError("no seed with the 1e-9 IoU margin")
    ev = E.DetectionEvaluator(C, thr, device=dev)
    for b, x in enumerate(gt):
        ev.add_ground_truth(image_indices[b], *x)
    ev.add_by_class(dets, image_indices)
    assert ev.num_rows == n
    res = ev.compute(curves=True)
    _check(res, _host(d, n_img, C, thr), n, "end to end")
    again = ev.compute(curves=True)
    for a, b_ in ((res.ap, again.ap), (res.rec, again.rec), (res.prec, again.prec), (res.tpfp, again.tpfp), (res.order, again.order)):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b_.view(torch.uint8) if b_.dtype != torch.uint8 else b_)
    # the plain nested list goes the same way
    ev2 = E.DetectionEvaluator(C, thr, device=dev)
    for b, x in enumerate(gt):
        ev2.add_ground_truth(image_indices[b], *x)
    ev2.add_by_class(plain, image_indices)
    assert torch.equal(ev2.compute().ap.view(torch.uint8), res.ap.view(torch.uint8))
    # and the drop-in entry for the reference's all_boxes[j][i]
    all_boxes = [[[] for _ in range(n_img)] for _ in range(C)]
    for b in range(B):
        for c in range(C):
            all_boxes[c][image_indices[b]] = host[b][c]
    gts = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in range(n_img)]
    for b, x in enumerate(gt):
        gts[image_indices[b]] = x
    res3 = E.evaluate_all_boxes(all_boxes, gts, thr, device=dev)
    assert torch.equal(res3.ap.view(torch.uint8), res.ap.view(torch.uint8))
