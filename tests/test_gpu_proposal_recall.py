"""The device proposal recall (dana_amd/evaluate.py `ProposalRecallEvaluator`, csrc/recall.hip: dana_eval_proposal_recall)
against the numpy restatement `proposal_recall_numpy` (itself pinned by tests/test_proposal_recall_host.py).

Bars: ov bit for bit (each is a fixed sequence of IEEE double operations on the same inputs); match, hits and npos as
integers; recalls and the per-class tables within 1 ulp with NaN in the same places (one division of exact integers); ar
within (T + 2) * 2^-52 relative (a mean of T such ratios)."""
import numpy as np
import pytest
import torch

import recall_cases as RC
from dana_amd import evaluate as E

pytestmark = pytest.mark.gpu

HAND = RC.hand_cases()
SEEDED = {
    "geometry": RC.geometry_case,                                    # every list length x object count of the launch geometry
    "one_of_each": lambda: RC.geometry_case(iou_thrs=(0.5,), limits=(0,), area_rng=["all"]),  # T = L = A = 1
    "full_parameters": RC.full_parameter_case,                       # T = 16, L = 8, A = 8
    "contested": RC.contested_case,                                  # the re-scan path
    "rpn_sized": RC.rpn_sized_case,                                  # 2000 rows in one list
    "three_classes": RC.three_class_case,                            # others=True, an image of one class
    "quantised": lambda: RC.seeded_case(21, [(40, 12), (7, 9), (3, 5)], n_cls=2, quantum=8., extent=120., others=True,
                                        limits=(0, 5), iou_thrs=(0.25, 0.5, 0.75)),  # exact ties
}
_REF = {}


def _reference(name):
    """(args, numpy result) of a case, computed once"""
    if name not in _REF:
        args = (HAND[name] if name in HAND else SEEDED[name]())["args"]
        _REF[name] = (args, E.proposal_recall_numpy(**args))
    return _REF[name]


def _evaluator(dev, a, per_image=False):
    ev = E.ProposalRecallEvaluator(a["n_cls"], dev, iou_thresholds=a["iou_thrs"], limits=a["limits"],
                                   area_ranges=a["area_rng"], others=a["others"])
    if per_image:  # (the seeded cases list their objects image by image, so the rows arrive in the same order)
        for im in np.unique(a["gt_img"]):
            sel = a["gt_img"] == im
            ev.add_ground_truth(int(im), a["gt_box"][sel], a["gt_cls"][sel], None if a["gt_area"] is None else a["gt_area"][sel])
    else:
        ev.add_ground_truth_packed(torch.from_numpy(a["gt_box"]).to(dev), a["gt_img"], a["gt_cls"], a["gt_area"])
    ev.add_proposals(torch.from_numpy(a["boxes"]).to(dev), a["counts"], a["offsets"], a["prob_img"], a["prob_cls"])
    return ev


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _within_ulp(got, want, rel=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bound = np.spacing(np.abs(want[ok])) if rel is None else rel * np.abs(want[ok])
    assert (np.abs(got[ok] - want[ok]) <= bound).all(), float(np.abs(got[ok] - want[ok]).max())


def _check(res, ref):
    ov, match = res.ov.cpu().numpy(), res.match.cpu().numpy()
    assert ov.shape == ref["ov"].shape and match.shape == ref["match"].shape
    assert np.array_equal(_bits(ov), _bits(ref["ov"])), "ov differs in %d places" % (_bits(ov) != _bits(ref["ov"])).sum()
    assert np.array_equal(match, ref["match"])
    hits, npos = res.hits.cpu().numpy(), res.npos.cpu().numpy()
    assert hits.dtype == np.int64 and npos.dtype == np.int64
    assert np.array_equal(hits, ref["hits"]) and np.array_equal(npos, ref["npos"])
    assert np.array_equal(res.pair_gt, ref["pair_gt"]) and np.array_equal(res.unit_tab, ref["unit_tab"])
    T = ref["hits"].shape[1]
    _within_ulp(res.recalls.cpu().numpy(), ref["recalls"])
    _within_ulp(res.ar.cpu().numpy(), ref["ar"], rel=(T + 2) * 2. ** -52)
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = ref["hits"] / ref["npos"][:, None, None, :, :].astype(np.float64)
    _within_ulp(res.per_class_recalls.cpu().numpy(), pc)
    _within_ulp(res.per_class_ar.cpu().numpy(), pc.mean(1), rel=(T + 2) * 2. ** -52)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_through_the_device(dev, name):
    a, ref = _reference(name)
    res = _evaluator(dev, a).compute()
    _check(res, ref)
    e = HAND[name]["expect"]  # and the written-out answers themselves
    assert np.array_equal(res.ov.cpu().numpy(), np.asarray(e["ov"], np.float64))
    assert np.array_equal(res.match.cpu().numpy(), np.asarray(e["match"]))
    assert np.array_equal(res.hits.cpu().numpy(), RC.dense(e["hits"], tuple(res.hits.shape)))


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_seeded_cases_equal_the_numpy_restatement(dev, name):
    a, ref = _reference(name)
    res = _evaluator(dev, a, per_image=name in ("geometry", "three_classes")).compute()
    _check(res, ref)
    assert ref["n_pairs"] > 0 and (ref["ov"] > 0).any()
    if name == "geometry":
        m, n = ref["unit_tab"][:, 1], ref["unit_tab"][:, 3] - ref["unit_tab"][:, 2]
        assert sorted(set(m.tolist())) == [0, 1, 40, 63, 64, 65, 255, 256, 257, 300]
        assert sorted(set(n.tolist())) == [1, 2, 3, 64, 65, 130, 300] and (m < n).any()
    if name == "full_parameters":
        assert ref["hits"].shape[1:4] == (16, 8, 8) and (ref["npos"][1] > 0).any()
    if name == "one_of_each":
        assert ref["hits"].shape[1:4] == (1, 1, 1)
    if name == "three_classes":  # image 1: every object is of class 0, so the other unit of its class-0 list is empty
        u = ref["unit_tab"]
        other = u[(u[:, 8] == 1) & (u[:, 7] == 0)]
        assert ((other[:, 3] - other[:, 2]) + (other[:, 5] - other[:, 4]) == 0).any()


def test_views_limits_and_selectivity(dev):
    a, ref = _reference("three_classes")
    res = _evaluator(dev, a).compute()
    assert torch.equal(res.gt_overlaps(10), res.ov[1, 0]) and torch.equal(res.matched_rows(0, "all"), res.match[0, 0])
    assert res.gt_overlaps(0).data_ptr() == res.ov.data_ptr()  # views, not copies
    with pytest.raises(ValueError, match="not one of"):
        res.gt_overlaps(7)
    with pytest.raises(ValueError, match="not one of"):
        res.gt_overlaps(0, "small")
    _within_ulp(res.selectivity().cpu().numpy(), ref["ar"][0] / ref["ar"][1], rel=(2 * (3 + 2) + 1) * 2. ** -52)  # two ar's and a division
    pooled = E.ProposalRecallResult.from_counts(res.hits * 2, res.npos * 2, res.params)
    assert torch.equal(pooled.recalls, res.recalls)


def test_two_calls_give_the_same_bytes(dev):
    a, _ = _reference("contested")
    b, _ = _reference("geometry")
    for args in (a, b):
        ev = _evaluator(dev, args)
        r1 = ev.compute()
        r2 = ev.compute()
        assert r1.ov.data_ptr() != r2.ov.data_ptr()
        for x, y in ((r1.ov, r2.ov), (r1.match, r2.match), (r1.hits, r2.hits), (r1.npos, r2.npos)):
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_bookkeeping_on_the_device(dev):
    a, ref = _reference("three_classes")
    ev = _evaluator(dev, a)
    t = ev.tables()
    for k in ("unit_tab", "gt_order", "pair_unit", "pair_gt"):
        assert np.array_equal(t[k], ref[k]), k
    # ids on the device are refused: nothing is read back
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    box = torch.zeros((1, 4), device=dev)
    rows = ev.num_rows
    with pytest.raises(ValueError, match="host integers"):
        ev.add_proposals(box, [1], None, ids, 0)
    with pytest.raises(ValueError, match="host integers"):
        ev.add_proposals(box, [1], None, 0, ids)
    with pytest.raises(ValueError, match="host integers"):
        ev.add_proposals(box, ids + 1, None, 0, 0)
    with pytest.raises(ValueError, match="host integers"):
        ev.add_ground_truth(0, box, ids)
    with pytest.raises(ValueError, match="host integers"):
        ev.add_ground_truth_packed(box, ids, [0])
    assert ev.num_rows == rows and np.array_equal(ev.tables()["unit_tab"], ref["unit_tab"])
    # lists that do not follow each other in the packed buffer are gathered; the growing buffer keeps what it had
    src = torch.arange(40, dtype=torch.float32, device=dev).view(10, 4)
    ev.add_proposals(src, [2, 0, 3], [7, 0, 1], [5, 5, 6], [0, 1, 2])
    stored, p_img, p_cls, cnt, off = ev.proposals()
    assert torch.equal(stored[rows:], src[[7, 8, 1, 2, 3]]) and torch.equal(stored[:rows].cpu(), torch.from_numpy(a["boxes"]))
    assert p_img[-3:].tolist() == [5, 5, 6] and cnt[-3:].tolist() == [2, 0, 3] and off[-3:].tolist() == [rows, rows + 2, rows + 2]
    ev.add_proposals(torch.ones((1500, 4), device=dev), [1500], None, 8, 0)  # past the first capacity: the buffer grows
    assert torch.equal(ev.proposals()[0][rows:rows + 5], src[[7, 8, 1, 2, 3]]) and ev.num_rows == rows + 1505
    # an evaluator nothing was added to: zero counts, NaN ratios, no launch
    empty = E.ProposalRecallEvaluator(2, dev, limits=(0,), area_ranges=["all"]).compute()
    assert int(empty.hits.abs().sum()) == 0 and int(empty.npos.sum()) == 0 and torch.isnan(empty.ar).all()
    assert empty.ov.shape == (1, 1, 0)


def test_add_rois_of_a_class_sweep(dev):
    """the model level: the rois of an eval-mode sweep forward, divided by the image scale on the device"""
    from test_gpu_support_cache import _episode, _model, _sets
    classes = [2, 0, 1]
    m = _model(dev)[0]
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        sweep = cache.sweep(classes)
        rois = m(im, info, gt, nb, sweep)[0].clone()
    B, C, R = 2, len(classes), rois.size(1)
    assert rois.shape == (B * C, R, 5)
    info = info.clone()
    info[:, 2] = torch.tensor([1.6, 0.7], device=dev)  # the scales of two resized images
    scale = info[:, 2].cpu().numpy()
    img_ids = [4, 9]
    ev = E.ProposalRecallEvaluator(3, dev, limits=(10, 100, 0), area_ranges=["all", "small", "medium", "large"], others=True)
    ev.add_rois(rois, info, img_ids, sweep.classes)
    stored, p_img, p_cls, cnt, off = ev.proposals()
    assert p_img.tolist() == [4, 4, 4, 9, 9, 9] and p_cls.tolist() == classes * 2 and cnt.tolist() == [R] * 6
    want = rois.cpu().numpy()[:, :, 1:5] / np.repeat(scale, C).astype(np.float32)[:, None, None]
    got = stored.cpu().numpy().reshape(B * C, R, 4)
    assert want.dtype == np.float32 and (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    # ground truth: the episode's boxes in original-image pixels, classes by position
    g_box, g_img, g_cls = [], [], []
    for b in range(B):
        k = int(nb[b])
        g_box.append(gt[b, :k, :4].cpu().numpy() / np.float32(scale[b]))
        g_img += [img_ids[b]] * k
        g_cls += [(b + j) % 3 for j in range(k)]
        ev.add_ground_truth(img_ids[b], g_box[-1], g_cls[-k:] if k else [])
    g_box = np.concatenate(g_box, 0)
    assert g_box.shape[0] > 0
    res = ev.compute()
    ref = E.proposal_recall_numpy(got.reshape(-1, 4), p_img, p_cls, cnt, off, g_box, g_img, g_cls, 3, limits=(10, 100, 0),
                                  area_rng=["all", "small", "medium", "large"], others=True)
    _check(res, ref)
    assert ref["n_pairs"] == C * g_box.shape[0]  # every object: one target unit and C - 1 other units of its image
    # counts: a caller that knows the real lengths keeps the padding out
    ev2 = E.ProposalRecallEvaluator(3, dev, limits=(0,), area_ranges=["all"])
    keep = [R, R - 10, 5, 0, 1, R]
    ev2.add_rois(rois, info, img_ids, sweep.classes, counts=keep)
    s2, _, _, c2, o2 = ev2.proposals()
    assert c2.tolist() == keep and ev2.num_rows == sum(keep)
    for p in range(B * C):
        assert torch.equal(s2[o2[p]:o2[p] + c2[p]], stored.view(B * C, R, 4)[p, :keep[p]])
    with pytest.raises(ValueError, match="problems"):
        ev2.add_rois(rois, info, [1, 2, 3], sweep.classes)
