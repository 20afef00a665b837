"""The device error diagnosis (dana_amd/diagnose.py `diagnose_errors`, `DetectionDiagnoser`; csrc/diagnose.hip) against the
numpy restatement `diagnose.tide_numpy`, which tests/test_diagnose_host.py pins to the hand-worked cases and to a brute force.

Bars: order, cls_offsets, tpfp, npos, det_type, det_ref, gt_state, counts and confusion equal as integers; the baseline AP
bit-equal to `DetectionEvaluator`'s at the same threshold; ap_fixed within 1 ulp of the restatement's (`_ulp_close` of
tests/test_gpu_evaluate.py), NaN in the same places -- both sides round the exact sum of the same terms once, so the
bound does not depend on how many terms a class has. Every seeded input keeps |IoU - t| >= 1e-9 for both thresholds
(`find_case` fails when no seed does), so a last-bit difference in one double division cannot flip a type.

Sizes are the smallest at which the launch geometry changes path: 0 / 1 / 63 / 64 / 65 / 130 objects in an image (the
64-object chunks of type_kernel), 1 / 64 / 65 / 130 detections in a (class, image) segment (its 64-detection chunks), a
number of segments that is no multiple of the 4 a workgroup takes, more than 4096 rows (two tiles of the radix sort) and a
class of more than 2048 ranks (two tiles of the curve kernel)."""
import numpy as np
import pytest
import torch

import diagnose_cases as DC
from dana_amd import diagnose as D, evaluate as E
from test_gpu_evaluate import _ulp_close

pytestmark = pytest.mark.gpu

HAND = DC.hand_cases()
OBJS = [0, 1, 63, 64, 65, 130]
DETS = [1, 64, 65, 130]

SEEDED = {
    # every object count x every segment length, 5 classes: 30 segments
    "geometry_5_classes": lambda s: DC.random_case(s, 6, 5, lambda i: OBJS[i], lambda c, i: DETS[(c + i) % 4]),
    "geometry_1_class": lambda s: DC.random_case(s, 6, 1, lambda i: OBJS[i], lambda c, i: DETS[i % 4]),
    "tied_scores": lambda s: DC.random_case(s, 6, 5, lambda i: OBJS[i], lambda c, i: DETS[(c + 2 * i) % 4], tie_scores=True),
    "stray_ids": lambda s: DC.random_case(s, 5, 3, lambda i: 6, lambda c, i: 9, stray=7),
    "all_difficult": lambda s: DC.random_case(s, 3, 2, lambda i: 4, lambda c, i: 6, difficult=2.0),
    # 30 x 130 = 3900 ranks in class 0 (two curve tiles), 5100 rows (two sort tiles)
    "two_tiles": lambda s: DC.random_case(s, 30, 3, lambda i: 5, lambda c, i: 130 if c == 0 else 20),
    "contested": lambda s: DC.contested_case(s),
}


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)


def _tensors(case, dev):
    return (_t(case["det"], np.float32, dev).reshape(-1, 5), _t(case["det_img"], np.int32, dev), _t(case["det_cls"], np.int32, dev),
            _t(case["gt_box"], np.float32, dev).reshape(-1, 4), _t(case["gt_img"], np.int32, dev), _t(case["gt_cls"], np.int32, dev),
            _t(case["gt_difficult"], np.uint8, dev))


def _device(case, dev, t_f=0.5, t_b=0.1, use07=False):
    return D.diagnose_errors(*_tensors(case, dev), case["n_img"], case["n_cls"], _t([t_f, t_b], np.float64, dev), use07)


def _bits(x):
    return x.contiguous().view(torch.uint8) if x.dtype != torch.uint8 else x


def _check(res, ref, tag, evaluator_ap=None):
    offs = res.cls_offsets.cpu().numpy()
    assert np.array_equal(offs, ref["cls_offsets"]), tag
    valid = int(offs[-1])
    assert np.array_equal(res.order.cpu().numpy()[:valid], ref["order"][:valid]), tag
    for k in ("tpfp", "npos", "det_type", "det_ref", "gt_state", "counts", "confusion"):
        got = getattr(res, k).cpu().numpy()
        assert got.shape == ref[k].shape and np.array_equal(got, ref[k]), (tag, k)
    if evaluator_ap is not None:
        assert torch.equal(_bits(res.ap), _bits(evaluator_ap)), tag
    ap = res.ap.cpu().numpy()  # against the restatement: the bound of tests/test_gpu_evaluate.py
    assert np.array_equal(np.isnan(ap), np.isnan(ref["ap"])), tag
    assert not np.isfinite(ap).any() or np.nanmax(np.abs(ap - ref["ap"])) <= (ap.size + ref["det_type"].size + 16) * 2.0 ** -52, tag
    got = res.ap_fixed.cpu().numpy()
    fin = np.isfinite(ref["ap_fixed"]) & np.isfinite(got) & (ref["ap_fixed"] != 0)
    worst = float((np.abs(got - ref["ap_fixed"])[fin] / np.abs(ref["ap_fixed"][fin])).max() / 2.0 ** -52) if fin.any() else 0.
    print("%s: n = %d, types %s, ap_fixed off by at most %.2f x 2^-52 relative" % (
        tag, ref["det_type"].size, np.bincount(ref["det_type"], minlength=7).tolist(), worst))
    assert _ulp_close(got, ref["ap_fixed"]), (tag, worst)
    assert _ulp_close(res.delta_ap().cpu().numpy(), got - res.ap.cpu().numpy()[None, :]), tag


def _evaluator_ap(case, dev, t_f, use07):
    return E.eval_ap(*_tensors(case, dev), case["n_img"], case["n_cls"], _t([t_f], np.float64, dev), use07).ap[:, 0]


@pytest.mark.parametrize("use07", [False, True], ids=["area", "07"])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(dev, name, use07):
    case = HAND[name]["args"]
    res = _device(case, dev, use07=use07)
    _check(res, DC.host(case, use_07_metric=use07), name, _evaluator_ap(case, dev, 0.5, use07))
    if not use07:  # and the written-out answers themselves
        e = HAND[name]["expect"]
        assert res.det_type.cpu().tolist() == e["det_type"] and res.det_ref.cpu().tolist() == e["det_ref"]
        assert res.gt_state.cpu().tolist() == e["gt_state"] and res.counts.cpu().tolist() == e["counts"]
        assert res.confusion.cpu().tolist() == e["confusion"]
        for o, k in enumerate(D.ORACLE_NAMES):
            assert _ulp_close(res.ap_fixed[o].cpu().numpy(), np.asarray(e["ap_fixed"][k], np.float64)), k


@pytest.mark.parametrize("use07", [False, True], ids=["area", "07"])
@pytest.mark.parametrize("name", sorted(SEEDED))
def test_seeded_cases(dev, name, use07):
    case = DC.find_case(SEEDED[name], 500)
    res = _device(case, dev, use07=use07)
    ref = DC.host(case, use_07_metric=use07)
    _check(res, ref, name, _evaluator_ap(case, dev, 0.5, use07))
    if name == "contested":  # many Cls detections of several classes on one object; rows moved into an empty class
        C = case["n_cls"]
        assert ref["counts"][:, 1].sum() >= 100 and (ref["confusion"][0, 1:C] > 0).sum() >= 3
        assert ref["cls_offsets"][C] == ref["cls_offsets"][C - 1] and ref["ap"][C - 1] == 0.
        assert abs(res.ap_fixed[0, C - 1].item() - 1.0) <= 1e-12
    if name == "geometry_5_classes":
        assert (np.bincount(ref["det_type"], minlength=7)[1:] > 0).all()  # every type occurs


def test_other_thresholds(dev):
    make = SEEDED["geometry_5_classes"]
    for t_f, t_b in ((0.75, 0.3), (0.3, 0.05)):  # (t_b = 0 cannot keep the margin: disjoint boxes have IoU 0 exactly)
        case = DC.find_case(make, 600, t_f, t_b)
        _check(_device(case, dev, t_f, t_b), DC.host(case, t_f, t_b), "t_f=%g t_b=%g" % (t_f, t_b),
               _evaluator_ap(case, dev, t_f, False))


def test_empty_sides(dev):
    case = DC.find_case(SEEDED["stray_ids"], 700)
    none = dict(case, det=np.zeros((0, 5), np.float32), det_img=np.zeros(0, np.int32), det_cls=np.zeros(0, np.int32))
    res = _device(none, dev)
    _check(res, DC.host(none), "n = 0")
    assert (res.counts[:, :6] == 0).all() and res.counts[:, 6].sum().item() == int((DC.host(none)["gt_state"] == 3).sum()) > 0
    bare = dict(case, gt_box=np.zeros((0, 4), np.float32), gt_img=np.zeros(0, np.int32), gt_cls=np.zeros(0, np.int32),
                gt_difficult=np.zeros(0, np.uint8))
    res = _device(bare, dev)
    _check(res, DC.host(bare), "g = 0")
    assert torch.isnan(res.ap_fixed).all() and (res.det_type[res.det_type != 0] == DC.BKG).all()
    both = dict(none, gt_box=bare["gt_box"], gt_img=bare["gt_img"], gt_cls=bare["gt_cls"], gt_difficult=bare["gt_difficult"])
    _check(_device(both, dev), DC.host(both), "n = 0 and g = 0")


def test_two_calls_give_the_same_bits(dev):
    case = DC.find_case(SEEDED["tied_scores"], 800)
    a, b = _device(case, dev), _device(case, dev)
    for k in ("ap", "ap_fixed", "order", "cls_offsets", "tpfp", "npos", "det_type", "det_ref", "gt_state", "counts", "confusion"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k


def test_sweep_to_diagnosis_end_to_end(golden_dir, dev):
    """the accumulating API on the lists of a small class sweep, built as test_sweep_to_average_precision_end_to_end does"""
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
    host = [[dets[b][c].cpu().numpy() for c in range(C)] for b in range(B)]
    image_indices = [5 + 2 * b for b in range(B)]
    n_img = max(image_indices) + 1
    n = sum(h.shape[0] for row in host for h in row)
    assert n > 0
    for seed in range(8):  # synthetic ground truth: rounded copies of some detections under ANY class, and unrelated boxes
        rng = np.random.RandomState(seed)
        gt = []
        for b in range(B):
            boxes, labels = [], []
            for c in range(C):
                for k in rng.permutation(host[b][c].shape[0])[:3]:
                    boxes.append(np.round(host[b][c][k, :4] + rng.uniform(-3, 3, 4)))
                    labels.append(rng.randint(C))
                x, y = rng.randint(0, 100, 2)
                boxes.append([x, y, x + 40, y + 30])
                labels.append(c)
            gt.append((np.asarray(boxes, np.float32), np.asarray(labels, np.int32), (rng.rand(len(boxes)) < 0.2).astype(np.uint8)))
        case = dict(det=np.concatenate([h for row in host for h in row]),
                    det_img=np.concatenate([np.full(host[b][c].shape[0], image_indices[b]) for b in range(B) for c in range(C)]),
                    det_cls=np.concatenate([np.full(host[b][c].shape[0], c) for b in range(B) for c in range(C)]),
                    gt_box=np.concatenate([x[0] for x in gt]), gt_cls=np.concatenate([x[1] for x in gt]),
                    gt_img=np.concatenate([np.full(x[1].size, image_indices[b]) for b, x in enumerate(gt)]),
                    gt_difficult=np.concatenate([x[2] for x in gt]), n_img=n_img, n_cls=C)
        if DC.margin(case) >= 1e-9:
            break
    else:
        raise AssertionError("no seed with the 1e-9 IoU margin")
    dg = D.DetectionDiagnoser(C, device=dev)
    ev = E.DetectionEvaluator(C, (0.5,), device=dev)
    for b, x in enumerate(gt):
        dg.add_ground_truth(image_indices[b], *x)
        ev.add_ground_truth(image_indices[b], *x)
    dg.add_by_class(dets, image_indices)
    ev.add_by_class(dets, image_indices)
    assert dg.num_rows == n
    res = dg.compute()
    ref = DC.host(case)
    _check(res, ref, "end to end", ev.compute().ap[:, 0])
    assert torch.equal(_bits(res.mean_ap().reshape(1)), _bits(ev.compute().mean_ap()))
    s = res.summary()
    assert s["count"] == {k: int(ref["counts"][:, j].sum()) for j, k in enumerate(D.TYPE_NAMES)}
    assert abs(s["mean_ap"] - ref["mean_ap"]) <= 1e-12
    for o, k in enumerate(D.ORACLE_NAMES):
        assert _ulp_close(np.asarray(s["delta_ap"][k]), res.delta_ap()[o].cpu().numpy())
        d = ref["delta_map"][o]
        assert (np.isnan(d) and np.isnan(s["delta_map"][k])) or abs(s["delta_map"][k] - d) <= 1e-12, k
    # the drop-in entry for the reference's all_boxes[j][i] gives the same diagnosis
    all_boxes = [[[] for _ in range(n_img)] for _ in range(C)]
    for b in range(B):
        for c in range(C):
            all_boxes[c][image_indices[b]] = host[b][c]
    gts = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for _ in range(n_img)]
    for b, x in enumerate(gt):
        gts[image_indices[b]] = x
    res2 = D.diagnose_all_boxes(all_boxes, gts, device=dev)
    assert torch.equal(res2.counts, res.counts) and torch.equal(res2.confusion, res.confusion)
    assert torch.equal(_bits(res2.ap_fixed), _bits(res.ap_fixed))
