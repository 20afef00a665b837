"""The error diagnosis on the host (dana_amd/diagnose.py: `tide_numpy`, `diagnose_min_iou_margin`, `all_boxes_arrays`, the
argument checks): the hand-worked cases of tests/diagnose_cases.py, step 1 bit-equal to `voc_numpy`, an independent
per-detection brute force, the invariants the rules imply, and the refusals. No GPU."""
import os

import numpy as np
import pytest

import diagnose_cases as DC
from dana_amd import _lib, diagnose as D, evaluate as E

HAND = DC.hand_cases()

RANDOM = {
    "mixed": lambda s: DC.random_case(s, 6, 4, lambda i: [0, 1, 3, 5, 8, 2][i], lambda c, i: 5),
    "one_class": lambda s: DC.random_case(s, 5, 1, lambda i: 3, lambda c, i: 9),
    "tied": lambda s: DC.random_case(s, 4, 3, lambda i: 4, lambda c, i: 8, tie_scores=True),
    "stray": lambda s: DC.random_case(s, 4, 3, lambda i: 3, lambda c, i: 4, stray=5),
    "all_difficult": lambda s: DC.random_case(s, 3, 2, lambda i: 3, lambda c, i: 4, difficult=2.0),
    "crowded": lambda s: DC.random_case(s, 2, 5, lambda i: 70, lambda c, i: 30 if c == 1 else 3),
    "contested": lambda s: DC.contested_case(s),
}


def _nan_close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(
        (np.abs(a - b)[~np.isnan(b)] <= tol).all())


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    case, e = HAND[name]["args"], HAND[name]["expect"]
    r = DC.host(case)
    for k in ("order", "cls_offsets", "det_type", "det_ref", "gt_state", "counts", "confusion", "npos"):
        assert np.array_equal(r[k], np.asarray(e[k])), (k, r[k])
    assert _nan_close(r["ap"], e["ap"]), r["ap"]
    for o, k in enumerate(D.ORACLE_NAMES):
        assert _nan_close(r["ap_fixed"][o], e["ap_fixed"][k]), (k, r["ap_fixed"][o])
        if k in e["delta_map"]:
            assert _nan_close(r["delta_map"][o], e["delta_map"][k]), (k, r["delta_map"][o])
    assert _nan_close(r["mean_ap"], e["mean_ap"])
    assert _nan_close(r["delta_ap"], r["ap_fixed"] - r["ap"][None, :], 0.)


def test_hand_case_under_the_11_point_metric():
    # six_types, use_07_metric: class 0's curve is recall 0.5 at precision 1 -> 6 of the 11 points (0.0 .. 0.5) see 1;
    # under the Loc oracle the other five see 2/3
    r = DC.host(HAND["six_types"]["args"], use_07_metric=True)
    assert _nan_close(r["ap"], [6. / 11., 0.])
    assert _nan_close(r["ap_fixed"][1], [6. / 11. + 5. * (2. / 3.) / 11., 0.])
    assert _nan_close(r["ap_fixed"][7], [1., np.nan])


def _step1_equal(case, t_f, use07):
    r = DC.host(case, t_f, 0.1, use07)
    v = E.voc_numpy(*[case[k] for k in DC.ARG_NAMES], [t_f], use07)
    for k in ("order", "cls_offsets", "npos"):
        assert np.array_equal(r[k], v[k]), k
    assert np.array_equal(r["tpfp"], v["tpfp"][0])
    assert np.array_equal(r["ap"].view(np.int64), v["ap"][:, 0].copy().view(np.int64))  # bit for bit, NaN included


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_step_one_is_voc_numpy(name):
    case = DC.find_case(RANDOM[name], 100)
    _step1_equal(case, 0.5, False)
    _step1_equal(case, 0.5, True)


def test_step_one_is_voc_numpy_on_the_fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "eval_voc.npz")))
    case = dict({k: g[k] for k in DC.ARG_NAMES[:7]}, n_img=int(g["n_img"]), n_cls=int(g["n_cls"]))
    _step1_equal(case, 0.5, False)
    _step1_equal(case, 0.7, True)


def _iou(b, g):
    """voc_eval's IoU on Python floats"""
    iw = max(min(g[2], b[2]) - max(g[0], b[0]) + 1., 0.)
    ih = max(min(g[3], b[3]) - max(g[1], b[1]) + 1., 0.)
    inters = iw * ih
    uni = (b[2] - b[0] + 1.) * (b[3] - b[1] + 1.) + (g[2] - g[0] + 1.) * (g[3] - g[1] + 1.) - inters
    return inters / uni


def _brute_force(case, t_f=0.5, t_b=0.1):
    """Types, refs and states BY DETECTION ROW from plain loops: the greedy marking of step 1 with its own bookkeeping of
    which object each TP took, then one double loop per false positive."""
    det = [[float(x) for x in row] for row in case["det"]]
    gt = [[float(x) for x in row] for row in case["gt_box"]]
    n_img, n_cls = case["n_img"], case["n_cls"]
    d_img, d_cls = [int(x) for x in case["det_img"]], [int(x) for x in case["det_cls"]]
    g_img, g_cls = [int(x) for x in case["gt_img"]], [int(x) for x in case["gt_cls"]]
    diff = [bool(x) for x in case["gt_difficult"]]
    g_ok = [0 <= g_cls[j] < n_cls and 0 <= g_img[j] < n_img for j in range(len(gt))]
    d_ok = [0 <= d_cls[i] < n_cls and 0 <= d_img[i] < n_img for i in range(len(det))]
    types, refs = [0] * len(det), [-1] * len(det)
    state = [3 if g_ok[j] and not diff[j] else 0 for j in range(len(gt))]
    taken = set()
    fps = []
    for c in range(n_cls):
        rows = sorted((i for i in range(len(det)) if d_ok[i] and d_cls[i] == c), key=lambda i: (-det[i][4], i))
        for i in rows:
            best, bj = -np.inf, -1
            for j in range(len(gt)):
                if g_ok[j] and g_cls[j] == c and g_img[j] == d_img[i]:
                    v = _iou(det[i], gt[j])
                    if v > best:
                        best, bj = v, j
            if best > t_f and diff[bj]:
                continue  # code 0
            if best > t_f and bj not in taken:
                taken.add(bj)
                types[i], refs[i], state[bj] = DC.TP, bj, 1
            else:
                fps.append(i)
    for i in fps:
        same, js, other, jo = -np.inf, -1, -np.inf, -1
        for j in range(len(gt)):
            if state[j] == 0 or g_img[j] != d_img[i]:
                continue
            v = _iou(det[i], gt[j])
            if g_cls[j] == d_cls[i]:
                if v > same:
                    same, js = v, j
            elif v > other:
                other, jo = v, j
        if same > t_f:
            types[i], refs[i] = DC.DUPE, js
        elif same >= t_b:
            types[i], refs[i] = DC.LOC, js
        elif other > t_f:
            types[i], refs[i] = DC.CLS, jo
        elif other >= t_b:
            types[i], refs[i] = DC.BOTH, jo
        else:
            types[i] = DC.BKG
    for i in fps:
        if types[i] in (DC.LOC, DC.CLS) and state[refs[i]] == 3:
            state[refs[i]] = 2
    return np.asarray(types), np.asarray(refs), np.asarray(state)


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_against_the_brute_force(name):
    case = DC.find_case(RANDOM[name], 200)
    r = DC.host(case)
    types, refs, state = _brute_force(case)
    n = case["det"].shape[0]
    by_row_type, by_row_ref = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    by_row_type[r["order"]], by_row_ref[r["order"]] = r["det_type"], r["det_ref"]
    assert np.array_equal(by_row_type, types)
    assert np.array_equal(by_row_ref, refs)
    assert np.array_equal(r["gt_state"], state)
    if name not in ("all_difficult", "contested"):  # (contested holds TP, Dupe and Cls by construction)
        assert len(set(types.tolist())) >= 4, "the case exercises too few types: %s" % sorted(set(types.tolist()))


@pytest.mark.parametrize("name", sorted(RANDOM))
@pytest.mark.parametrize("use07", [False, True], ids=["area", "07"])
def test_invariants(name, use07):
    case = DC.find_case(RANDOM[name], 300)
    r = DC.host(case, use_07_metric=use07)
    C, n = case["n_cls"], case["det"].shape[0]
    valid = int(r["cls_offsets"][-1])
    rank_cls = case["det_cls"][r["order"]]
    # every in-range detection has exactly one type (0 exactly where step 1 says "difficult"), the others none
    assert ((r["det_type"][:valid] == 0) == (r["tpfp"][:valid] == 0)).all() and (r["det_type"][valid:] == 0).all()
    assert ((r["det_type"] == DC.TP) == (r["tpfp"] == 1)).all() and r["det_type"].max(initial=0) <= 6
    # every counted object has exactly one state
    gok = (case["gt_cls"] >= 0) & (case["gt_cls"] < C) & (case["gt_img"] >= 0) & (case["gt_img"] < case["n_img"])
    counted = gok & (case["gt_difficult"] == 0)
    assert ((r["gt_state"] > 0) == counted).all() and r["gt_state"].max(initial=0) <= 3
    # counts and confusion agree with the per-row outputs and with each other
    for c in range(C):
        for ty in range(1, 7):
            assert r["counts"][c, ty - 1] == int(((r["det_type"][:valid] == ty) & (rank_cls[:valid] == c)).sum())
        assert r["counts"][c, 6] == int(((r["gt_state"] == 3) & (case["gt_cls"] == c)).sum())
        assert r["confusion"][c, C] == int(((r["gt_state"] >= 2) & (case["gt_cls"] == c)).sum())
        assert r["confusion"][:, c].sum() == r["counts"][c, :6].sum()  # column margin: the class's typed detections
        assert r["confusion"][c, c] == r["counts"][c, 0]
        assert r["confusion"][C, c] == r["counts"][c, 2:6].sum()
        assert r["counts"][c, 0] == int(((r["gt_state"] == 1) & (case["gt_cls"] == c)).sum())  # one TP per detected object
        assert r["npos"][c] == r["counts"][c, 0] + r["confusion"][c, C]
    assert r["confusion"][:C, :C].sum() - np.trace(r["confusion"][:C, :C]) == r["counts"][:, 1].sum() and r["confusion"][C, C] == 0
    # refs: a TP's and a Dupe's object is detected, a Cls ref is of another class, a Loc ref of the same
    ref = r["det_ref"]
    for ty in (DC.TP, DC.DUPE):
        assert (r["gt_state"][ref[r["det_type"] == ty]] == 1).all()
    assert (case["gt_cls"][ref[r["det_type"] == DC.CLS]] != rank_cls[r["det_type"] == DC.CLS]).all()
    assert (case["gt_cls"][ref[r["det_type"] == DC.LOC]] == rank_cls[r["det_type"] == DC.LOC]).all()
    assert (ref[(r["det_type"] == DC.BKG) | (r["det_type"] == 0)] == -1).all()
    # no oracle lowers an AP
    fin = np.isfinite(r["ap_fixed"])
    assert (r["ap_fixed"][fin] >= np.broadcast_to(r["ap"], r["ap_fixed"].shape)[fin] - 1e-12).all()
    assert (r["delta_map"][np.isfinite(r["delta_map"])] >= -1e-12).all()
    assert np.isfinite(r["ap_fixed"][:5]).all(0).tolist() == (r["npos"] > 0).tolist()  # these oracles leave npos alone


def test_contested_case_is_contested():
    case = DC.find_case(DC.contested_case, 7)
    r = DC.host(case)
    cls_rows = r["det_type"] == DC.CLS
    rank_cls = case["det_cls"][r["order"]]
    assert cls_rows.sum() >= 100 and np.unique(rank_cls[cls_rows & (r["det_ref"] == 0)]).size >= 3
    # object 1 (the last class, no detections of its own) is undetected and covered: the Cls oracle gives its class an AP of 1
    assert r["gt_state"].tolist() == [1, 2] and r["ap"][-1] == 0. and r["ap_fixed"][0][-1] == 1.0
    # object 0 is detected: its many Cls claimants are removed, none moves
    assert r["ap_fixed"][0][0] == r["ap"][0]


def test_min_iou_margin():
    a = HAND["six_types"]["args"]
    m = DC.margin(a)  # the closest: IoU 1/3 against 0.5 -> 1/6; IoU 0 against 0.1 -> 0.1
    assert abs(m - 0.1) <= 1e-15
    a2 = dict(a, det=np.asarray([[0, 0, 99, 199, .9]], np.float32), det_img=a["det_img"][:1], det_cls=np.asarray([1], np.int32))
    assert DC.margin(a2) == 0.0  # IoU with A0 is exactly 0.5, whatever the class: all classes are looked at
    assert DC.margin(dict(a2, det_img=np.asarray([5], np.int32))) == np.inf  # out of range: no part


def test_all_boxes_layout():
    case = DC.find_case(RANDOM["mixed"], 400)
    C, n_img = case["n_cls"], case["n_img"]
    all_boxes = [[[] for _ in range(n_img)] for _ in range(C)]
    for c in range(C):
        for i in range(n_img):
            rows = case["det"][(case["det_cls"] == c) & (case["det_img"] == i)]
            if rows.shape[0]:
                all_boxes[c][i] = rows
    gts = []
    for i in range(n_img):
        sel = case["gt_img"] == i
        gts.append((case["gt_box"][sel], case["gt_cls"][sel], case["gt_difficult"][sel]) if i % 2 else
                   (case["gt_box"][sel], case["gt_cls"][sel]) if not case["gt_difficult"][sel].any() else
                   (case["gt_box"][sel], case["gt_cls"][sel], case["gt_difficult"][sel]))
    a = D.all_boxes_arrays(all_boxes, gts)
    assert a["n_img"] == n_img and a["n_cls"] == C and a["det"].shape[0] == case["det"].shape[0]
    assert (np.diff(a["det_cls"]) >= 0).all()  # class by class, image by image
    r, ref = DC.host(a), DC.host(case)
    for k in ("counts", "confusion", "npos", "gt_state"):  # (the objects keep their order; the detections' ranks may not)
        assert np.array_equal(r[k], ref[k]), k
    assert _nan_close(r["ap_fixed"], ref["ap_fixed"], 0.) and _nan_close(r["ap"], ref["ap"], 0.)
    one = D.all_boxes_arrays(all_boxes, gts, add_one=True)
    assert np.array_equal(one["det"][:, :4], a["det"][:, :4] + 1.) and np.array_equal(one["det"][:, 4], a["det"][:, 4])
    empty = D.all_boxes_arrays([[[]], [[]]], [(np.zeros((0, 4)), [])])
    assert empty["det"].shape == (0, 5) and empty["gt_box"].shape == (0, 4) and empty["n_cls"] == 2 and empty["n_img"] == 1
    with pytest.raises(ValueError):
        D.all_boxes_arrays([[[]]], [(np.zeros((2, 4)), [0])])


def test_argument_checks():
    for t_f, t_b in ((0.5, 0.5), (0.5, 0.6), (0.5, -0.1), (float("nan"), 0.1), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            D.DetectionDiagnoser(3, t_f=t_f, t_b=t_b)  # refused before any device is touched
        with pytest.raises(ValueError):
            DC.host(HAND["six_types"]["args"], t_f, t_b)
    with pytest.raises(ValueError):
        D.DetectionDiagnoser(0)
    q = _lib.lib().query
    assert q("dana_diagnose_errors_workspace_bytes", 1000, 100, 50, 20) > 0
    assert q("dana_diagnose_errors_workspace_bytes", 1 << 20, 100, 50, 20) > q("dana_diagnose_errors_workspace_bytes", 1000, 100, 50, 20)
    for bad in ((-1, 4, 3, 2), (8, -1, 3, 2), (8, 4, 0, 2), (8, 4, 3, 0), (8, 4, 1 << 20, 1 << 12), (8, 4, 1, 1 << 15),
                ((1 << 30) + 1, 4, 3, 2)):
        assert q("dana_diagnose_errors_workspace_bytes", *bad) == 0, bad
    names = [a for _, a in _lib.lib().protos["dana_diagnose_errors"][1]]
    assert names[:13] == ["det", "det_img", "det_cls", "n", "gt_box", "gt_img", "gt_cls", "gt_difficult", "g", "n_img",
                          "n_cls", "thresholds", "use_07_metric"]
    ok = [None, None, None, 0, None, None, None, None, 0, 1, 1, 8, 0, None, 8, None, 8, 8, None, None, None, 8, 8, 8, 8, 1 << 20,
          None]
    for at, v in ((3, -1), (8, -1), (9, 0), (10, 0), (11, None), (24, None), (3, 5), (8, 5), (25, 16)):
        args = list(ok)
        args[at] = v
        with pytest.raises(_lib.DanaError):  # every refusal comes before the first launch
            _lib.lib().call("dana_diagnose_errors", *args)
