"""Proposal recall on the host (dana_amd/evaluate.py: `proposal_recall_numpy`, the tables behind
`ProposalRecallEvaluator`, `ProposalRecallResult.from_counts`, the argument checks of dana_eval_proposal_recall): hand-worked
cases with their answers written out, the numpy restatement against an independent sorted sweep (tests/recall_cases.py),
the host bookkeeping and the refusals. No GPU."""
import numpy as np
import pytest
import torch

import recall_cases as RC
from dana_amd import _lib, evaluate as E

HAND = RC.hand_cases()
KEYS = ("ov", "match", "hits", "npos", "pair_gt")


def _same(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k  # ov: equal doubles, bit for bit (no NaN in it)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    case = HAND[name]
    e = case["expect"]
    for fn in (E.proposal_recall_numpy, RC.recall_by_sorted_sweep):
        r = fn(**case["args"])
        assert np.array_equal(r["ov"], np.asarray(e["ov"], np.float64)), (fn.__name__, r["ov"])
        assert np.array_equal(r["match"], np.asarray(e["match"], np.int64)), (fn.__name__, r["match"])
        assert np.array_equal(r["hits"], RC.dense(e["hits"], r["hits"].shape)), fn.__name__
        assert np.array_equal(r["npos"], RC.dense(e["npos"], r["npos"].shape)), fn.__name__
        if "pair_gt" in e:
            assert r["pair_gt"].tolist() == e["pair_gt"]
    r = E.proposal_recall_numpy(**case["args"])
    for key, v in e.get("recalls", {}).items():
        assert r["recalls"][key] == v and r["ar"][key[0], key[2], key[3]] == v  # one threshold: ar is that recall


def test_shared_best_is_not_the_per_object_maximum():
    a = HAND["shared_best"]["args"]
    r = E.proposal_recall_numpy(**a)
    per_object = E._iou_matrix(a["boxes"].astype(np.float64), a["gt_box"].astype(np.float64)).max(0)
    assert (per_object >= 0.82).sum() == 2 and r["hits"][0, 1, 0, 0, 0] == 1 and r["recalls"][0, 1, 0, 0] == 0.5


SEEDED = {
    "geometry": lambda: RC.geometry_case(),
    "quantised": lambda: RC.seeded_case(21, [(40, 12), (7, 9), (3, 5)], n_cls=2, quantum=8., extent=120., others=True,
                                        limits=(0, 5), iou_thrs=(0.25, 0.5, 0.75)),
    "quantised_area": lambda: RC.seeded_case(22, [(30, 10), (12, 20)], n_cls=1, quantum=16., extent=400., with_area=True,
                                             area_rng=None, limits=(3, 0)),
    "full_parameters": RC.full_parameter_case,
    "contested": RC.contested_case,
    "rpn_sized": RC.rpn_sized_case,
    "three_classes": RC.three_class_case,
}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_numpy_restatement_equals_the_sorted_sweep(name):
    a = SEEDED[name]()["args"]
    r = E.proposal_recall_numpy(**a)
    _same(r, RC.recall_by_sorted_sweep(**a))
    assert r["n_pairs"] > 0 and (r["ov"] > 0).any()
    if name.startswith("quantised"):  # exact ties do occur: equal IoUs of one object with two candidates of its list
        u = r["unit_tab"][0]
        m = E._iou_matrix(a["boxes"][u[0]:u[0] + u[1]].astype(np.float64),
                          a["gt_box"][r["pair_gt"][:u[3] - u[2]]].astype(np.float64))
        assert any(np.unique(col[col > 0]).size < (col > 0).sum() for col in m.T)


def test_tables_order_units_and_pairs():
    # ground truth in arrival order: (image, class) = (1,0) (0,2) (0,0) (1,0) (0,2) (0,1); lists: (0,2) 5 rows at 0,
    # (1,0) 3 rows at 5, (0,2) again 0 rows at 8, (2,1) 4 rows at 8 (an image without ground truth)
    g_img, g_cls = [1, 0, 0, 1, 0, 0], [0, 2, 0, 0, 2, 1]
    t = E._recall_tables([0, 1, 0, 2], [2, 0, 2, 1], [5, 3, 0, 4], [0, 5, 8, 8], g_img, g_cls, 3, others=True)
    assert t["gt_order"].tolist() == [2, 5, 1, 4, 0, 3]  # by (image, class), arrival order inside: stable
    assert t["unit_tab"].dtype == np.int32 and t["gt_order"].dtype == np.int32
    assert t["unit_tab"].tolist() == [
        [0, 5, 2, 4, 0, 0, 0, 2, 0], [5, 3, 4, 6, 0, 0, 2, 0, 0], [8, 0, 2, 4, 0, 0, 4, 2, 0], [8, 4, 6, 6, 0, 0, 6, 1, 0],
        [0, 5, 0, 2, 4, 4, 6, 2, 1], [5, 3, 4, 4, 6, 6, 8, 0, 1], [8, 0, 0, 2, 4, 4, 8, 2, 1], [8, 4, 6, 6, 6, 6, 10, 1, 1]]
    assert t["n_pairs"] == 10
    assert t["pair_unit"].tolist() == [0, 0, 1, 1, 2, 2, 4, 4, 6, 6]
    assert t["pair_gt"].tolist() == [1, 4, 0, 3, 1, 4, 2, 5, 2, 5]
    # without others: the first four units and their pairs
    t0 = E._recall_tables([0, 1, 0, 2], [2, 0, 2, 1], [5, 3, 0, 4], [0, 5, 8, 8], g_img, g_cls, 3)
    assert np.array_equal(t0["unit_tab"], t["unit_tab"][:4]) and t0["n_pairs"] == 6
    assert t0["pair_gt"].tolist() == t["pair_gt"].tolist()[:6]
    # nothing at all
    e = E._recall_tables([], [], [], [], [], [], 2, others=True)
    assert e["unit_tab"].shape == (0, 9) and e["n_pairs"] == 0 and e["gt_order"].size == 0


def test_refusals_on_the_host():
    z = np.zeros((2, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.ProposalRecallEvaluator(3, device="cpu")
    with pytest.raises(ValueError, match="1..16"):
        E.ProposalRecallEvaluator(3, iou_thresholds=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match="1..8 limits"):
        E.ProposalRecallEvaluator(3, limits=range(1, 10))
    with pytest.raises(ValueError, match="1..8 limits"):
        E.ProposalRecallEvaluator(3, limits=())
    with pytest.raises(ValueError, match="area ranges"):
        E.ProposalRecallEvaluator(3, area_ranges=np.zeros((9, 2)))
    with pytest.raises(ValueError, match="unknown area range 'tiny'"):
        E.ProposalRecallEvaluator(3, area_ranges=["all", "tiny"])
    with pytest.raises(ValueError, match="unknown area range 8"):
        E.ProposalRecallEvaluator(3, area_ranges=[8])
    with pytest.raises(ValueError, match="num_classes"):
        E.ProposalRecallEvaluator(0)
    ev = E.ProposalRecallEvaluator(3, area_ranges=["large", 1])  # constructing needs no device
    assert ev.params[3] == ("large", "small") and ev.params[2].tolist() == [[96. ** 2, 1e10], [0., 32. ** 2]]
    assert ev.params[1].tolist() == [10, 100, 300, 1000] and np.array_equal(ev.params[0], np.asarray(E.COCO_THRESHOLDS))
    with pytest.raises(ValueError, match="at most 65536"):
        ev.add_proposals(np.zeros((65537, 4), np.float32), [65537], None, 0, 0)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        ev.add_proposals(z, [2], None, 0, 3)
    with pytest.raises(ValueError, match="as many counts"):
        ev.add_proposals(z, [1, 1], None, [0, 1, 2], 0)
    with pytest.raises(ValueError, match="run past"):
        ev.add_proposals(torch.zeros((2, 4)), [2], [1], 0, 0)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        ev.add_ground_truth(0, z, [0, 3])
    with pytest.raises(ValueError, match="2 boxes"):
        ev.add_ground_truth(0, z, [0])
    assert ev.num_rows == 0 and not ev._prob and not ev._gt
    with pytest.raises(ValueError, match="at most 65536"):
        E.proposal_recall_numpy(np.zeros((65537, 4)), [0], [0], [65537], [0], z, [0, 0], [0, 0], 1)
    with pytest.raises(ValueError, match="ground-truth ids"):
        E.proposal_recall_numpy(z, [0], [0], [2], [0], z, [0, 0], [0, 5], 2)


def test_entry_point_validates_arguments_without_a_device():
    P = 0x1000  # never dereferenced: validation comes first
    names = ["boxes", "unit_tab", "n_units", "gt_box", "gt_area", "gt_order", "g", "n_pairs", "n_cls", "iou_thr", "n_thr",
             "limits", "n_limits", "area_rng", "n_area", "ov", "match", "hits", "npos", "workspace", "workspace_bytes",
             "stream"]
    ok = [P, P, 4, P, None, P, 6, 9, 3, P, 10, P, 4, P, 8, P, P, P, P, P, 1 << 30, None]
    assert [a for _, a in _lib.lib().protos["dana_eval_proposal_recall"][1]] == names

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return _lib.lib().call("dana_eval_proposal_recall", *a)

    for key, bads in (("n_thr", (0, 17, -1)), ("n_limits", (0, 9)), ("n_area", (0, 9))):
        for bad in bads:
            with pytest.raises(_lib.DanaError, match=key):
                call(**{key: bad})
    for kw in (dict(n_units=-1), dict(g=-2), dict(n_pairs=-1), dict(n_cls=0), dict(n_pairs=1 << 31)):
        with pytest.raises(_lib.DanaError, match="bad shape"):
            call(**kw)
    with pytest.raises(_lib.DanaError, match="overflow"):
        call(n_cls=1 << 22)
    for name in ("iou_thr", "limits", "area_rng", "hits", "npos", "unit_tab", "gt_box", "gt_order", "ov", "match", "workspace"):
        with pytest.raises(_lib.DanaError, match="null"):
            call(**{name: None})
    with pytest.raises(_lib.DanaError, match="null"):
        call(g=0)
    for name in ("boxes", "gt_box"):
        with pytest.raises(_lib.DanaError, match="16-byte aligned"):
            call(**{name: P + 4})
    with pytest.raises(_lib.DanaError, match="workspace too small"):
        call(workspace_bytes=16)
    q = _lib.lib().query
    base = q("dana_eval_proposal_recall_workspace_bytes", 1 << 20, 1000, 5000, 10, 4, 8)
    assert base >= 5000 * 4 + 4 * 8 * 5000 * 12
    for bad in ((-1, 4, 9, 10, 4, 8), (8, -1, 9, 10, 4, 8), (8, 4, -1, 10, 4, 8), (8, 4, 9, 17, 4, 8), (8, 4, 9, 10, 9, 8),
                (8, 4, 9, 10, 4, 0), (8, 4, 1 << 31, 10, 4, 8)):
        assert q("dana_eval_proposal_recall_workspace_bytes", *bad) == 0
    assert base > q("dana_eval_proposal_recall_workspace_bytes", 1 << 20, 1000, 5000, 10, 1, 1) > 0


def test_recalls_and_ar_from_the_default_thresholds_by_hand():
    # boxes 10 wide at the origin, so that every IoU is a ratio of heights: the list has heights 10, 12, 15, 21, the objects
    # 10, 11, 13, 16, 19, 40. In IoU order: h10 <- row 0 (1), h16 <- row 2 (15/16 = 0.9375), h13 <- row 1 (12/13 = 0.923;
    # h11's 11/12 = 0.917 comes later and finds row 1 taken), h19 <- row 3 (19/21 = 0.905); h11 and h40 find nothing: 0.
    H = lambda h: (0, 0, 9, h - 1)
    case = RC._case([H(10), H(12), H(15), H(21)], [(0, 0, 4)], [(0, 0, H(h)) for h in (10, 11, 13, 16, 19, 40)], 1,
                    iou_thrs=None, limits=(0, 2))
    r = E.proposal_recall_numpy(**case["args"])
    assert r["ov"][0, 0].tolist() == [1.0, 0.0, 12. / 13., 15. / 16., 19. / 21., 0.0]
    assert r["match"][0, 0].tolist() == [0, -1, 1, 2, 3, -1]
    # thresholds .50 .55 .. .90: four hits each (the lowest matched IoU is 0.905); .95: one (the IoU of 1)
    by_hand = [4] * 9 + [1]
    assert len(E.COCO_THRESHOLDS) == 10
    assert r["hits"][0, :, 0, 0, 0].tolist() == by_hand and r["npos"][0, 0, 0] == 6
    assert np.array_equal(r["recalls"][0, :, 0, 0], np.asarray(by_hand) / 6.)
    assert abs(r["ar"][0, 0, 0] - 37. / 60.) < 1e-15
    # a budget of 2 (heights 10, 12): h10 <- row 0 (1), h13 <- row 1 (0.923 beats h11's 0.917), four objects missed
    assert r["ov"][1, 0].tolist() == [1.0, 0.0, 12. / 13., 0.0, 0.0, 0.0]
    assert r["hits"][0, :, 1, 0, 0].tolist() == [2] * 9 + [1]
    assert abs(r["ar"][0, 1, 0] - 19. / 60.) < 1e-15
    assert np.isnan(r["recalls"][1]).all() and np.isnan(r["ar"][1]).all()  # no other units


def test_from_counts_pools_integer_tables():
    a = dict(RC.three_class_case()["args"], n_cls=4)  # class 3 has neither lists nor objects: NaN in the per-class tables
    r = E.proposal_recall_numpy(**a)
    params = E._recall_params(a["iou_thrs"], a["limits"], a["area_rng"])
    hits, npos = torch.from_numpy(r["hits"]), torch.from_numpy(r["npos"])
    res = E.ProposalRecallResult.from_counts(hits, npos, params)
    assert np.array_equal(res.recalls.numpy(), r["recalls"], equal_nan=True)
    assert np.allclose(res.ar.numpy(), r["ar"], rtol=5 * 2. ** -52, atol=0, equal_nan=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = r["hits"] / r["npos"][:, None, None, :, :].astype(np.float64)
    assert np.array_equal(res.per_class_recalls.numpy(), pc, equal_nan=True)
    assert np.isnan(pc).any() and res.per_class_ar.shape == (2, 2, 1, 4)
    sel = res.selectivity().numpy()
    assert sel.shape == (2, 1) and np.allclose(sel, r["ar"][0] / r["ar"][1], rtol=1e-14)
    # two ranks' counts summed: the pooled recall is the ratio of the sums, not the mean of the ratios
    b = RC.seeded_case(15, [(25, 6)], n_cls=3, others=True, iou_thrs=(0.3, 0.5, 0.7), limits=(0, 10))["args"]
    r2 = E.proposal_recall_numpy(**dict(b, n_cls=4))
    pooled = E.ProposalRecallResult.from_counts(hits + torch.from_numpy(r2["hits"]), npos + torch.from_numpy(r2["npos"]), params)
    want = (r["hits"] + r2["hits"]).sum(-1) / (r["npos"] + r2["npos"]).sum(-1)[:, None, None, :].astype(np.float64)
    assert np.array_equal(pooled.recalls.numpy(), want, equal_nan=True)
    assert pooled.ov is None
    with pytest.raises(ValueError, match="compute"):
        pooled.gt_overlaps(0)
    with pytest.raises(ValueError, match="from_counts"):
        E.ProposalRecallResult.from_counts(hits[:, :2], npos, params)
    # without others the selectivity is NaN
    r0 = E.proposal_recall_numpy(**dict(a, others=False))
    res0 = E.ProposalRecallResult.from_counts(torch.from_numpy(r0["hits"]), torch.from_numpy(r0["npos"]), params)
    assert torch.isnan(res0.selectivity()).all() and not torch.isnan(res0.ar[0]).any()
