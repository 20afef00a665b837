"""Soft-NMS and box voting on the device (postprocess.merge_detections(method=, vote_thresh=), csrc/merge.hip:
merge_soft_kernel, merge_vote_kernel) against the host restatement `postprocess.merge_soft_numpy`.

Hard and linear, with and without voting: everything bit for bit -- both sides perform the same IEEE operations in the
same order, so no margin condition applies, ties included. Gaussian: the discrete outputs (group, row, votes, counts,
offsets) are equal, after asserting the restatement's pick and drop margins >= 1e-4, and each score is within a relative
L * 2**-23 of the restatement's, L the length of that list's concatenation (<= 80 here: <= 9.6e-6): each update differs from
the restatement's by at most one fp32 rounding, because the two double exp implementations agree to within 1 ulp of a
double, and a row receives fewer than L updates. Voted coordinates are bit for bit under every method: the double sums are
ordered and weighted by the original scores. The cases and the cached references are tests/soft_merge_cases.py's."""
import numpy as np
import pytest
import torch

import soft_merge_cases as C
from dana_amd import _lib, ops, postprocess as PP
from dana_amd.config import cfg

pytestmark = pytest.mark.gpu


def _pack(lists, dev):
    """host lists -> (packed device buffer, host int32 counts, offsets)"""
    counts = np.asarray([len(q) for q in lists], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    packed = np.concatenate(lists, 0) if len(lists) else np.zeros((0, 5), np.float32)
    buf = torch.zeros((max(len(packed), 1), 5), dtype=torch.float32, device=dev)
    buf[:len(packed)] = torch.from_numpy(np.ascontiguousarray(packed, np.float32)).to(dev)
    return buf, torch.from_numpy(counts), torch.from_numpy(offsets)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _list_lengths(lists, groups):
    return [sum(len(q) for q in lists[i:i + groups]) for i in range(0, len(lists), groups)]


def _assert_equals(m, ref, lengths, exact_scores=True):
    n = len(ref["dets"])
    assert isinstance(m, PP.MergedDetections) and len(m) == n
    assert m.counts.dtype == torch.int32 and m.offsets.dtype == torch.int32
    assert np.array_equal(m.counts.numpy(), ref["counts"]) and np.array_equal(m.offsets.numpy(), ref["offsets"])
    assert m.layout_dev.cpu().tolist() == ref["counts"].tolist() + ref["offsets"].tolist()
    total = int(ref["offsets"][-1])
    assert m.total == total and m.group.shape == (total,) and m.row.shape == (total,)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if n else np.zeros(0, dt)  # noqa: E731
    assert np.array_equal(m.group.cpu().numpy(), cat(ref["group"], np.int32))
    assert np.array_equal(m.row.cpu().numpy(), cat(ref["row"], np.int32))
    if ref["votes"] is None:
        assert m.votes is None
    else:
        assert m.votes.dtype == torch.int32 and m.votes.is_cuda
        assert np.array_equal(m.votes.cpu().numpy(), cat(ref["votes"], np.int32))
    got = m.packed[:total].cpu().numpy()
    exp = np.concatenate(ref["dets"], 0) if n else np.zeros((0, 5), np.float32)
    assert np.array_equal(_bits(got[:, :4]), _bits(exp[:, :4]))  # coordinates: copies, or ordered double sums
    if exact_scores:
        assert np.array_equal(_bits(got[:, 4]), _bits(exp[:, 4]))
    else:
        for l in range(n):
            a, b = int(ref["offsets"][l]), int(ref["offsets"][l + 1])
            err = np.abs(got[a:b, 4].astype(np.float64) - exp[a:b, 4].astype(np.float64))
            bound = lengths[l] * 2.0 ** -23 * np.abs(exp[a:b, 4].astype(np.float64))
            assert lengths[l] <= 80 and np.all(err <= bound), (l, float((err / np.maximum(bound, 1e-300)).max(initial=0)))
    for l in range(n):
        assert m[l].shape == (int(ref["counts"][l]), 5)


@pytest.mark.parametrize("case,method,vote,variant,vote_score", C.runs(), ids=lambda v: str(v))
def test_device_equals_the_restatement(dev, case, method, vote, variant, vote_score):
    lists, groups = C.CASES[case]
    ref = C.reference(case, method, vote, variant, vote_score)
    if C.needs_margin(method, vote):
        assert ref["margin"]["pick"] >= C.MARGIN and ref["margin"]["drop"] >= C.MARGIN, ref["margin"]
    kw = dict(C.VARIANTS[variant])
    m = PP.merge_detections(_pack(lists, dev), groups, C.THR, with_layout=True, method=method,
                            vote_thresh=C.VOTE if vote else None, vote_score=vote_score, **kw)
    # the Gaussian decay's scores carry the double exp; with vote_score="avg" the score is a function of the original scores again
    _assert_equals(m, ref, _list_lengths(lists, groups), exact_scores=method != "gaussian" or vote_score == "avg")


def test_worked_case_on_the_device(dev):
    A, B, Cc, D = [0, 0, 9, 9, .9], [0, 0, 9, 4, .8], [0, 5, 9, 9, .7], [20, 20, 29, 29, .6]
    lists = [np.asarray([A, B, Cc, D], np.float32)]
    m = PP.merge_detections(_pack(lists, dev), 1, 0.3, method="linear", min_score=0.001, vote_thresh=0.5)
    got = m.packed[:4].cpu().numpy()
    assert [float(s) for s in got[:, 4]] == [0.8999999761581421, 0.6000000238418579, 0.4000000059604645, 0.3499999940395355]
    assert np.array_equal(got[0, :4], np.asarray([0.0, 1.4583334, 9.0, 7.3333335], np.float32))
    assert m.row.cpu().tolist() == [0, 3, 1, 2] and m.votes.cpu().tolist() == [3, 1, 2, 2]
    hard = PP.merge_detections(_pack(lists, dev), 1, 0.3, method="hard", vote_thresh=0.5)
    assert hard.row.cpu().tolist() == [0, 3] and hard.votes.cpu().tolist() == [3, 1]
    assert torch.equal(hard.packed[:2, :4].cpu(), m.packed[:2, :4].cpu())


def test_defaults_make_the_existing_call(dev):
    """method="hard" without voting is dana_detect_merge, and its plain return is still a list"""
    lists, groups = C.CASES["empty_between"]
    plain = PP.merge_detections(_pack(lists, dev), groups, C.THR, method="hard", vote_thresh=None)
    assert type(plain) is list
    ref = C.reference("empty_between", "hard")
    for l, d in enumerate(plain):
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(ref["dets"][l]))
    m = PP.merge_detections(_pack(lists, dev), groups, C.THR, with_layout=True)
    assert m.votes is None and np.array_equal(m.counts.numpy(), ref["counts"])


def test_device_layout_needs_and_uses_capacity(dev):
    lists, groups = C.CASES["empty_middle_group"]
    packed, c, o = _pack(lists, dev)
    with pytest.raises(ValueError, match="capacity"):
        PP.merge_detections((packed, c.to(dev), o.to(dev)), groups, C.THR, method="linear")
    with pytest.raises(ValueError, match="capacity 60 is below the longest concatenation"):
        PP.merge_detections((packed, c, o), groups, C.THR, method="linear", capacity=60)
    for method, vote in (("linear", True), ("gaussian", False), ("hard", True)):
        ref = C.reference("empty_middle_group", method, vote)
        for cap in (70, 83):  # exactly the concatenation, and a padded frame
            m = PP.merge_detections((packed, c.to(dev), o.to(dev)), groups, C.THR, capacity=cap, method=method,
                                    vote_thresh=C.VOTE if vote else None)
            _assert_equals(m, ref, [70], exact_scores=method != "gaussian")


def test_no_lists_and_no_rows(dev):
    packed = torch.zeros((1, 5), device=dev)
    none = PP.merge_detections((packed, torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)), 2,
                               method="linear", vote_thresh=0.5)
    assert len(none) == 0 and none.total == 0 and none.offsets.tolist() == [0] and none.votes.shape == (0,)
    empty = [np.zeros((0, 5), np.float32)] * 6
    for method in ("hard", "linear", "gaussian"):
        m = PP.merge_detections(_pack(empty, dev), 2, C.THR, method=method, vote_thresh=0.5)
        assert m.counts.tolist() == [0, 0, 0] and m.offsets.tolist() == [0, 0, 0, 0] and m.total == 0
    # the C entry point itself: stale output layout is zeroed, nothing is launched
    layout = torch.full((7,), 99, dtype=torch.int32, device=dev)
    _lib.lib().call("dana_detect_merge_soft", None, None, None, 3, 2, 0, 1, C.THR, 0, 0, 1, 0.5, 0.001, 0.5, 0, None, None,
                    None, None, layout.data_ptr(), layout.data_ptr() + 12, None, 0, ops._stream())
    assert layout.cpu().tolist() == [0] * 7


def test_small_workspace_and_large_capacity_are_errors_not_launches(dev):
    lists, groups = C.CASES["empty_between"]
    packed, c, o = _pack(lists, dev)
    L = _lib.lib()
    lay = torch.cat((c, o[:6])).to(dev)
    cap = 70
    out = torch.full((3 * cap, 5), -7.0, device=dev)
    ib = torch.full((9 * cap + 7,), -7, dtype=torch.int32, device=dev)  # group | row | votes | counts [3] | offsets [4]
    nbytes = L.query("dana_detect_merge_soft_workspace_bytes", 3, 2, cap)
    big = L.query("dana_detect_merge_soft_workspace_bytes", 3, 2, 3073)
    ws = ops._ws(max(nbytes, big), dev)

    def args(capacity, nb, method):
        return (packed.data_ptr(), lay.data_ptr(), lay.data_ptr() + 24, 3, 2, capacity, 1, C.THR, 0, 0, method, 0.5, 0.001,
                C.VOTE, 0, out.data_ptr(), ib.data_ptr(), ib.data_ptr() + 12 * cap, ib.data_ptr() + 24 * cap,
                ib.data_ptr() + 36 * cap, ib.data_ptr() + 36 * cap + 12, ws.data_ptr(), nb, ops._stream())

    for method in (0, 1, 2):
        with pytest.raises(_lib.DanaError, match=r"dana_detect_merge_soft: workspace \d+ < %d" % nbytes):
            L.call("dana_detect_merge_soft", *args(cap, nbytes - 1, method))
    for method in (1, 2):
        with pytest.raises(_lib.DanaError, match="capacity 3073 above the 3072 rows the soft-NMS kernel holds in LDS"):
            L.call("dana_detect_merge_soft", *args(3073, big, method))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ib == -7).all())  # nothing was launched
    # ... and with enough of both the same arguments give the restatement's result
    L.call("dana_detect_merge_soft", *args(cap, nbytes, 1))
    ref = C.reference("empty_between", "linear", True)
    host, total = ib.cpu().numpy(), int(ref["offsets"][-1])
    assert host[9 * cap:9 * cap + 3].tolist() == ref["counts"].tolist() and host[9 * cap + 3:].tolist() == ref["offsets"].tolist()
    assert np.array_equal(_bits(out[:total].cpu().numpy()), _bits(np.concatenate(ref["dets"])))
    assert host[6 * cap:6 * cap + total].tolist() == np.concatenate(ref["votes"]).tolist()
    assert bool((out[total:] == -7.0).all())  # nothing was written behind the emitted rows


# ---- end to end -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep(dev):
    """one small model: three shots as three 1-shot sets of a num_shot = 1 model, one 128 x 160 query image"""
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=1, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    im, info, gt, nb, _ = [t.to(dev) for t in S.episode_inputs(1, 1, 1, 128, 160, seed=5)]
    shots = S.episode_inputs(1, 1, 3, 128, 160, seed=7)[4].to(dev)  # [1, 3, 3, 320, 320]
    with torch.no_grad():
        cache = m.encode_supports(shots.view(3, 1, 3, 320, 320))
        rois, cls_prob, bbox_pred = m(im, info, gt, nb, cache.sweep())[:3]
    return dict(info=info, gt=gt, rois=rois, cls_prob=cls_prob, bbox_pred=bbox_pred)


def test_nms_thresh_none_returns_every_row_above_the_threshold(dev, sweep):
    """detections_by_class(nms_thresh=None): each list is the decode of its problem -- dana_detect_postprocess' sorted rows
    above the score threshold, before its NMS -- unsuppressed; the default keyword is cfg.TEST.NMS as before"""
    rois, cls_prob, bbox_pred, info = sweep["rois"], sweep["cls_prob"], sweep["bbox_pred"], sweep["info"]
    R, thresh = rois.size(1), 0.05
    cd = PP.detections_by_class(rois, cls_prob, bbox_pred, info, 3, thresh=thresh, nms_thresh=None, with_layout=True)
    nmsd = PP.detections_by_class(rois, cls_prob, bbox_pred, info, 3, thresh=thresh, with_layout=True)
    same = PP.detections_by_class(rois, cls_prob, bbox_pred, info, 3, thresh=thresh, nms_thresh=cfg.TEST.NMS, with_layout=True)
    assert torch.equal(nmsd.counts, same.counts) and torch.equal(nmsd.packed[:int(nmsd.offsets[3])], same.packed[:int(same.offsets[3])])
    f4 = PP.ctypes.c_float * 4
    more = 0
    for p in range(3):
        dets = torch.empty((R, 5), dtype=torch.float32, device=dev)
        ibuf = torch.empty((R + 2,), dtype=torch.int32, device=dev)
        ws = ops._ws(_lib.lib().query("dana_detect_postprocess_workspace_bytes", R), dev)
        _lib.lib().call("dana_detect_postprocess", ops._p(rois[p].contiguous()), ops._p(cls_prob[p * R:(p + 1) * R].contiguous()),
                        ops._p(bbox_pred[p * R:(p + 1) * R].contiguous()), ops._p(info.reshape(-1)[:3].float().contiguous()), R,
                        PP.ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_STDS), PP.ctypes.c_void_p),
                        PP.ctypes.cast(f4(*cfg.TRAIN.BBOX_NORMALIZE_MEANS), PP.ctypes.c_void_p),
                        int(bool(cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)), thresh, float(cfg.TEST.NMS), 0, ops._p(dets),
                        ibuf.data_ptr(), ibuf.data_ptr() + 4 * R, ops._p(ws), ws.numel(), ops._stream())
        n_valid = int(ibuf[R])
        fg = cls_prob[p * R:(p + 1) * R, 1]
        assert n_valid == int((fg > thresh).sum()) == int(cd.counts[p])
        assert torch.equal(cd[0][p], dets[:n_valid])  # the rows and their (stable, descending) order
        s = cd[0][p][:, 4].cpu()
        assert torch.equal(s, torch.sort(fg[fg > thresh].cpu(), descending=True, stable=True)[0])
        more += int(cd.counts[p]) - int(nmsd.counts[p])
    assert more > 0  # the NMS had removed something
    bat = PP.detections_batched(rois, cls_prob, bbox_pred, info.expand(3, -1), thresh=thresh, nms_thresh=None)
    assert all(torch.equal(a, b) for a, b in zip(bat, cd[0]))


def test_soft_ensemble_end_to_end(dev, sweep):
    """sweep -> detections_by_class -> ensemble_shots(method="linear", vote_thresh=0.8) equals the restatement over the same
    three per-shot lists read back; as_gt_boxes of it equals gt_boxes_numpy of the restatement; the evaluator takes it"""
    from dana_amd.evaluate import DetectionEvaluator
    info, gt = sweep["info"], sweep["gt"]
    cd = PP.detections_by_class(sweep["rois"], sweep["cls_prob"], sweep["bbox_pred"], info, num_classes=3, with_layout=True)
    per_shot = [d.cpu().numpy() for d in cd[0]]
    L = sum(len(d) for d in per_shot)
    assert L > 0
    ref = PP.merge_soft_numpy(per_shot, 3, cfg.TEST.NMS, method="linear", vote_thresh=0.8)
    ens = PP.ensemble_shots(cd, 3, method="linear", vote_thresh=0.8)
    assert len(ens) == 1 and len(ens[0]) == 1 and ens.num_classes == 1
    flat = PP.merge_detections(cd, 3, with_layout=True, method="linear", vote_thresh=0.8)
    _assert_equals(flat, ref, [L])
    assert np.array_equal(_bits(ens[0][0].cpu().numpy()), _bits(ref["dets"][0]))
    assert ens.group.cpu().tolist() == ref["group"][0].tolist() and ens.row.cpu().tolist() == ref["row"][0].tolist()
    assert ens.votes.cpu().tolist() == ref["votes"][0].tolist() and ens.total == len(ref["dets"][0])
    # soft-NMS keeps what the hard ensemble deletes, and K shots vote more than once somewhere
    assert ens.total >= PP.ensemble_shots(cd, 3).total and int(ens.votes.max()) >= 1
    scale = info[:, 2].cpu().numpy()
    for thr in (0.5, 0.05):
        gt_boxes, num = PP.as_gt_boxes(ens, info, 1, thr)
        ref_gt, ref_num = PP.gt_boxes_numpy(ref["dets"], scale, 1, thr, cfg.MAX_NUM_GT_BOXES)
        assert num.cpu().tolist() == ref_num.tolist() and np.array_equal(_bits(gt_boxes.cpu().numpy()), _bits(ref_gt))
    ev = DetectionEvaluator(1, device=dev)
    ev.add_ground_truth(0, gt[0, :3, :4], [0, 0, 0])
    ev.add_by_class(ens, [0])
    res = ev.compute()
    assert ev.num_rows == ens.total and res.ap.shape[0] == 1
    # soft-NMS in place of the per-class NMS: unsuppressed lists, one group per list
    raw = PP.detections_by_class(sweep["rois"], sweep["cls_prob"], sweep["bbox_pred"], info, 3, nms_thresh=None, with_layout=True)
    assert int(raw.counts.max()) > int(cd.counts.max())
    soft = PP.merge_detections(raw, 1, method="linear")
    ref1 = PP.merge_soft_numpy([d.cpu().numpy() for d in raw[0]], 1, cfg.TEST.NMS, method="linear")
    _assert_equals(soft, ref1, [int(c) for c in raw.counts])
