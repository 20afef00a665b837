"""Merging detection lists on the device (postprocess.merge_detections / ensemble_shots / cap_per_image / as_gt_boxes,
csrc/merge.hip) against the host restatements `postprocess.merge_numpy` (float64 IoU) and `gt_boxes_numpy`.

Every comparison is bit for bit: the float rows as int32 words, integer equality on counts, offsets, group and row. Each
NMS case first asserts merge_numpy's margin -- the smallest |IoU - threshold| over the decisions it took -- >= 1e-4
(test_gpu_forward_ops.py's bound for the proposal layer), so that no near-tie between the device's fp32 IoU and the
host's fp64 IoU decides anything. The inputs are built so that this holds by construction: boxes come in well separated
clusters of three nested sizes; inside a cluster equal sizes overlap almost completely (IoU > 0.8) and different sizes
hardly (IoU < 0.2), across clusters not at all."""
import os

import numpy as np
import pytest
import torch

from dana_amd import _lib, ops, postprocess as PP
from dana_amd.config import cfg

pytestmark = pytest.mark.gpu

THR = 0.3
SCALES = (1.0, 0.4, 0.15)


def _lists(seed, counts, clusters=None):
    """len(counts) float32 lists [k,5], each in descending score order; scores pairwise distinct over all lists"""
    rng = np.random.RandomState(seed)
    total = int(sum(counts))
    clusters = clusters or max(total // 12, 2)
    cols = int(np.ceil(np.sqrt(clusters)))
    score = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)
    out, at = [], 0
    for k in counts:
        c = rng.randint(0, clusters, k)
        side = 200.0 * np.asarray(SCALES)[rng.randint(0, 3, k)]
        cx = 150.0 + 300.0 * (c % cols) + rng.uniform(-0.01, 0.01, k) * side
        cy = 150.0 + 300.0 * (c // cols) + rng.uniform(-0.01, 0.01, k) * side
        w, h = side * rng.uniform(0.98, 1.02, k), side * rng.uniform(0.98, 1.02, k)
        d = np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score[at:at + k]), 1).astype(np.float32)
        out.append(d[np.argsort(-d[:, 4], kind="stable")])
        at += k
    return out


def _pack(lists, dev, gap=0):
    """host lists -> (packed device buffer, host int32 counts, offsets); `gap` unused rows in front of every list"""
    counts = np.asarray([len(q) for q in lists], np.int32)
    offsets = np.zeros(len(lists) + 1, np.int32)
    rows = [np.full((gap, 5), 7e4, np.float32)] if gap else []
    at = gap
    for i, q in enumerate(lists):
        offsets[i] = at
        rows += [q, np.full((gap, 5), 7e4, np.float32)] if gap else [q]
        at += len(q) + gap
    offsets[-1] = at
    packed = np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32)
    buf = torch.zeros((max(len(packed), 1), 5), dtype=torch.float32, device=dev)
    buf[:len(packed)] = torch.from_numpy(packed).to(dev)
    return buf, torch.from_numpy(counts), torch.from_numpy(offsets)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _assert_equals(m, ref):
    n = len(ref["dets"])
    assert len(m) == n and m.counts.dtype == torch.int32 and m.offsets.dtype == torch.int32
    assert m.counts.tolist() == ref["counts"].tolist() and m.offsets.tolist() == ref["offsets"].tolist()
    assert m.layout_dev.cpu().tolist() == ref["counts"].tolist() + ref["offsets"].tolist()
    total = int(ref["offsets"][-1])
    assert m.total == total and m.group.shape == (total,) and m.row.shape == (total,)
    exp = np.concatenate(ref["dets"], 0) if n else np.zeros((0, 5), np.float32)
    assert np.array_equal(_bits(m.packed[:total].cpu().numpy()), _bits(exp))
    assert torch.equal(m.packed[:total].cpu(), torch.from_numpy(exp))
    assert m.group.cpu().tolist() == (np.concatenate(ref["group"]).tolist() if n else [])
    assert m.row.cpu().tolist() == (np.concatenate(ref["row"]).tolist() if n else [])
    for l in range(n):
        assert torch.equal(m[l].cpu(), torch.from_numpy(ref["dets"][l])), l


def _check(dev, lists, groups, thr=THR, inclusive=False, max_dets=0, capacity=None, gap=0):
    ref = PP.merge_numpy(lists, groups, thr, inclusive, max_dets)
    if thr is not None:
        assert ref["margin"] >= 1e-4, ref["margin"]
    m = PP.merge_detections(_pack(lists, dev, gap), groups, thr, inclusive, max_dets, with_layout=True, capacity=capacity)
    _assert_equals(m, ref)
    return m, ref


@pytest.mark.parametrize("inclusive", [False, True], ids=["gt", "ge"])
def test_one_list_one_group_is_returned_unchanged(dev, inclusive):
    """n_lists = 1, groups = 1: merging one already-NMS'd list gives the list back"""
    nmsd = [PP.merge_numpy(_lists(3, (90,), clusters=20), 1, THR, inclusive)["dets"][0][:37]]
    assert len(nmsd[0]) == 37
    m, ref = _check(dev, nmsd, 1, inclusive=inclusive)
    assert np.array_equal(_bits(ref["dets"][0]), _bits(nmsd[0])) and m.row.cpu().tolist() == list(range(37))


@pytest.mark.parametrize("inclusive", [False, True], ids=["gt", "ge"])
def test_empty_middle_group_and_more_than_one_mask_word(dev, inclusive):
    """n_lists = 1, groups = 3, counts (40, 0, 30): 70 rows cross the 64-bit NMS mask word"""
    _, ref = _check(dev, _lists(5, (40, 0, 30), clusters=30), 3, inclusive=inclusive)
    assert 8 < ref["counts"][0] < 70 and set(ref["group"][0].tolist()) == {0, 2}


def test_all_empty_list_between_two_others(dev):
    """n_lists = 3, groups = 2, counts (5,9 | 0,0 | 64,64): the offsets carry over the empty list; a list of exactly 128 rows"""
    m, ref = _check(dev, _lists(7, (5, 9, 0, 0, 64, 64)), 2)
    assert ref["counts"][1] == 0 and ref["offsets"][1] == ref["offsets"][2] and ref["counts"][0] and ref["counts"][2]
    assert m[1].shape == (0, 5)
    _check(dev, _lists(7, (5, 9, 0, 0, 64, 64)), 2, gap=3)  # the input lists need not be adjacent in the packed buffer


def test_lists_longer_than_a_workgroup_with_padding(dev):
    """n_lists = 2, groups = 5, ~70 rows per group (~350 per list > one 256-thread workgroup), capacity 13 above the need"""
    counts = (70, 66, 74, 69, 71, 73, 68, 70, 72, 65)
    need = max(sum(counts[:5]), sum(counts[5:]))
    _check(dev, _lists(11, counts), 5, capacity=need + 13)
    _check(dev, _lists(11, counts), 5, inclusive=True)


def test_largest_case(dev):
    """n_lists = 2, groups = 4, 300 rows per group: 1 200 rows per list"""
    _, ref = _check(dev, _lists(13, (300,) * 8), 4)
    assert ref["counts"].min() > 128  # the survivors themselves span more than two mask words


def _tie_lists():
    a = _lists(17, (12,), clusters=12)[0]
    a[:, 4] = np.asarray([0.9, 0.9, 0.8, 0.8, 0.8, 0.7, 0.6, 0.6, 0.5, 0.5, 0.5, 0.5], np.float32)  # ties inside a list too
    b = a.copy()  # the same boxes with the same scores in the next group
    c = a.copy()  # ... and equal scores on boxes that overlap nothing
    c[:, :4] += np.float32(5000.0)
    return [a, b, c]


@pytest.mark.parametrize("inclusive", [False, True], ids=["gt", "ge"])
def test_stable_tie_rule(dev, inclusive):
    """duplicated boxes with equal scores across groups: the lower group's row survives under both NMS rules; equal
    scores on disjoint boxes: both survive, in concatenation order"""
    lists = _tie_lists()
    m, ref = _check(dev, lists, 3, inclusive=inclusive)
    assert 1 not in ref["group"][0] and {0, 2} == set(ref["group"][0].tolist())
    g, s = ref["group"][0], ref["dets"][0][:, 4]
    for i in range(len(g) - 1):
        if s[i] == s[i + 1]:
            assert (g[i], ref["row"][0][i]) < (g[i + 1], ref["row"][0][i + 1])
    _check(dev, lists, 3, thr=None)  # NMS off: the pure stable merge, 36 rows
    _check(dev, lists + lists[::-1], 3, inclusive=inclusive)  # two lists, the second with the groups the other way round


@pytest.mark.parametrize("which", ["1", "K-1", "K", "K+7", "0"])
def test_max_dets(dev, which):
    lists = _lists(7, (5, 9, 0, 0, 64, 64))
    K = int(PP.merge_numpy(lists, 2, THR)["counts"][2])
    assert K > 8
    md = {"1": 1, "K-1": K - 1, "K": K, "K+7": K + 7, "0": 0}[which]
    _, ref = _check(dev, lists, 2, max_dets=md)
    assert ref["counts"][2] == (min(K, md) if md else K)


def test_nms_off_with_cap_on_twenty_groups(dev):
    """the max_per_image cut: 20 class lists per image, no NMS, the best 100 rows"""
    counts = tuple(3 + (7 * i) % 11 for i in range(40))
    lists = _lists(19, counts)
    m, ref = _check(dev, lists, 20, thr=None, max_dets=100)
    assert ref["counts"].tolist() == [100, 100] and len(set(ref["group"][0].tolist())) > 10
    # ... and spelled as cap_per_image on a ClassDetections
    packed, c, o = _pack(lists, dev)
    flat = [packed[int(o[p]):int(o[p]) + int(c[p])] for p in range(40)]
    cd = PP.ClassDetections([flat[:20], flat[20:]])
    cd.packed, cd.counts, cd.offsets, cd.num_classes = packed, c, o, 20  # (no layout_dev: uploaded from the host pair)
    capped = PP.cap_per_image(cd, 100)
    _assert_equals(capped, ref)
    assert capped.list_index().tolist() == [0] * 100 + [1] * 100


def test_device_layout_needs_and_uses_capacity(dev):
    lists = _lists(5, (40, 0, 30), clusters=30)
    packed, c, o = _pack(lists, dev)
    with pytest.raises(ValueError, match="capacity"):
        PP.merge_detections((packed, c.to(dev), o.to(dev)), 3)
    m = PP.merge_detections((packed, c.to(dev), o.to(dev)), 3, THR, with_layout=True, capacity=70)
    _assert_equals(m, PP.merge_numpy(lists, 3, THR))
    plain = PP.merge_detections((packed, c, o), 3, THR)
    assert isinstance(plain, list) and len(plain) == 1 and torch.equal(plain[0], m[0])
    assert torch.equal(PP.merge_detections((packed, c, o), 3)[0], PP.merge_detections((packed, c, o), 3, cfg.TEST.NMS)[0])


def test_no_lists_and_no_rows(dev):
    packed = torch.zeros((1, 5), device=dev)
    none = PP.merge_detections((packed, torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)), 2, with_layout=True)
    assert len(none) == 0 and none.total == 0 and none.offsets.tolist() == [0]
    empty = [np.zeros((0, 5), np.float32)] * 6
    m, _ = _check(dev, empty, 2)
    assert m.counts.tolist() == [0, 0, 0] and m.offsets.tolist() == [0, 0, 0, 0]
    # the C entry point itself: stale output layout is zeroed, nothing is launched
    layout = torch.full((7,), 99, dtype=torch.int32, device=dev)
    _lib.lib().call("dana_detect_merge", None, None, None, 3, 2, 0, 1, THR, 0, 0, None, None, None, layout.data_ptr(),
                    layout.data_ptr() + 12, None, 0, ops._stream())
    assert layout.cpu().tolist() == [0] * 7
    torch.cuda.synchronize()


def test_small_workspace_and_small_capacity_are_errors_not_faults(dev):
    lists = _lists(11, (70, 66, 74, 69, 71, 73, 68, 70, 72, 65))
    packed, c, o = _pack(lists, dev)
    need = max(int(c[:5].sum()), int(c[5:].sum()))
    # the wrapper checks capacity on the host, from the caller's counts
    with pytest.raises(ValueError, match="capacity %d is below the longest concatenation" % (need - 9)):
        PP.merge_detections((packed, c, o), 5, THR, capacity=need - 9)
    L = _lib.lib()
    lay = torch.cat((c, o[:10])).to(dev)
    cap = need - 9
    out = torch.zeros((2 * cap, 5), device=dev)
    ib = torch.zeros((4 * cap + 5,), dtype=torch.int32, device=dev)
    nbytes = L.query("dana_detect_merge_workspace_bytes", 2, 5, cap)
    ws = ops._ws(nbytes, dev)
    args = lambda nb: (packed.data_ptr(), lay.data_ptr(), lay.data_ptr() + 40, 2, 5, cap, 1, THR, 0, 0, out.data_ptr(),  # noqa: E731
                       ib.data_ptr(), ib.data_ptr() + 8 * cap, ib.data_ptr() + 16 * cap, ib.data_ptr() + 16 * cap + 8,
                       ws.data_ptr(), nb, ops._stream())
    with pytest.raises(_lib.DanaError, match=r"dana_detect_merge: workspace \d+ < %d" % nbytes):
        L.call("dana_detect_merge", *args(nbytes - 1))
    # the C entry point trusts capacity: a value below the true maximum truncates each concatenation at `capacity` rows
    L.call("dana_detect_merge", *args(nbytes))
    cut = []
    for l in range(2):
        room = cap
        for q in lists[5 * l:5 * l + 5]:
            cut.append(q[:room])
            room -= len(cut[-1])
    ref = PP.merge_numpy(cut, 5, THR)
    assert ref["margin"] >= 1e-4 and sum(len(q) for q in cut[5:]) == cap
    host = ib.cpu().numpy()
    assert host[4 * cap:4 * cap + 2].tolist() == ref["counts"].tolist() and host[4 * cap + 2:].tolist() == ref["offsets"].tolist()
    total = int(ref["offsets"][-1])
    assert np.array_equal(_bits(out[:total].cpu().numpy()), _bits(np.concatenate(ref["dets"])))
    assert host[:total].tolist() == np.concatenate(ref["group"]).tolist()
    assert host[2 * cap:2 * cap + total].tolist() == np.concatenate(ref["row"]).tolist()
    assert not out[total:].any()  # nothing was written behind the survivors


def test_reference_golden_through_the_device(golden_dir, dev):
    """tests/golden/merge_dets.npz: the reference's own chain (utils.py:192-199) with its CPU operator, which suppresses at >="""
    g = np.load(os.path.join(golden_dir, "merge_dets.npz"))
    for i in range(int(g["n_cases"])):
        counts = g["c%d_counts" % i]
        lists = np.split(g["c%d_dets" % i], np.cumsum(counts)[:-1])
        m, _ = _check(dev, lists, len(lists), thr=float(g["nms_thresh"]), inclusive=True)
        assert np.array_equal(_bits(m[0].cpu().numpy()), _bits(g["c%d_out" % i])), i


# ---- as_gt_boxes ------------------------------------------------------------------------------------------------------------

def _gt_lists():
    sorted_list = _lists(23, (8,))[0]
    sorted_list[:, 4] = np.asarray([0.95, 0.9, 0.7, 0.5, 0.5, 0.45, 0.2, 0.1], np.float32)  # two rows AT the threshold
    many = _lists(29, (300,))[0]  # scores 300/301 .. 1/301: 150 above 0.5; more rows than one 256-lane pass
    shuffled = many[np.random.RandomState(1).permutation(300)]  # unsorted: passing rows scattered over every wavefront
    return [sorted_list, np.zeros((0, 5), np.float32), many, shuffled]


@pytest.mark.parametrize("max_boxes", [50, 2, 200])
@pytest.mark.parametrize("labels", ["scalar", "tensor"])
def test_as_gt_boxes_bit_for_bit(dev, max_boxes, labels):
    lists = _gt_lists()
    scale = np.asarray([1.7, 0.6, 2.3, 0.37], np.float32)
    info = torch.tensor([[96., 128., float(s), 5.] for s in scale], device=dev)  # (a fourth column: the row stride is passed on)
    lab = 3 if labels == "scalar" else np.asarray([1., 2., 5., 4.], np.float32)
    ref_gt, ref_num = PP.gt_boxes_numpy(lists, scale, lab, 0.5, max_boxes)
    assert ref_num.tolist() == [min(3, max_boxes), 0, min(150, max_boxes), min(150, max_boxes)]
    gt, num = PP.as_gt_boxes(_pack(lists, dev), info, lab if labels == "scalar" else torch.from_numpy(lab), 0.5, max_boxes)
    assert gt.shape == (4, max_boxes, 5) and gt.dtype == torch.float32 and num.dtype == torch.int64 and num.is_cuda
    assert num.cpu().tolist() == ref_num.tolist()
    assert np.array_equal(_bits(gt.cpu().numpy()), _bits(ref_gt))
    if max_boxes == 50:  # the default is cfg.MAX_NUM_GT_BOXES, the default threshold plot_box's 0.5
        gt2, num2 = PP.as_gt_boxes(_pack(lists, dev), info, lab if labels == "scalar" else torch.from_numpy(lab))
        assert torch.equal(gt2, gt) and torch.equal(num2, num)
    with pytest.raises(ValueError, match="im_info"):
        PP.as_gt_boxes(_pack(lists, dev), info[:3])


def test_as_gt_boxes_feeds_a_train_mode_forward(dev):
    """the layout, not just the numbers: (gt_boxes, num_boxes) go into one train-mode forward of the small model"""
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=1, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).train()
    im, info, _, _, sup = [t.to(dev) for t in S.episode_inputs(1, 2, 1, 128, 160, seed=3)]
    dets = np.asarray([[8., 6., 70., 60., 0.9], [40., 30., 120., 90., 0.8], [5., 50., 50., 94., 0.6], [1., 1., 30., 30., 0.4]],
                      np.float32)
    merged = PP.merge_detections(_pack([dets], dev), 1, None, with_layout=True)
    gt, nb = PP.as_gt_boxes(merged, info)
    assert gt.shape == (1, cfg.MAX_NUM_GT_BOXES, 5) and nb.cpu().tolist() == [3] and gt[0, :3, 4].cpu().tolist() == [1., 1., 1.]
    np.random.seed(0)
    with torch.no_grad():
        out = m(im, info, gt, nb, sup)
    losses = [float(x) for x in out[3:7]]
    assert all(np.isfinite(v) for v in losses) and losses[0] > 0, losses


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_shot_ensemble_end_to_end(dev):
    """three shots as three 1-shot sets of a num_shot = 1 model -> sweep -> detections_by_class -> ensemble_shots equals
    merge_numpy over the three per-shot lists read back; the result goes into the evaluator as it is"""
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.evaluate import DetectionEvaluator
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=1, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    im, info, gt, nb, _ = [t.to(dev) for t in S.episode_inputs(1, 1, 1, 96, 128, seed=5)]
    shots = S.episode_inputs(1, 1, 3, 96, 128, seed=7)[4].to(dev)  # [1, 3, 3, 320, 320]
    with torch.no_grad():
        cache = m.encode_supports(shots.view(3, 1, 3, 320, 320))
        rois, cls_prob, bbox_pred = m(im, info, gt, nb, cache.sweep())[:3]
    cd = PP.detections_by_class(rois, cls_prob, bbox_pred, info, num_classes=3, with_layout=True)
    assert cd.layout_dev.cpu().tolist() == cd.counts.tolist() + cd.offsets.tolist()
    per_shot = [d.cpu().numpy() for d in cd[0]]
    assert sum(len(d) for d in per_shot) > 0
    ref = PP.merge_numpy(per_shot, 3, cfg.TEST.NMS)
    assert ref["margin"] >= 1e-4, ref["margin"]
    ens = PP.ensemble_shots(cd, 3)
    assert len(ens) == 1 and len(ens[0]) == 1 and ens.num_classes == 1
    _assert_equals(PP.merge_detections(cd, 3, with_layout=True), ref)
    assert np.array_equal(_bits(ens[0][0].cpu().numpy()), _bits(ref["dets"][0]))
    assert ens.group.cpu().tolist() == ref["group"][0].tolist() and ens.row.cpu().tolist() == ref["row"][0].tolist()
    ev = DetectionEvaluator(1, device=dev)
    ev.add_ground_truth(0, gt[0, :3, :4], [0, 0, 0])
    ev.add_by_class(ens, [0])
    res = ev.compute()
    assert ev.num_rows == ens.total and res.ap.shape[0] == 1
    with pytest.raises(ValueError, match="multiple of shots"):
        PP.ensemble_shots(cd, 2)
