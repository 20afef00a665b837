"""View ensembles on the device (csrc/views.hip: dana_detect_fold_views through postprocess.fold_views / ensemble_views,
pipeline.plan_views through the existing assembler) against the host restatements.

The fold is compared with `postprocess.fold_views_numpy` bit for bit -- both sides perform the same IEEE fp32 operations --
on the seeded lists of tests/views_cases.py: rows, counts_out, offsets_out and src_row_out; rows behind a list's kept count
are unwritten and not compared. Chained with the merge, hard and linear agree bit for bit with `merge_soft_numpy` on
fold_views_numpy's lists, and Gaussian under test_gpu_soft_merge.py's bar (L * 2**-23 relative on scores, L <= 80), after
asserting the restatement's margins, which test_views_host.py has verified for exactly these cases."""
import numpy as np
import pytest
import torch

import soft_merge_cases as C
import views_cases as VC
from dana_amd import _lib, ops, pipeline as PL, postprocess as PP

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ---- the fold against its restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_src", [True, False], ids=["src_row", "no_src_row"])
@pytest.mark.parametrize("name", sorted(VC.FOLD_SHAPES))
def test_fold_equals_the_restatement(dev, name, with_src):
    B, V, Cn = VC.FOLD_SHAPES[name]
    lists, table, packed, counts, offsets = VC.fold_inputs(name)
    ref = VC.fold_reference(name)
    P, rows = len(lists), len(packed)
    d_in = torch.from_numpy(packed).to(dev)
    lay = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    out = torch.full((rows, 5), SENTINEL, device=dev)
    ibuf = torch.full((2 * P + rows,), int(SENTINEL), dtype=torch.int32, device=dev)  # counts | offsets | src_row

    def run():
        _lib.lib().call("dana_detect_fold_views", d_in.data_ptr(), lay.data_ptr(), lay.data_ptr() + 4 * P, B, V, Cn,
                        d_table.data_ptr(), VC.STRIDE, out.data_ptr(), ibuf.data_ptr(), ibuf.data_ptr() + 4 * P,
                        ibuf.data_ptr() + 8 * P if with_src else None, ops._stream())
        return out.cpu().numpy(), ibuf.cpu().numpy()

    got, ints = run()
    assert np.array_equal(d_in.cpu().numpy().view(np.int32), packed.view(np.int32))  # the input is only read
    c_out, o_out, src = ints[:P], ints[P:2 * P], ints[2 * P:]
    assert c_out.tolist() == ref["counts"].tolist()
    assert o_out.tolist() == [int(offsets[p]) for p in ref["source"]]  # offsets_out[q] = offsets_in[p]
    written = np.zeros(rows, bool)
    for q, p in enumerate(ref["source"]):
        a, k = int(offsets[p]), int(ref["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(ref["dets"][q])), (q, p)
        if with_src:
            assert src[a:a + k].tolist() == ref["src_row"][q].tolist(), (q, p)
        written[a:a + k] = True
    # nothing is written outside the kept rows: not behind a list's kept count, not in the gaps between the lists
    assert np.all(got[~written] == SENTINEL) and np.all(src[~written] == int(SENTINEL))
    if not with_src:
        assert np.all(src == int(SENTINEL))
    # two runs give the same bytes
    got2, ints2 = run()
    assert np.array_equal(_bits(got), _bits(got2)) and np.array_equal(ints, ints2)


def _cd(lists, n_images, Cn, dev):
    """host lists in problem order -> what detections_by_class(..., with_layout=True) returns for them"""
    counts = np.asarray([len(q) for q in lists], np.int32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    flat = np.concatenate(lists, 0) if len(lists) else np.zeros((0, 5), np.float32)
    packed = torch.zeros((max(len(flat), 1), 5), dtype=torch.float32, device=dev)
    packed[:len(flat)] = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(dev)
    views = [packed[int(offsets[p]):int(offsets[p + 1])] for p in range(len(lists))]
    cd = PP.ClassDetections([views[b * Cn:(b + 1) * Cn] for b in range(n_images)])
    cd.packed, cd.counts, cd.offsets, cd.num_classes = packed, torch.from_numpy(counts), torch.from_numpy(offsets), Cn
    cd.layout_dev = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    return cd


def _views(table, B, V):
    return PL.ViewSet(B, V, table[:, :5], np.ones(B * V), np.zeros(B * V))


@pytest.mark.parametrize("name", sorted(VC.FOLD_SHAPES))
def test_fold_views_returns_the_restatement(dev, name):
    """the Python entry on the contiguous layout detections_by_class writes: device counts / offsets, src_row, capacity"""
    B, V, Cn = VC.FOLD_SHAPES[name]
    lists, table = VC.fold_inputs(name)[:2]
    ref = VC.fold_reference(name)
    cd = _cd(lists, B * V, Cn, dev)
    folded = PP.fold_views(cd, _views(table, B, V))
    assert folded.counts.is_cuda and folded.offsets.is_cuda and folded.src_row.is_cuda and folded.layout_dev is None
    assert folded.packed.data_ptr() != cd.packed.data_ptr() and (folded.n_images, folded.views, folded.num_classes) == (B, V, Cn)
    assert folded.counts.cpu().tolist() == ref["counts"].tolist()
    assert folded.offsets.cpu().tolist() == [int(cd.offsets[p]) for p in ref["source"]]
    got, src = folded.packed.cpu().numpy(), folded.src_row.cpu().numpy()
    for q, p in enumerate(ref["source"]):
        a, k = int(cd.offsets[p]), int(ref["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(ref["dets"][q])) and src[a:a + k].tolist() == ref["src_row"][q].tolist()
    per_list = np.asarray([len(q) for q in lists]).reshape(B, V, Cn).sum(1)
    assert folded.capacity == int(per_list.max()) >= int(ref["counts"].reshape(B * Cn, V).sum(1).max())
    with pytest.raises(ValueError, match="images in the detections"):
        PP.fold_views(cd, _views(np.concatenate((table, table)), 2 * B, V))


# ---- identity --------------------------------------------------------------------------------------------------------------

def test_one_unmirrored_view_is_merge_detections(dev):
    """V = 1, no flip, no window, frames larger than every box: ensemble_views is merge_detections(cd, 1)"""
    lists, groups = C.CASES["empty_between"]  # six lists, two of them empty
    B, Cn = 3, 2
    cd = _cd(lists, B, Cn, dev)
    table = np.asarray([[4000.0, 3000.0, 0, -np.inf, np.inf]] * B, np.float32)
    ens = PP.ensemble_views(cd, _views(table, B, 1))
    ref = PP.merge_detections(cd, 1, with_layout=True)
    assert isinstance(ens, PP.MergedDetections) and len(ens) == B and all(len(r) == Cn for r in ens) and ens.num_classes == Cn
    assert torch.equal(ens.counts, ref.counts) and torch.equal(ens.offsets, ref.offsets) and ens.total == ref.total > 0
    assert torch.equal(ens.packed[:ens.total], ref.packed[:ref.total])
    assert torch.equal(ens.group, ref.group) and torch.equal(ens.row, ref.row) and ens.votes is None
    assert int(ens.group.max()) == 0
    for b in range(B):
        for c in range(Cn):
            assert torch.equal(ens[b][c], ref[b * Cn + c])
    # ... and the folded rows it merged are the input's own bits
    assert torch.equal(ens.folded.packed[:int(cd.offsets[-1])], cd.packed[:int(cd.offsets[-1])])


# ---- chained with the merge ----------------------------------------------------------------------------------------------

def _assert_merged(m, ref, B, Cn, lengths, exact_scores):
    n = B * Cn
    assert isinstance(m, PP.MergedDetections) and len(m) == B and m.num_classes == Cn
    assert np.array_equal(m.counts.numpy(), ref["counts"]) and np.array_equal(m.offsets.numpy(), ref["offsets"])
    total = int(ref["offsets"][-1])
    cat = lambda xs: np.concatenate(xs).astype(np.int32)  # noqa: E731
    assert m.total == total and np.array_equal(m.group.cpu().numpy(), cat(ref["group"]))
    assert np.array_equal(m.row.cpu().numpy(), cat(ref["row"]))
    if ref.get("votes") is None:
        assert m.votes is None
    else:
        assert np.array_equal(m.votes.cpu().numpy(), cat(ref["votes"]))
    got, exp = m.packed[:total].cpu().numpy(), np.concatenate(ref["dets"], 0)
    assert np.array_equal(_bits(got[:, :4]), _bits(exp[:, :4]))  # coordinates: copies of folded rows, or ordered double sums
    if exact_scores:
        assert np.array_equal(_bits(got[:, 4]), _bits(exp[:, 4]))
    else:
        for l in range(n):
            a, b = int(ref["offsets"][l]), int(ref["offsets"][l + 1])
            err = np.abs(got[a:b, 4].astype(np.float64) - exp[a:b, 4].astype(np.float64))
            bound = lengths[l] * 2.0 ** -23 * np.abs(exp[a:b, 4].astype(np.float64))
            assert lengths[l] <= 80 and np.all(err <= bound), (l, float((err / np.maximum(bound, 1e-300)).max(initial=0)))
    for l in range(n):
        assert m[l // Cn][l % Cn].shape == (int(ref["counts"][l]), 5)


@pytest.mark.parametrize("method,vote", VC.CHAINED_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(VC.CHAINED))
def test_ensemble_views_equals_fold_then_merge_restated(dev, name, method, vote):
    lists, table, B, V, Cn = VC.chained_inputs(name)
    folded = VC.folded_reference(name)
    ref = VC.chained_reference(name, method, vote)
    if C.needs_margin(method, vote):
        assert ref["margin"]["pick"] >= C.MARGIN and ref["margin"]["drop"] >= C.MARGIN, ref["margin"]
    lengths = [int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn)]
    cd = _cd(lists, B * V, Cn, dev)
    ens = PP.ensemble_views(cd, _views(table, B, V), C.THR, method=method, vote_thresh=VC.VOTE if vote else None)
    _assert_merged(ens, ref, B, Cn, lengths, exact_scores=method != "gaussian")
    assert set(ens.group.cpu().tolist()) == set(range(V))  # every view contributes, the mirrored ones included
    if method == "hard" and not vote:  # ... and the float64 merge agrees where its margin holds
        ref64 = PP.merge_numpy(folded["dets"], V, C.THR)
        assert ref64["margin"] >= C.MARGIN
        _assert_merged(ens, ref64, B, Cn, lengths, exact_scores=True)


# ---- through the model ---------------------------------------------------------------------------------------------------

MEANS = np.array([102.9801, 115.9465, 122.7717], dtype=np.float32)
FRAMES = [(96, 128, []), (120, 90, []), ("flip", 0, []), ("flip", 1, [])]
SCALES = (64, 96)


@pytest.fixture(scope="module")
def assembled(dev):
    from test_gpu_episode_assembler import make_pool
    pool, src = make_pool(dev, FRAMES, seed=3)
    plan, views = PL.plan_views(pool, [(0, 2), (1, 3)], scales=SCALES, flip=True)
    H, W = plan.holder_hw
    hold = PL.EpisodeHolders(plan.batch, 1, 0, H, W, dev, support_size=32, max_num_box=4)
    for t in hold.tensors()[:4]:
        t.fill_(7)
    out = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS).assemble(plan)
    return dict(pool=pool, src=src, plan=plan, views=views, out=out)


def test_assembled_views_are_the_per_image_path(dev, assembled):
    plan, views, src, out = (assembled[k] for k in ("plan", "views", "src", "out"))
    im_data, im_info, gt, nb = out[:4]
    H, W = plan.holder_hw
    assert (views.n_images, views.views, plan.batch) == (2, 4, 8) and (H, W) == (128, 128) and im_data.shape == (8, 3, H, W)
    b = 0
    for row, twin in ((0, 2), (1, 3)):
        frame = torch.from_numpy(src[row][0]).to(dev)
        for s in SCALES:
            for f in (False, True):
                assert src[twin if f else row][1] == f
                ref, scale = PL.prep_im_for_blob(frame, MEANS, target_size=s, flipped=f)
                want = torch.zeros((3, H, W), device=dev)
                want[:, :ref.size(0), :ref.size(1)] = ref.permute(2, 0, 1)
                assert torch.equal(im_data[b], want), b
                assert im_info[b].cpu().tolist() == [float(H), float(W), float(np.float32(scale))]
                b += 1
    assert int(nb.sum()) == 0 and float(gt.abs().max()) == 0  # views carry no ground truth
    assert views.table[:, :3].tolist() == [[128, 96, f, ] for _ in SCALES for f in (0, 1)] + [[90, 120, f] for _ in SCALES for f in (0, 1)]


def test_views_through_the_model(dev, assembled):
    from test_gpu_support_cache import _episode, _model, _sets
    from dana_amd import program
    from dana_amd.evaluate import CocoEvaluator
    from dana_amd.config import cfg
    views = assembled["views"]
    im_data, im_info, gt, nb = assembled["out"][:4]
    m, _ = _model(dev)
    with torch.no_grad():
        cache = m.encode_supports(_sets(_episode(dev, 2)[4]))
        rois, cls_prob, bbox_pred = m(im_data, im_info, gt, nb, cache.sweep())[:3]
    Cn, V, B = len(cache), views.views, views.n_images
    assert Cn == 2 and rois.size(0) == B * V * Cn
    cd = PP.detections_by_class(rois, cls_prob, bbox_pred, im_info, Cn, with_layout=True, nms_thresh=None)
    assert int(cd.counts.sum()) > 0 and V * rois.size(1) <= 3072
    ens = PP.ensemble_views(cd, views, method="linear", vote_thresh=0.8)
    # the numpy chain on cd's own lists read back
    lists = [cd[b][c].cpu().numpy() for b in range(B * V) for c in range(Cn)]
    folded = PP.fold_views_numpy(lists, views.table, V, Cn)
    ref = PP.merge_soft_numpy(folded["dets"], V, cfg.TEST.NMS, method="linear", vote_thresh=0.8)
    lengths = [int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn)]
    _assert_merged(ens, ref, B, Cn, lengths, exact_scores=True)
    assert ens.total > 0 and int(ens.votes.max()) >= 1
    # the fold it merged is the restatement's, and src_row leads back into cd's lists
    got, src = ens.folded.packed.cpu().numpy(), ens.folded.src_row.cpu().numpy()
    for q, p in enumerate(folded["source"]):
        a, k = int(cd.offsets[p]), int(folded["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(folded["dets"][q])) and src[a:a + k].tolist() == folded["src_row"][q].tolist()
    # every output box lies inside its frame (voted boxes are means of boxes inside it); group is a view index
    box = ens.packed[:ens.total].cpu().numpy()
    for i in range(B):
        fw, fh = views.table[i * V, 0], views.table[i * V, 1]
        a, b = int(ens.offsets[i * Cn]), int(ens.offsets[(i + 1) * Cn])
        d = box[a:b]
        if not len(d):
            continue
        assert d[:, 0].min() >= 0 and d[:, 1].min() >= 0 and d[:, 2].max() <= fw - 1 and d[:, 3].max() <= fh - 1
        assert np.all(d[:, 0] <= d[:, 2]) and np.all(d[:, 1] <= d[:, 3])
    g = ens.group.cpu().numpy()
    assert g.min() >= 0 and g.max() < V
    # something was mirrored back: the mirrored views' lists differ from their folded form
    assert any(not np.array_equal(lists[p][folded["src_row"][q]][:, 0], folded["dets"][q][:, 0])
               for q, p in enumerate(folded["source"]) if views.table[p // Cn, 2])
    # the evaluator and the pseudo-label path take the result unchanged
    ev = CocoEvaluator(Cn, device=dev)
    for i in range(B):
        ev.add_ground_truth(i, [[10, 10, 30, 30]], [0])
    ev.add_by_class(ens, list(range(B)))
    assert ev.num_rows == ens.total
    info_lists = torch.tensor([[views.table[l // Cn * V, 1], views.table[l // Cn * V, 0], 1.0] for l in range(B * Cn)], device=dev)
    gt_boxes, num = PP.as_gt_boxes(ens, info_lists, 1, 0.05)
    ref_gt, ref_num = PP.gt_boxes_numpy(ref["dets"], np.ones(B * Cn, np.float32), 1, 0.05, cfg.MAX_NUM_GT_BOXES)
    assert num.cpu().tolist() == ref_num.tolist() and np.array_equal(_bits(gt_boxes.cpu().numpy()), _bits(ref_gt))
    # recorded into a LaunchProgram (which refuses any device-to-host read): one C-ABI entry and no torch op
    p = program.LaunchProgram(dev)
    with p.recording():
        again = PP.fold_views(cd, views)
    assert p.stats["launches"] == 1 and p.stats["torch_ops"] == 0
    assert torch.equal(again.counts, ens.folded.counts) and torch.equal(again.offsets, ens.folded.offsets)
