"""Tiled inference on the device (csrc/views.hip: dana_detect_fold_tiles through postprocess.fold_tiles / ensemble_views,
pipeline.plan_tiles through the existing assembler) against the host restatements.

The tile fold is compared with `postprocess.fold_tiles_numpy` bit for bit -- both sides perform the same IEEE fp32 operations
-- on the seeded lists of tests/tiles_cases.py: rows, counts_out, offsets_out and src_row_out; rows behind a list's kept count
are unwritten and not compared. Chained with the merge, hard and linear agree bit for bit with `merge_soft_numpy` on
fold_tiles_numpy's lists, and Gaussian under test_gpu_soft_merge.py's bar (L * 2**-23 relative on scores, L <= 80), after
asserting the restatement's margins, which test_tiles_host.py has verified for exactly these cases."""
import numpy as np
import pytest
import torch

import soft_merge_cases as C
import tiles_cases as TC
from dana_amd import _lib, ops, pipeline as PL, postprocess as PP
from test_gpu_views import SENTINEL, _assert_merged, _bits, _cd, _views

pytestmark = pytest.mark.gpu


# ---- the fold against its restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_src", [True, False], ids=["src_row", "no_src_row"])
@pytest.mark.parametrize("name", sorted(TC.FOLD_SHAPES))
def test_tile_fold_equals_the_restatement(dev, name, with_src):
    B, V, Cn = TC.FOLD_SHAPES[name]
    lists, table, packed, counts, offsets, _ = TC.fold_inputs(name)
    ref = TC.fold_reference(name)
    P, rows = len(lists), len(packed)
    d_in = torch.from_numpy(packed).to(dev)
    lay = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    out = torch.full((rows, 5), SENTINEL, device=dev)
    ibuf = torch.full((2 * P + rows,), int(SENTINEL), dtype=torch.int32, device=dev)  # counts | offsets | src_row

    def run():
        _lib.lib().call("dana_detect_fold_tiles", d_in.data_ptr(), lay.data_ptr(), lay.data_ptr() + 4 * P, B, V, Cn,
                        d_table.data_ptr(), TC.STRIDE, out.data_ptr(), ibuf.data_ptr(), ibuf.data_ptr() + 4 * P,
                        ibuf.data_ptr() + 8 * P if with_src else None, ops._stream())
        return out.cpu().numpy(), ibuf.cpu().numpy()

    got, ints = run()
    assert np.array_equal(d_in.cpu().numpy().view(np.int32), packed.view(np.int32))  # the input is only read
    assert np.array_equal(d_table.cpu().numpy().view(np.int32), table.view(np.int32))
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


def _tiles(table, B, V):
    return PL.TileSet(B, V, table[:, :13], np.ones(B * V), np.zeros(B * V), np.zeros((B * V, 4)))


@pytest.mark.parametrize("name", sorted(TC.FOLD_SHAPES))
def test_fold_tiles_returns_the_restatement(dev, name):
    """the Python entry on the contiguous layout detections_by_class writes: device counts / offsets, src_row, capacity"""
    B, V, Cn = TC.FOLD_SHAPES[name]
    lists, table = TC.fold_inputs(name)[:2]
    ref = TC.fold_reference(name)
    cd = _cd(lists, B * V, Cn, dev)
    folded = PP.fold_tiles(cd, _tiles(table, B, V))
    assert isinstance(folded, PP.FoldedViews)
    assert folded.counts.is_cuda and folded.offsets.is_cuda and folded.src_row.is_cuda and folded.layout_dev is None
    assert folded.packed.data_ptr() != cd.packed.data_ptr() and (folded.n_images, folded.views, folded.num_classes) == (B, V, Cn)
    assert folded.counts.cpu().tolist() == ref["counts"].tolist()
    assert folded.offsets.cpu().tolist() == [int(cd.offsets[p]) for p in ref["source"]]
    got, src = folded.packed.cpu().numpy(), folded.src_row.cpu().numpy()
    for q, p in enumerate(ref["source"]):
        a, k = int(cd.offsets[p]), int(ref["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(ref["dets"][q])) and src[a:a + k].tolist() == ref["src_row"][q].tolist()
    # the capacity comes from the INPUT counts, an upper bound of the folded concatenation
    per_list = np.asarray([len(q) for q in lists]).reshape(B, V, Cn).sum(1)
    assert folded.capacity == int(per_list.max()) >= int(ref["counts"].reshape(B * Cn, V).sum(1).max())
    with pytest.raises(ValueError, match="fold_tiles: .* images in the detections"):
        PP.fold_tiles(cd, _tiles(np.concatenate((table, table)), 2 * B, V))


# ---- chained with the merge ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,vote", TC.CHAINED_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(TC.CHAINED))
def test_ensemble_views_folds_a_tile_set_with_the_tile_fold(dev, name, method, vote):
    lists, table, B, V, Cn = TC.chained_inputs(name)
    folded = TC.folded_reference(name)
    ref = TC.chained_reference(name, method, vote)
    if C.needs_margin(method, vote):
        assert ref["margin"]["pick"] >= C.MARGIN and ref["margin"]["drop"] >= C.MARGIN, ref["margin"]
    lengths = [int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn)]
    cd = _cd(lists, B * V, Cn, dev)
    ens = PP.ensemble_views(cd, _tiles(table, B, V), C.THR, method=method, vote_thresh=TC.VOTE if vote else None)
    _assert_merged(ens, ref, B, Cn, lengths, exact_scores=method != "gaussian")
    assert set(ens.group.cpu().tolist()) == set(range(V))  # every view index occurs: the tiles and the mirrored ones
    assert ens.folded.counts.cpu().tolist() == folded["counts"].tolist()
    if method == "hard" and not vote:  # ... and the float64 merge agrees where its margin holds
        ref64 = PP.merge_numpy(folded["dets"], V, C.THR)
        assert ref64["margin"] >= C.MARGIN
        _assert_merged(ens, ref64, B, Cn, lengths, exact_scores=True)


@pytest.mark.parametrize("name", sorted(TC.CHAINED))
def test_a_plain_view_set_still_takes_the_view_fold(dev, name):
    """the dispatch: the same lists with a ViewSet of the table's first five columns are folded by dana_detect_fold_views --
    no tile test, no seam rule, no translation -- and merged as before"""
    lists, table, B, V, Cn = TC.chained_inputs(name)
    cd = _cd(lists, B * V, Cn, dev)
    views = _views(table, B, V)
    ens = PP.ensemble_views(cd, views, C.THR, method="linear", vote_thresh=TC.VOTE)
    f = PP.fold_views(cd, views)
    ref = PP.merge_detections(f, V, C.THR, with_layout=True, capacity=f.capacity, method="linear", vote_thresh=TC.VOTE)
    plain = TC.plain_views_reference(name)
    assert ens.folded.counts.cpu().tolist() == plain["counts"].tolist() != TC.folded_reference(name)["counts"].tolist()
    assert torch.equal(ens.counts, ref.counts) and torch.equal(ens.offsets, ref.offsets) and ens.total == ref.total > 0
    assert torch.equal(ens.packed[:ens.total], ref.packed[:ref.total])
    assert torch.equal(ens.group, ref.group) and torch.equal(ens.row, ref.row) and torch.equal(ens.votes, ref.votes)
    got = ens.folded.packed.cpu().numpy()
    for q, p in enumerate(plain["source"]):
        a, k = int(cd.offsets[p]), int(plain["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(plain["dets"][q]))


# ---- through the assembler and the model ---------------------------------------------------------------------------------

MEANS = np.array([102.9801, 115.9465, 122.7717], dtype=np.float32)
FRAMES = [(96, 128, []), (120, 90, []), ("flip", 0, []), ("flip", 1, [])]
TILING = dict(grid=(2, 2), scale=96, overlap=16, margin=2, flip=True, full_frame=64)  # test_tiles_host.py's hand-worked plan


def _assemble(dev, pool, rows):
    plan, tiles = PL.plan_tiles(pool, rows, **TILING)
    H, W = plan.holder_hw
    hold = PL.EpisodeHolders(plan.batch, 1, 0, H, W, dev, support_size=32, max_num_box=4)
    for t in hold.tensors()[:4]:
        t.fill_(7)
    return plan, tiles, PL.EpisodeAssembler(pool, hold, pixel_means=MEANS).assemble(plan)


@pytest.fixture(scope="module")
def pooled(dev):
    from test_gpu_episode_assembler import make_pool
    pool, src = make_pool(dev, FRAMES, seed=3)
    return dict(pool=pool, src=src)


def test_assembled_tiles_are_crops_of_the_prepared_frame(dev, pooled):
    pool, src = pooled["pool"], pooled["src"]
    plan, tiles, out = _assemble(dev, pool, [(0, 2), (1, 3)])
    im_data, im_info, gt, nb = out[:4]
    H, W = plan.holder_hw
    assert (tiles.n_images, tiles.views, plan.batch) == (2, 10, 20) and (H, W) == (85, 85) and im_data.shape == (20, 3, H, W)
    b = 0
    for row, twin in ((0, 2), (1, 3)):
        frame = torch.from_numpy(src[row][0]).to(dev)
        for t in range(5):
            for f in (False, True):
                assert src[twin if f else row][1] == f
                ref, scale = PL.prep_im_for_blob(frame, MEANS, target_size=64 if t == 0 else 96, flipped=f)
                y_s, x_s, ch, cw = tiles.windows[b].tolist()
                if t == 0:
                    assert (y_s, x_s, ch, cw) == (0, 0, ref.size(0), ref.size(1))
                else:
                    assert ch < ref.size(0) and cw < ref.size(1) and y_s + ch <= ref.size(0) and x_s + cw <= ref.size(1)
                want = torch.zeros((3, H, W), device=dev)
                want[:, :ch, :cw] = ref[y_s:y_s + ch, x_s:x_s + cw].permute(2, 0, 1)
                assert torch.equal(im_data[b], want), b
                assert im_info[b].cpu().tolist() == [float(H), float(W), float(np.float32(scale))]
                b += 1
    assert int(nb.sum()) == 0 and float(gt.abs().max()) == 0  # tiles carry no ground truth
    # the four tiles of a view together read every pixel of the prepared frame, and the last ones end at its far sides
    assert tiles.windows[8].tolist() == [40, 56, 56, 72] and tiles.windows[18].tolist() == [56, 40, 72, 56]


def test_tiles_through_the_model(dev, pooled):
    from test_gpu_support_cache import _episode, _model, _sets
    from dana_amd import program
    from dana_amd.evaluate import CocoEvaluator
    from dana_amd.config import cfg
    plan, tiles, out = _assemble(dev, pooled["pool"], [(0, 2)])  # one frame and its twin: 10 view images
    im_data, im_info, gt, nb = out[:4]
    m, _ = _model(dev)
    with torch.no_grad():
        cache = m.encode_supports(_sets(_episode(dev, 2)[4]))
        rois, cls_prob, bbox_pred = m(im_data, im_info, gt, nb, cache.sweep())[:3]
    Cn, V, B = len(cache), tiles.views, tiles.n_images
    assert (B, V, Cn) == (1, 10, 2) and rois.size(0) == B * V * Cn
    cd = PP.detections_by_class(rois, cls_prob, bbox_pred, im_info, Cn, with_layout=True, nms_thresh=None)
    assert int(cd.counts.sum()) > 0 and V * rois.size(1) <= 3072
    ens = PP.ensemble_views(cd, tiles, method="linear", vote_thresh=0.8)
    # the numpy chain on cd's own lists read back
    lists = [cd[b][c].cpu().numpy() for b in range(B * V) for c in range(Cn)]
    folded = PP.fold_tiles_numpy(lists, tiles.table, V, Cn)
    ref = PP.merge_soft_numpy(folded["dets"], V, cfg.TEST.NMS, method="linear", vote_thresh=0.8)
    lengths = [int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn)]
    _assert_merged(ens, ref, B, Cn, lengths, exact_scores=True)
    assert ens.total > 0 and int(ens.votes.max()) >= 1
    got, src = ens.folded.packed.cpu().numpy(), ens.folded.src_row.cpu().numpy()
    for q, p in enumerate(folded["source"]):
        a, k = int(cd.offsets[p]), int(folded["counts"][q])
        assert np.array_equal(_bits(got[a:a + k]), _bits(folded["dets"][q])) and src[a:a + k].tolist() == folded["src_row"][q].tolist()
    # every output box lies inside its frame (voted boxes are means of boxes inside it); group is a view index
    d = ens.packed[:ens.total].cpu().numpy()
    fw, fh = tiles.table[0, 0], tiles.table[0, 1]
    assert d[:, 0].min() >= 0 and d[:, 1].min() >= 0 and d[:, 2].max() <= fw - 1 and d[:, 3].max() <= fh - 1
    assert np.all(d[:, 0] <= d[:, 2]) and np.all(d[:, 1] <= d[:, 3])
    g = ens.group.cpu().numpy()
    assert g.min() >= 0 and g.max() < V
    # a kept row came from an unmirrored tile with an x offset, and the fold moved it by that offset
    moved = [(q, p) for q, p in enumerate(folded["source"])
             if tiles.table[p // Cn, 5] > 0 and not tiles.table[p // Cn, 2] and len(folded["dets"][q])]
    assert moved and all(np.all(folded["dets"][q][:, 0] != lists[p][folded["src_row"][q]][:, 0]) for q, p in moved)
    assert any(np.array_equal(folded["dets"][q][:, 0], np.clip(lists[p][folded["src_row"][q]][:, 0], 0, None) + tiles.table[p // Cn, 5])
               for q, p in moved)
    # the evaluator and the pseudo-label path take the result unchanged
    ev = CocoEvaluator(Cn, device=dev)
    ev.add_ground_truth(0, [[10, 10, 30, 30]], [0])
    ev.add_by_class(ens, [0])
    assert ev.num_rows == ens.total
    info_lists = torch.tensor([[fh, fw, 1.0]] * Cn, device=dev)
    gt_boxes, num = PP.as_gt_boxes(ens, info_lists, 1, 0.05)
    ref_gt, ref_num = PP.gt_boxes_numpy(ref["dets"], np.ones(B * Cn, np.float32), 1, 0.05, cfg.MAX_NUM_GT_BOXES)
    assert num.cpu().tolist() == ref_num.tolist() and np.array_equal(_bits(gt_boxes.cpu().numpy()), _bits(ref_gt))
    # recorded into a LaunchProgram (which refuses any device-to-host read): one C-ABI entry and no torch op
    p = program.LaunchProgram(dev)
    with p.recording():
        again = PP.fold_tiles(cd, tiles)
    assert p.stats["launches"] == 1 and p.stats["torch_ops"] == 0
    assert torch.equal(again.counts, ens.folded.counts) and torch.equal(again.offsets, ens.folded.offsets)
